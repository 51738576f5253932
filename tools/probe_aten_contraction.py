"""Which of ATen's add-with-alpha statements round once (fma) on this device?  Each form of `a + alpha * b` the optimiser steps use
is compared with the two-kernel form (a multiply, then an add: two roundings) and, in float32, with the float64-exact sum rounded
once.  halo_optim.hip's fma / mul + add choices rest on this and on tests/test_gpu_optim.py.

    python tools/probe_aten_contraction.py > profiles/r28_aten_contraction.txt
"""
import torch

if not torch.cuda.is_available():
    raise SystemExit("tools/probe_aten_contraction.py needs a ROCm device")
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(1)
n = 1 << 18
for dtype in (torch.float32, torch.float64):
    a = torch.randn(n, device=dev, dtype=dtype, generator=gen)
    b = torch.randn(n, device=dev, dtype=dtype, generator=gen)
    for s in (0.9, 5e-4, -0.0037, 1 - 0.1):
        prod = b * s                       # one kernel, one rounding
        two = a + prod                     # a second kernel, a second rounding
        forms = {
            "add(alpha)": a.add(b, alpha=s),
            "add_(alpha)": a.clone().add_(b, alpha=s),
            "_foreach_add(alpha)": torch._foreach_add([a.clone()], [b], alpha=s)[0],
            "_foreach_add_(alpha)": None,
            "mul then add (tensor * python scalar, +)": a + (s * b),
        }
        t = [a.clone()]
        torch._foreach_add_(t, [b], alpha=s)
        forms["_foreach_add_(alpha)"] = t[0]
        line = []
        for k, v in forms.items():
            diff_two = (v != two).float().mean().item()
            if dtype == torch.float32:
                s32 = torch.tensor(s, dtype=torch.float32).double().item()
                exact = (a.double() + b.double() * s32).float()          # product exact in double, one rounding but for rare double roundings
                diff_one = (v != exact).float().mean().item()
                line.append("%s: differs from two roundings at %.4f, from one rounding at %.6f" % (k, diff_two, diff_one))
            else:
                line.append("%s: differs from two roundings at %.4f" % (k, diff_two))
        print(str(dtype), "alpha", s)
        for l in line:
            print("   ", l)
print("probe done")
