"""Timing aid: halo_amd.dwconv.depthwise_bn_relu (halo_dwconv.hip) against the three stock statements of DepthwiseSeparableConv2d's
first half -- depthwise 3x3 nn.Conv2d, FrozenBatchNorm2d (x * scale + bias), ReLU(inplace=True) -- under autograd, in the same
process on the same device, float32, at the five blocks of the v3+ head at both training crops (batch 2) and at the B = 1
inference shapes of the target crop:

    aspp6 / aspp12 / aspp18   2 x 2048 x  80 x 160 (target 640 x 1280)   2 x 2048 x  90 x 160 (source 720 x 1280)   d = 6, 12, 18
    dec0                      2 x  560 x 160 x 320                       2 x  560 x 180 x 320                       d = 1
    dec1                      2 x  512 x 160 x 320                       2 x  512 x 180 x 320                       d = 1

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst.  The two sides alternate window by window.  Reported: forward alone (no_grad), forward + backward (gradients
for x and conv.weight), the fused forward's achieved bytes/s against its one-read-one-write traffic, and
torch.cuda.max_memory_allocated over one forward + backward above what the operands hold.

    python tools/time_dwconv.py [--out profiles/r08_time_dwconv.txt] [--n 10] [--repeats 7]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd.dwconv import depthwise_bn_relu, fallback_reason, torch_statement  # noqa: E402

BLOCKS = [("aspp6", 2048, 6, 8), ("aspp12", 2048, 12, 8), ("aspp18", 2048, 18, 8), ("dec0", 560, 1, 4), ("dec1", 512, 1, 4)]   # name, C, d, stride
CROPS = [("target", 640, 1280), ("source", 720, 1280)]


class FrozenBatchNorm2d(nn.Module):
    """the frozen norm of the heads: four buffers, y = x * scale + bias"""

    def __init__(self, n):
        super().__init__()
        for name, v in (("weight", torch.ones(n)), ("bias", torch.zeros(n)), ("running_mean", torch.zeros(n)), ("running_var", torch.ones(n))):
            self.register_buffer(name, v)

    def forward(self, x):
        scale = self.weight * self.running_var.rsqrt()
        bias = self.bias - self.running_mean * scale
        return x * scale.reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)


def windows(fns, n, repeats):
    """per closure the sorted per-call times (ms) of `repeats` windows of n calls; the closures alternate window by window"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / n)
    return [sorted(t) for t in out]


def fmt(t):
    return "%.4f / %.4f / %.4f" % (t[0], t[len(t) // 2], t[-1])


def med(t):
    return t[len(t) // 2]


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_dwconv.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    shapes = [(name, crop, 2, C, ch // s, cw // s, d) for crop, ch, cw in CROPS for name, C, d, s in BLOCKS]
    shapes += [(name, "target/B=1", 1, C, 640 // s, 1280 // s, d) for name, C, d, s in BLOCKS]
    act = nn.ReLU(inplace=True)
    for name, crop, B, C, H, W, d in shapes:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((B, C, H, W), device=dev, generator=gen).requires_grad_(B > 1)
        conv = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False).to(dev)
        bn = FrozenBatchNorm2d(C).to(dev)
        with torch.no_grad():
            bn.weight.copy_(0.25 + 1.5 * torch.rand(C, device=dev, generator=gen))
            bn.bias.copy_(0.4 * torch.randn(C, device=dev, generator=gen))
            bn.running_mean.copy_(0.5 * torch.randn(C, device=dev, generator=gen))
            bn.running_var.copy_(0.3 + 1.5 * torch.rand(C, device=dev, generator=gen))
        assert fallback_reason(x, conv, bn) is None, fallback_reason(x, conv, bn)
        ops = {"fused": lambda t: depthwise_bn_relu(t, conv, bn, act), "stock": lambda t: torch_statement(t, conv, bn, act)}
        sides = {}
        for tag, op in ops.items():
            def fwd(op=op):
                with torch.no_grad():
                    op(x)

            def both(op=op):
                torch.autograd.grad(op(x), [x, conv.weight], g)
            sides[tag] = dict(fwd=fwd, both=both)
        kinds = ("fwd", "both") if B > 1 else ("fwd",)
        g = torch.randn((B, C, H, W), device=dev, generator=gen) if B > 1 else None
        order = [(t, k) for k in kinds for t in ("fused", "stock")]
        times = dict(zip(order, windows([sides[t][k] for t, k in order], args.n, args.repeats)))
        nbytes = x.numel() * 4
        say("%-7s %-10s %s  d = %d  (x: %.0f MB)" % (name, crop, "x".join(map(str, (B, C, H, W))), d, nbytes / 1e6))
        for k, label in (("fwd", "forward"), ("both", "fwd+bwd")):
            if k not in kinds:
                continue
            f, s = times[("fused", k)], times[("stock", k)]
            say("    %-8s fused %s   stock %s   stock/fused (medians) x%.2f%s" % (label, fmt(f), fmt(s), med(s) / med(f),
                                                                                   "" if med(f) <= med(s) else "   FUSED LOSES"))
        say("    fused forward: %.2f TB/s of its one-read-one-write traffic (%.0f MB)" % (2 * nbytes / (med(times[("fused", "fwd")]) * 1e-3) / 1e12,
                                                                                      2 * nbytes / 1e6))
        if B > 1:
            with torch.no_grad():
                diff = float((ops["fused"](x) - ops["stock"](x)).abs().max())
            say("    max |fused - stock| of y = %.3g; peak memory above the operands over one fwd+bwd: fused %.1f MiB, stock %.1f MiB"
                % (diff, peak_mb(sides["fused"]["both"]), peak_mb(sides["stock"]["both"])))
        del sides, times, x, g, conv, bn
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
