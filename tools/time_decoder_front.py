"""Timing aid: halo_amd.dwconv.upsample_cat_depthwise_bn_relu (the halo_upcat_* kernels of halo_dwconv.hip) against the composition a
v3+ head runs at the front of its decoder under use_device_resize + use_fused_depthwise,

    depthwise_bn_relu(torch.cat([resize_or_interpolate(a, (H, W)), s], 1), conv, bn)

under autograd, in the same process on the same device, float32, at the head's shapes:

    target crop 640 x 1280    a 2 x 512 x 80 x 160    s 2 x 48 x 160 x 320
    source crop 720 x 1280    a 2 x 512 x 90 x 160    s 2 x 48 x 180 x 320
    target crop, B = 1        forward only

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst.  The two sides alternate window by window.  Reported: forward alone (no_grad), forward + backward (gradients
for a, s and conv.weight), the byte COUNTS of both sides (from the shapes: nothing here measures traffic), and
torch.cuda.max_memory_allocated over one forward + backward above what the operands hold.  A side "loses" when its median is above
the other's by more than the other's best-to-worst spread.

    python tools/time_decoder_front.py [--out profiles/r11_time_decoder_front.txt] [--n 10] [--repeats 7]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd.dwconv import depthwise_bn_relu, fallback_reason, upcat_fallback_reason, upsample_cat_depthwise_bn_relu  # noqa: E402
from halo_amd.resize import resize_or_interpolate  # noqa: E402
from tools.time_dwconv import FrozenBatchNorm2d, fmt, med, peak_mb, windows  # noqa: E402

SHAPES = [("target", 2, 80, 160, 160, 320), ("source", 2, 90, 160, 180, 320), ("target/B=1", 1, 80, 160, 160, 320)]   # crop, B, h, w, H, W
CA, CS = 512, 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_decoder_front.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    act = nn.ReLU(inplace=True)
    C = CA + CS
    for crop, B, h, w, H, W in SHAPES:
        train = B > 1
        gen = torch.Generator(device=dev).manual_seed(0)
        a = torch.randn((B, CA, h, w), device=dev, generator=gen).requires_grad_(train)
        s = torch.randn((B, CS, H, W), device=dev, generator=gen).requires_grad_(train)
        conv = nn.Conv2d(C, C, 3, 1, 1, 1, groups=C, bias=False).to(dev)
        bn = FrozenBatchNorm2d(C).to(dev)
        with torch.no_grad():
            bn.weight.copy_(0.25 + 1.5 * torch.rand(C, device=dev, generator=gen))
            bn.bias.copy_(0.4 * torch.randn(C, device=dev, generator=gen))
            bn.running_mean.copy_(0.5 * torch.randn(C, device=dev, generator=gen))
            bn.running_var.copy_(0.3 + 1.5 * torch.rand(C, device=dev, generator=gen))
        assert upcat_fallback_reason(a, s, conv, bn) is None, upcat_fallback_reason(a, s, conv, bn)

        def composed(ta, ts):
            x = torch.cat([resize_or_interpolate(ta, (H, W)), ts], 1)
            assert fallback_reason(x, conv, bn) is None
            return depthwise_bn_relu(x, conv, bn, act)

        ops = {"fused": lambda ta, ts: upsample_cat_depthwise_bn_relu(ta, ts, conv, bn, act), "composed": composed}
        g = torch.randn((B, C, H, W), device=dev, generator=gen) if train else None
        sides = {}
        for tag, op in ops.items():
            def fwd(op=op):
                with torch.no_grad():
                    op(a, s)

            def both(op=op):
                torch.autograd.grad(op(a, s), [a, s, conv.weight], g)
            sides[tag] = dict(fwd=fwd, both=both)
        kinds = ("fwd", "both") if train else ("fwd",)
        order = [(t, k) for k in kinds for t in ("fused", "composed")]
        times = dict(zip(order, windows([sides[t][k] for t, k in order], args.n, args.repeats)))
        na, ns, ny = a.numel() * 4, s.numel() * 4, B * C * H * W * 4
        nup = B * CA * H * W * 4
        say("%-10s a %s  s %s" % (crop, "x".join(map(str, a.shape)), "x".join(map(str, s.shape))))
        say("    byte counts (from the shapes, not measured), forward: fused %.0f MB (a %.0f + s %.0f + y %.0f); composed %.0f MB "
            "(resize %.0f + %.0f, cat 2 x %.0f, conv 2 x %.0f)" % ((na + ns + ny) / 1e6, na / 1e6, ns / 1e6, ny / 1e6,
                                                                   (na + nup + ns + nup + ny + 2 * ny) / 1e6, na / 1e6, nup / 1e6, ny / 1e6, ny / 1e6))
        for k, label in (("fwd", "forward"), ("both", "fwd+bwd")):
            if k not in kinds:
                continue
            f, c = times[("fused", k)], times[("composed", k)]
            lost = med(f) - med(c) > c[-1] - c[0]
            say("    %-8s fused %s   composed %s   composed/fused (medians) x%.2f%s" % (label, fmt(f), fmt(c), med(c) / med(f),
                                                                                         "   FUSED LOSES" if lost else ""))
        say("    fused forward: %.2f TB/s of its counted traffic" % ((na + ns + ny) / (med(times[("fused", "fwd")]) * 1e-3) / 1e12))
        if train:
            with torch.no_grad():
                same = torch.equal(ops["fused"](a, s), ops["composed"](a, s))
            say("    y bit-equal: %s; peak memory above the operands over one fwd+bwd: fused %.1f MiB, composed %.1f MiB"
                % (same, peak_mb(sides["fused"]["both"]), peak_mb(sides["composed"]["both"])))
        del sides, times, a, s, g, conv, bn
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
