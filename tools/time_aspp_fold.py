"""Timing aid: the bottleneck stage of a v3+ head with the image-pooling branch folded into the norm + ReLU pass
(halo_amd.aspp.pooled_bottleneck, the halo_pool_fold_* kernels of halo_norm.hip) against the statements a head runs there under
use_device_resize + fuse_norm_relu_pairs,

    bottleneck(torch.cat(branches + [pooled.expand(-1, -1, H, W)], 1))        # conv 3x3 over 2560 channels, fused norm + ReLU

from the four branch outputs (B x 512 x H x W each) and the pooled map (B x 512 x 1 x 1) to the bottleneck's ReLU output (B x 512 x
H x W), under autograd, in the same process on the same device, float32:

    target crop 640 x 1280    B = 2, 80 x 160
    source crop 720 x 1280    B = 2, 90 x 160
    target crop, B = 1        80 x 160

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst.  The two sides alternate window by window.  Reported: forward alone (no_grad), forward + backward (gradients
for the four branch outputs, the pooled map and the conv's weight), and torch.cuda.max_memory_allocated over one forward + backward
above what the operands hold.  The folded stage WINS a shape when its median is below the stock side's by more than the stock
side's own best-to-worst spread; a shape it does not win belongs in halo_amd.aspp.EXCLUDED_SHAPES.  No hardware counters are read.

    python tools/time_aspp_fold.py [--out profiles/r14_time_aspp_fold.txt] [--n 5] [--repeats 7]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd import aspp  # noqa: E402
from halo_amd.hooks import fuse_norm_relu_pairs  # noqa: E402
from tools.time_dwconv import FrozenBatchNorm2d, fmt, med, peak_mb, windows  # noqa: E402

SHAPES = [("target", 2, 80, 160), ("source", 2, 90, 160), ("target/B=1", 1, 80, 160)]   # crop, B, H, W
BRANCHES, CB, CG, CO = 4, 512, 512, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_aspp_fold.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    was = set(aspp.EXCLUDED_SHAPES)
    aspp.EXCLUDED_SHAPES.clear()                 # the measurement decides that list: time every shape on the folded path
    for crop, B, H, W in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        branches = [torch.randn((B, CB, H, W), device=dev, generator=gen).relu_().requires_grad_(True) for _ in range(BRANCHES)]
        pooled = torch.randn((B, CG, 1, 1), device=dev, generator=gen).relu_().requires_grad_(True)
        stage = nn.Sequential(nn.Conv2d(BRANCHES * CB + CG, CO, 3, padding=1, bias=False), FrozenBatchNorm2d(CO), nn.ReLU(inplace=True)).to(dev)
        with torch.no_grad():
            stage[0].weight.mul_(0.3)
            stage[1].weight.copy_(0.25 + 1.5 * torch.rand(CO, device=dev, generator=gen))
            stage[1].bias.copy_(0.4 * torch.randn(CO, device=dev, generator=gen))
            stage[1].running_mean.copy_(0.5 * torch.randn(CO, device=dev, generator=gen))
            stage[1].running_var.copy_(0.3 + 1.5 * torch.rand(CO, device=dev, generator=gen))
        conv, bn, act = stage
        assert fuse_norm_relu_pairs(stage) == 1
        g = torch.randn((B, CO, H, W), device=dev, generator=gen)
        wanted = branches + [pooled, conv.weight]

        def folded():
            p = torch.cat(branches, dim=1)
            assert aspp.pool_fold_fallback_reason(p, pooled, conv, bn, act) is None
            return aspp.pooled_bottleneck(p, pooled, conv, bn, act)

        def stock():
            return stage(torch.cat(branches + [pooled.expand(-1, -1, H, W)], dim=1))

        sides = {}
        for tag, op in (("folded", folded), ("stock", stock)):
            def fwd(op=op):
                with torch.no_grad():
                    op()

            def both(op=op):
                torch.autograd.grad(op(), wanted, g)
            sides[tag] = dict(fwd=fwd, both=both)
        order = [(t, k) for k in ("fwd", "both") for t in ("folded", "stock")]
        times = dict(zip(order, windows([sides[t][k] for t, k in order], args.n, args.repeats)))
        say("%-10s branches %d x %dx%dx%dx%d  pooled %dx%dx1x1" % (crop, BRANCHES, B, CB, H, W, B, CG))
        wins = True
        for k, label in (("fwd", "forward"), ("both", "fwd+bwd")):
            f, s = times[("folded", k)], times[("stock", k)]
            won = med(s) - med(f) > s[-1] - s[0]
            wins = wins and won
            say("    %-8s folded %s   stock %s   stock/folded (medians) x%.3f   stock spread %.4f   %s"
                % (label, fmt(f), fmt(s), med(s) / med(f), s[-1] - s[0], "folded wins" if won else "NO WIN"))
        with torch.no_grad():
            a, b = folded(), stock()
            mag = float(b.abs().max())
            say("    max |folded - stock| %.3g at max |stock| %.3g" % (float((a - b).abs().max()), mag))
            del a, b
        say("    peak memory above the operands over one fwd+bwd: folded %.1f MiB, stock %.1f MiB"
            % (peak_mb(sides["folded"]["both"]), peak_mb(sides["stock"]["both"])))
        say("    verdict: %s" % ("served" if wins else "(%d, %d, %d) belongs in halo_amd.aspp.EXCLUDED_SHAPES" % (B, H, W)))
        del sides, times, branches, pooled, g, stage, conv, bn, act, wanted
        torch.cuda.empty_cache()
    aspp.EXCLUDED_SHAPES.update(was)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
