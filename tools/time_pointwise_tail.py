"""Timing aid: the pointwise tail of the v3+ heads' separable blocks -- FrozenBatchNorm2d, in-place ReLU and, behind decoder[1] of the
hyperbolic head, nn.Dropout2d(0.1) -- as one HIP pass (halo_amd.norm.norm_relu / norm_relu_dropout2d, halo_norm.hip) against torch's
own statements

    F.relu(bn(x), inplace=True)                    drop(F.relu(bn(x), inplace=True))

over the output of the block's 1 x 1 conv, in the same process on the same device, float32:

    decoder tails   512 x 160 x 320 (target crop), 512 x 180 x 320 (source crop)
    ASPP tails      512 x  80 x 160 (target crop), 512 x  90 x 160 (source crop)         each at B = 2 and B = 1

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst.  The two sides alternate window by window.  Three modes: the forward under no_grad, forward + backward of
the tail alone (gradient for x), forward + backward of the tail with the dropout in training mode.  The size rule of the envelope
(halo_amd.norm.AUTOGRAD_MIN_ELEMENTS) is switched off for the run: the measurement decides it.  The fused pass WINS a shape and mode
when its median is below the stock side's by more than the stock side's own best-to-worst spread.  No hardware counters are read.

    python tools/time_pointwise_tail.py [--out profiles/r15_time_pointwise_tail.txt] [--n 5] [--repeats 7]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from halo_amd import norm  # noqa: E402
from tools.time_dwconv import FrozenBatchNorm2d, fmt, med, windows  # noqa: E402

C = 512
PLANES = [("decoder target", 160, 320), ("decoder source", 180, 320), ("ASPP target", 80, 160), ("ASPP source", 90, 160)]
MODES = [("fwd", "forward, no_grad"), ("both", "fwd+bwd"), ("drop", "fwd+bwd, Dropout2d(0.1)")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_pointwise_tail.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    rule = norm.AUTOGRAD_MIN_ELEMENTS
    norm.AUTOGRAD_MIN_ELEMENTS = {k: 0 for k in rule}
    won_sizes = {k: [] for k, _ in MODES}
    lost_sizes = {k: [] for k, _ in MODES}
    for B in (2, 1):
        for where, H, W in PLANES:
            gen = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn((B, C, H, W), device=dev, generator=gen).requires_grad_(True)
            g = torch.randn((B, C, H, W), device=dev, generator=gen)
            bn = FrozenBatchNorm2d(C).to(dev)
            with torch.no_grad():
                bn.weight.copy_(0.25 + 1.5 * torch.rand(C, device=dev, generator=gen))
                bn.bias.copy_(0.4 * torch.randn(C, device=dev, generator=gen))
                bn.running_mean.copy_(0.5 * torch.randn(C, device=dev, generator=gen))
                bn.running_var.copy_(0.3 + 1.5 * torch.rand(C, device=dev, generator=gen))
            drop = nn.Dropout2d(0.1).train()
            assert norm.fallback_reason(x, bn) is None and norm.dropout_fallback_reason(x, bn, drop) is None
            ops = {"fused": (lambda: norm.norm_relu(x, bn), lambda: norm.norm_relu_dropout2d(x, bn, drop)),
                   "stock": (lambda: F.relu(bn(x), inplace=True), lambda: drop(F.relu(bn(x), inplace=True)))}
            sides = {}
            for tag, (tail, tail_drop) in ops.items():
                def fwd(op=tail):
                    with torch.no_grad():
                        op()

                def both(op=tail):
                    torch.autograd.grad(op(), x, g)

                def with_drop(op=tail_drop):
                    torch.autograd.grad(op(), x, g)
                sides[tag] = dict(fwd=fwd, both=both, drop=with_drop)
            order = [(t, k) for k, _ in MODES for t in ("fused", "stock")]
            times = dict(zip(order, windows([sides[t][k] for t, k in order], args.n, args.repeats)))
            say("%-15s x %dx%dx%dx%d  (%d elements)" % (where, B, C, H, W, x.numel()))
            for k, label in MODES:
                f, s = times[("fused", k)], times[("stock", k)]
                won = med(s) - med(f) > s[-1] - s[0]
                (won_sizes if won else lost_sizes)[k].append(x.numel())
                say("    %-24s fused %s   stock %s   stock/fused (medians) x%.3f   stock spread %.4f   %s"
                    % (label, fmt(f), fmt(s), med(s) / med(f), s[-1] - s[0], "fused wins" if won else "NO WIN"))
            # the same bits, checked where they are timed (one seed for both sides of the dropout)
            with torch.no_grad():
                assert torch.equal(ops["fused"][0](), ops["stock"][0]())
                torch.manual_seed(1)
                a = ops["fused"][1]()
                torch.manual_seed(1)
                assert torch.equal(a, ops["stock"][1]())
                del a
            del sides, times, ops, x, g, bn
            torch.cuda.empty_cache()
    norm.AUTOGRAD_MIN_ELEMENTS = rule
    for k, label in MODES:
        lost = max(lost_sizes[k]) if lost_sizes[k] else 0
        above = sorted(n for n in won_sizes[k] if n > lost)
        say("%-24s smallest size from which every timed size wins: %s   (sizes lost: %s)"
            % (label, above[0] if above else "none", sorted(set(lost_sizes[k])) or "none"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
