"""Timing aid: halo_amd.norm.norm_relu_maxpool (halo_maxpool.hip) against the two chains it replaces behind the stem's convolution,
in the same process on the same data, float32:

  stock    FrozenBatchNorm2d (x * scale + bias as torch statements, scale and bias recomputed per call), ReLU(inplace=True),
           nn.MaxPool2d(3, 2, 1);
  pair     halo_amd.norm.norm_relu (halo_norm.hip, what fuse_norm_relu_pairs runs) followed by nn.MaxPool2d(3, 2, 1): the best chain
           without the fused pool;
  fused    halo_amd.norm.norm_relu_maxpool.

Shapes: conv1's output at the 640 x 1280 training crop and at 720 x 1280 (batch 2), at the 1024 x 2048 validation and acquisition
geometry (batch 2: a flip pair; batch 1), and two smaller ones for the speed rule under autograd (there norm_relu's own rule
hands the pair's norm to the stock statements, so "pair" is what a model under fuse_norm_relu_pairs runs).  Per shape: forward alone under
no_grad, forward + backward (gradient for x), and torch.cuda.max_memory_allocated over one forward + backward above what is held
before it.  HIP events around n calls after warm-up calls of every timed closure; `repeats` windows per figure, printed as best /
median / worst; the three sides alternate window by window.  Also reported: the fused passes' achieved bytes/s against their
algorithmic traffic.  The whole list runs `--runs` times in one process (the speed rule asks for two separate runs).  Every shape
runs under its own alarm, whose expiry ends the process, and the first failure ends the run; the lines so far are in --out.

    python tools/time_stem_pool.py [--out profiles/r17_time_stem_pool.txt] [--n 10] [--repeats 7] [--runs 2]
"""
import argparse
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd import norm  # noqa: E402
from halo_amd.norm import norm_relu, norm_relu_maxpool, pool_fallback_reason  # noqa: E402
from tools.time_norm_relu import FrozenBatchNorm2d, fmt, med, peak_mb, randomize, windows  # noqa: E402

SHAPES = [("train 640x1280 B=2", (2, 64, 320, 640)), ("train 720x1280 B=2", (2, 64, 360, 640)), ("validate flip pair", (2, 64, 512, 1024)),
          ("acquire B=1", (1, 64, 512, 1024)), ("small 1", (2, 64, 80, 160)), ("small 2", (2, 64, 160, 320))]


def time_shape(say, dev, args, label, shape):
    gen = torch.Generator(device=dev).manual_seed(0)
    B, C, H, W = shape
    x = torch.randn(shape, device=dev, generator=gen).requires_grad_(True)
    bn, pool = FrozenBatchNorm2d(C).to(dev), nn.MaxPool2d(3, 2, 1)
    randomize(bn, gen, dev)
    assert pool_fallback_reason(x, bn, pool) is None, pool_fallback_reason(x, bn, pool)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.randn((B, C, OH, OW), device=dev, generator=gen)
    act = nn.ReLU(inplace=True)
    ops = (("fused", lambda: norm_relu_maxpool(x, bn, pool)), ("pair", lambda: pool(norm_relu(x, bn))), ("stock", lambda: pool(act(bn(x)))))
    sides = {}
    for tag, op in ops:
        def fwd(op=op):
            with torch.no_grad():
                op()

        def both(op=op):
            torch.autograd.grad(op(), [x], g)
        sides[tag] = dict(fwd=fwd, both=both)
    order = [(t, k) for k in ("fwd", "both") for t, _ in ops]
    times = dict(zip(order, windows([sides[t][k] for t, k in order], args.n, args.repeats)))
    nx, no = x.numel() * 4, g.numel() * 4
    say("%-20s %s  (x: %.1f MB, out: %.1f MB)" % (label, "x".join(map(str, shape)), nx / 1e6, no / 1e6))
    wins = True
    for kind, name in (("fwd", "forward"), ("both", "fwd+bwd")):
        f, p, s = (times[(t, kind)] for t in ("fused", "pair", "stock"))
        lost = med(f) > min(med(p), med(s))
        wins = wins and not lost
        say("    %-8s fused %s   pair %s   stock %s   pair/fused x%.2f  stock/fused x%.2f (medians)%s"
            % (name, fmt(f), fmt(p), fmt(s), med(p) / med(f), med(s) / med(f), "   FUSED LOSES" if lost else ""))
    fwd_bytes, bwd_bytes = nx + no, no + no // 4 + nx        # x -> out (no codes under no_grad); g + codes -> g_x
    say("    fused forward (no_grad): %.2f TB/s of its algorithmic traffic (%.1f MB); fused fwd+bwd: %.2f TB/s of %.1f MB"
        % (fwd_bytes / (med(times[("fused", "fwd")]) * 1e-3) / 1e12, fwd_bytes / 1e6,
           (fwd_bytes + no // 4 + bwd_bytes) / (med(times[("fused", "both")]) * 1e-3) / 1e12, (fwd_bytes + no // 4 + bwd_bytes) / 1e6))
    with torch.no_grad():
        y_f, y_s = norm_relu_maxpool(x, bn, pool), pool(act(bn(x)))
    gx_f, = torch.autograd.grad(norm_relu_maxpool(x, bn, pool), [x], g)
    gx_s, = torch.autograd.grad(pool(act(bn(x))), [x], g)
    same = torch.equal(y_f, y_s), torch.equal(gx_f, gx_s)
    del y_f, y_s, gx_f, gx_s
    say("    torch.equal to the stock chain: out %s, g_x %s; peak memory above the operands over one fwd+bwd: fused %.1f MiB, pair %.1f MiB, "
        "stock %.1f MiB" % (same + tuple(peak_mb(sides[t]["both"]) for t in ("fused", "pair", "stock"))))
    if not all(same):
        raise SystemExit("the fused operator differs from the stock chain")
    return wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file, line by line")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2, help="how often the whole list of shapes is timed")
    ap.add_argument("--step-seconds", type=int, default=60, help="alarm per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_stem_pool.py needs a ROCm device")
    dev = torch.device("cuda:0")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")

    def say(s):
        print(s, flush=True)
        if out is not None:
            out.write(s + "\n")
            out.flush()

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    rule, norm.POOL_AUTOGRAD_MIN_ELEMENTS = norm.POOL_AUTOGRAD_MIN_ELEMENTS, 0           # time the kernels at every size
    say("halo_amd.norm.POOL_AUTOGRAD_MIN_ELEMENTS as shipped: %d (0 while timing)" % rule)
    for run in range(args.runs):
        say("run %d" % (run + 1))
        losers = []
        for label, shape in SHAPES:
            signal.alarm(args.step_seconds)                     # no handler: an overrun ends the process
            if not time_shape(say, dev, args, label, shape):
                losers.append(shape)
            signal.alarm(0)
            torch.cuda.empty_cache()
        say("run %d: shapes at which a fused median is above the pair's or the stock chain's: %s" % (run + 1, losers or "none"))
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
