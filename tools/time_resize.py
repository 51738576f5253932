"""Timing aid: halo_amd.resize.bilinear_resize (halo_bilinear_upsample forward, the gather adjoint of halo_resize.hip backward)
against stock F.interpolate(mode='bilinear', align_corners=True) under autograd, in the same process on the same device, float32
and float64, at the training paths' resizes:

    body    2 x 256 x  40 x  80 -> 160 x  320    the v3+ head's bottleneck output -> low-level feature size
    target  2 x  19 x 160 x 320 -> 640 x 1280    target logits
    source  2 x  19 x 180 x 320 -> 720 x 1280    source logits / LocalConsistentLoss input
    embed   2 x  64 x  80 x 160 -> 640 x 1280    the v2 head's embedding (float64 in the model)

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst so that the spread is on the page next to every difference.  The two sides alternate window by window.
Also: whether two stock backward calls on the same operands are bit-equal (and the two device ones), and
torch.cuda.max_memory_allocated over one forward + backward above what the operands hold.

    python tools/time_resize.py [--out profiles/r07_time_resize.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from halo_amd.resize import bilinear_resize  # noqa: E402

SHAPES = [("body", (2, 256, 40, 80), (160, 320)), ("target", (2, 19, 160, 320), (640, 1280)),
          ("source", (2, 19, 180, 320), (720, 1280)), ("embed", (2, 64, 80, 160), (640, 1280))]


def windows(fns, n=20, repeats=7):
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


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def stock_resize(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_resize.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over 7 windows of 20 calls: best / median / worst")
    for dtype in (torch.float32, torch.float64):
        for name, shape, size in SHAPES:
            gen = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn(shape, device=dev, dtype=dtype, generator=gen).requires_grad_(True)
            g = torch.randn(shape[:2] + size, device=dev, dtype=dtype, generator=gen)
            sides = {}
            for tag, op in (("device", bilinear_resize), ("stock", stock_resize)):
                y = op(x, size)

                def fwd(op=op):
                    with torch.no_grad():
                        op(x, size)

                def bwd(y=y):
                    torch.autograd.grad(y, x, g, retain_graph=True)

                def both(op=op):
                    torch.autograd.grad(op(x, size), x, g)

                (a,), (b,) = torch.autograd.grad(y, x, g, retain_graph=True), torch.autograd.grad(y, x, g, retain_graph=True)
                sides[tag] = dict(fwd=fwd, bwd=bwd, both=both, grad=a, equal=bool(torch.equal(a, b)))
            order = [(t, k) for k in ("fwd", "bwd", "both") for t in ("device", "stock")]
            times = dict(zip(order, windows([sides[t][k] for t, k in order])))
            gd, gs = sides["device"]["grad"].double(), sides["stock"]["grad"].double()
            say("%-6s %s %s -> %s" % (name, str(dtype).replace("torch.", ""), "x".join(map(str, shape)), "x".join(map(str, size))))
            for k, label in (("fwd", "forward"), ("bwd", "backward"), ("both", "fwd+bwd")):
                d, s = times[("device", k)], times[("stock", k)]
                say("    %-8s device %s   stock %s   stock/device (medians) x%.2f" % (label, fmt(d), fmt(s), s[len(s) // 2] / d[len(d) // 2]))
            say("    two backward calls bit-equal: device %s, stock %s; max |device - stock| = %.3g of max |stock| = %.3g"
                % (sides["device"]["equal"], sides["stock"]["equal"], float((gd - gs).abs().max()), float(gs.abs().max())))
            say("    peak memory above the operands over one fwd+bwd: device %.1f MiB, stock %.1f MiB"
                % (peak_mb(sides["device"]["both"]), peak_mb(sides["stock"]["both"])))
            del sides, times, x, g
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
