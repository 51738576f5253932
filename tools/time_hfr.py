"""Timing aid: the v3+ head's HFR weighted normalisation, fused (halo_amd.hfr.weighted_normalize, halo_hfr.hip) against the
stock torch statement (halo_amd.hfr.torch_statement: permute copy, Linear, BatchNorm1d, ReLU, Linear, mean, clamp,
F.normalize, multiply, and autograd's backward of all of it) on the device, at

    target  2 x 64 x 160 x 320, training (the target crop)
    source  2 x 64 x 180 x 320, training (the source crop)
    eval    2 x 64 x 160 x 320, evaluation, forward only (the flip-TTA batch)

HIP events around n calls after warm-up (as tools/time_upsampled_loss.py); best of five.  The forward alone, forward plus
backward (to x and the six parameters), and torch.cuda.max_memory_allocated over one call above what the inputs hold.

    python tools/time_hfr.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd.hfr import torch_statement, weighted_normalize  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = [("target", 2, 64, (160, 320), True), ("source", 2, 64, (180, 320), True), ("eval", 2, 64, (160, 320), False)]


def timeit(fn, n=20, repeats=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / n)
    return best


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    print("device:", torch.cuda.get_device_name(0))
    for name, B, C, (h, w), training in SHAPES:
        torch.manual_seed(0)
        x = (torch.randn((B, C, h, w), device=dev) * 0.7).requires_grad_(training)
        g = torch.randn((B, C, h, w), device=dev)
        mlp = nn.Sequential(nn.Linear(C, C), nn.BatchNorm1d(C), nn.ReLU(), nn.Linear(C, C)).to(dev).train(training)
        params = [x] + list(mlp.parameters())

        def run(fn, backward):
            if backward:
                y = fn(x, mlp)
                torch.autograd.grad(y, params, g)
            else:
                with torch.no_grad():
                    fn(x, mlp)

        row = []
        for tag, fn in (("fused", weighted_normalize), ("stock", torch_statement)):
            t_f = timeit(lambda: run(fn, False))
            t_fb = timeit(lambda: run(fn, True)) if training else None
            mem = peak_mb(lambda: run(fn, training))
            row.append((tag, t_f, t_fb, mem))
        (_, ff, ffb, fm), (_, sf, sfb, sm) = row
        line = f"{name:6s} {B}x{C}x{h}x{w} {'train' if training else 'eval '}: fused fwd {ff:.3f} ms"
        if training:
            line += f", fwd+bwd {ffb:.3f} ms; stock fwd {sf:.3f} ms, fwd+bwd {sfb:.3f} ms, x{sfb / ffb:.1f}"
        else:
            line += f"; stock fwd {sf:.3f} ms, x{sf / ff:.1f}"
        line += f"; peak memory fused {fm:.1f} MiB, stock {sm:.1f} MiB"
        print(line, flush=True)


if __name__ == "__main__":
    main()
