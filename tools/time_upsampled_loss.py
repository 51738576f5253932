"""Timing aid: the training criterion, fused (halo_amd.training.upsampled_losses: one forward and one backward launch from the
low-resolution logits) against the stock chain every learner step runs (F.interpolate(align_corners=True) -> torch.softmax ->
CrossEntropyLoss(ignore_index=255) + NegativeLearningLoss -> backward to the low-resolution logits), at the training shapes:

    target  2 x 19 x 160 x 320 -> 640 x 1280, labels about 95 % 255 (an active mask)
    source  2 x 19 x 180 x 320 -> 720 x 1280, dense labels
    k16     2 x 16 x 160 x 320 -> 640 x 1280, dense labels

HIP events around n calls after warm-up (as tools/time_training_ops.py); best of five.  Also the forward alone, the backward
alone (the recomputed halo's cost shows as backward / forward) and torch.cuda.max_memory_allocated over one forward + backward
above what the inputs hold.

    python tools/time_upsampled_loss.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from halo_amd.training import upsampled_losses  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = [("target", 2, 19, (160, 320), (640, 1280), 0.05), ("source", 2, 19, (180, 320), (720, 1280), 1.0),
          ("k16", 2, 16, (160, 320), (640, 1280), 0.9)]


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


def stock(x, y):
    up = F.interpolate(x, size=y.shape[-2:], mode="bilinear", align_corners=True)
    ce = nn.CrossEntropyLoss(ignore_index=255)(up, y)
    p = torch.softmax(up, dim=1)
    mask = (p < 0.05).detach()
    nl = torch.sum(-1 * mask * torch.log(1 - p + 1e-6)) / torch.sum(mask)       # NegativeLearningLoss()(p)
    return ce, nl


def main():
    print("device:", torch.cuda.get_device_name(0))
    for name, B, K, (h, w), (H, W), frac in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = (torch.randn((B, K, h, w), device=dev, generator=g) * 2.5).requires_grad_(True)
        y = torch.randint(0, K, (B, H, W), device=dev, generator=g)
        y[torch.rand((B, H, W), device=dev, generator=g) >= frac] = 255

        def fused_fb():
            r = upsampled_losses(x, y, check_labels=False)
            (r.ce + r.nl).backward()

        def fused_f():
            with torch.no_grad():
                upsampled_losses(x, y, check_labels=False)

        def stock_fb():
            ce, nl = stock(x, y)
            (ce + nl).backward()

        r = upsampled_losses(x, y, check_labels=False)
        loss = r.ce + r.nl

        def fused_b():
            torch.autograd.grad(loss, x, retain_graph=True)

        t_fused, t_stock = timeit(fused_fb), timeit(stock_fb)
        t_f, t_b = timeit(fused_f), timeit(fused_b)
        m_fused, m_stock = peak_mb(fused_fb), peak_mb(stock_fb)
        print(f"{name:6s} {B}x{K}x{h}x{w} -> {H}x{W}: fused fwd+bwd {t_fused:.3f} ms (fwd {t_f:.3f}, bwd {t_b:.3f}), "
              f"stock fwd+bwd {t_stock:.3f} ms, x{t_stock / t_fused:.1f}; peak memory fused {m_fused:.1f} MiB, stock {m_stock:.1f} MiB")


if __name__ == "__main__":
    main()
