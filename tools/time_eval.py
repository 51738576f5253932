"""Timing aid: the validation metric, fused (halo_amd.metrics.flip_tta_confusion) against the reference's chain on the device
(BaseLearner.inference + validation_step + intersectionAndUnionGPU: upsample both views to label size, softmax, flip-average,
arg-max, ignore write, three float32 copies to the host and torch.histc there).  HIP events around each timed window; every
window ends in a device synchronise (the reference's chain synchronises by itself, per image).

    python tools/time_eval.py [--out profiles/r07_time_eval.txt]

Sizes: the v3+ head's 160 x 320 and the v2 head's 80 x 160 logits, K = 19, upsampled to 1024 x 2048; one image pair per call
and 16 pairs per call (one launch for the fused path, 16 images one after another for the chain, as the reference runs them).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from halo_amd.metrics import flip_tta_confusion  # noqa: E402

K, H, W = 19, 1024, 2048


def reference_chain(lg, label):
    """the reference's chain for B images, one after another (its loader batch is 1); returns the summed float32 arrays"""
    acc = torch.zeros((3, K))
    for i in range(label.shape[0]):
        out = F.interpolate(lg[2 * i: 2 * i + 2], size=(H, W), mode="bilinear", align_corners=True)
        out = F.softmax(out, dim=1)
        out = ((out[0] + out[1].flip(2)) / 2).unsqueeze(0)
        output = out.max(1)[1].view(-1)
        target = label[i].view(-1)
        output[target == 255] = 255
        inter = output[output == target]
        a_i = torch.histc(inter.float().cpu(), bins=K, min=0, max=K - 1)
        a_o = torch.histc(output.float().cpu(), bins=K, min=0, max=K - 1)
        a_t = torch.histc(target.float().cpu(), bins=K, min=0, max=K - 1)
        acc += torch.stack([a_i, a_o + a_t - a_i, a_t])
    return acc


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["device: %s" % torch.cuda.get_device_name(dev), "K = %d, label %d x %d, int64 labels with 10 %% ignored" % (K, H, W)]
    for h, w, head in ((160, 320, "v3+"), (80, 160, "v2")):
        for B in (1, 16):
            g = torch.Generator(device=dev).manual_seed(h + B)
            lg = torch.randn((2 * B, K, h, w), generator=g, device=dev) * 3
            label = torch.randint(0, K, (B, H, W), generator=g, device=dev)
            label[torch.rand((B, H, W), generator=g, device=dev) < 0.1] = 255
            fused_counts = flip_tta_confusion(lg, label, K).sum(0).cpu()
            chain_counts = reference_chain(lg, label)
            same = torch.equal(fused_counts.float(), chain_counts)
            out = torch.zeros((B, 3, K), dtype=torch.int64, device=dev)
            t_fused = timed(lambda: flip_tta_confusion(lg, label, K, out=out), args.reps)
            t_chain = timed(lambda: reference_chain(lg, label), max(2, args.reps // 4))
            lines.append("%s head %dx%d, %2d image pair(s): fused %.3f ms (%.3f ms/pair), reference chain %.2f ms (%.2f ms/pair), "
                         "%.0fx; counts equal: %s" % (head, h, w, B, t_fused, t_fused / B, t_chain, t_chain / B, t_chain / t_fused, same))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
