"""Inputs and a torch-CPU statement of the validation metric's chain (halo_amd.metrics, halo_eval.hip).

The chain is BaseLearner.inference + validation_step + intersectionAndUnionGPU (core/train_learners.py:57-128) written
out in plain torch on the CPU: upsample (align_corners=True), softmax over the classes, (view 0 + flipped view 1) / 2, the
first maximal class, then the reference's integer counts.  tests/golden/make_eval_fixtures.py pins it against the reference's
own code; the tests hold the HIP path to it.  The full-size inputs are rebuilt from a seed with numpy's PCG64 stream, so the
generator and the GPU box see the same arrays (`digest` says so).
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

FULLSIZE = {   # name -> (seed, K, h, w, H, W): the v3+ head (stride 6.4) and the v2 head (stride 12.8) at Cityscapes' label size
    "v3p_160x320": (11, 19, 160, 320, 1024, 2048),
    "v2_80x160": (12, 19, 80, 160, 1024, 2048),
}


def fullsize(name):
    """(logits (2, K, h, w) float32: an image and its flipped copy, label (H, W) int64 with 255 and out-of-range values)."""
    seed, K, h, w, H, W = FULLSIZE[name]
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((2, K, h, w), dtype=np.float32) * np.float32(3.0))
    logits[:, 2] += np.float32(1.5)                                  # a class that wins often
    logits[1, :, :, : w // 4] *= np.float32(30.0)                     # saturated softmax in one quarter of view 1
    label = rng.integers(0, K, (H, W), dtype=np.int64)
    label[rng.random((H, W)) < 0.1] = 255
    label[: H // 16, : W // 16] = 200                                 # outside [0, K): not a target, prediction still counted
    return logits, label


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def torch_chain_pred(logits, size, flip=True):
    """arg-max map (B, H, W) int64 of the chain for B images; logits (B*views, K, h, w) float32 torch tensor on the CPU."""
    views = 2 if flip else 1
    preds = []
    for i in range(logits.shape[0] // views):
        out = F.interpolate(logits[views * i: views * i + views], size=size, mode="bilinear", align_corners=True)
        out = F.softmax(out, dim=1)
        out = (out[0] + out[1].flip(2)) / 2 if flip else out[0]
        preds.append(out.unsqueeze(0).max(1)[1])
    return torch.cat(preds, 0)


def counts_from_pred(pred, label, K, ignore_index=255):
    """(3, K) int64 [intersection, union, target] of one image with the reference's semantics: o = ignore where the label is
    ignored, histc(bins=K, min=0, max=K-1) keeps the integers 0..K-1."""
    t = np.asarray(label).astype(np.int64).reshape(-1)
    o = np.where(t == ignore_index, ignore_index, np.asarray(pred).astype(np.int64).reshape(-1))

    def hist(v):
        v = v[(v >= 0) & (v < K)]
        return np.bincount(v, minlength=K).astype(np.int64)

    inter, out, tgt = hist(o[o == t]), hist(o), hist(t)
    return np.stack([inter, out + tgt - inter, tgt])
