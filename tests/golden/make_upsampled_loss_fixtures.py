#!/usr/bin/env python3
"""Generate tests/golden/upsampled_loss.npz by RUNNING the reference's own loss modules on the CPU under autograd.

Run where the reference's tree exists (it never travels to the GPU box):

    python tests/golden/make_upsampled_loss_fixtures.py         # writes tests/golden/upsampled_loss.npz

What runs: F.interpolate(mode='bilinear', align_corners=True) as the heads call it with `size` (core/models/classifier.py),
nn.CrossEntropyLoss(ignore_index=255) as BaseLearner builds it (core/train_learners.py:45), torch.softmax and the reference's
core/loss/negative_learning_loss.py NegativeLearningLoss() with its default threshold, then torch.autograd.grad of each loss
with respect to the low-resolution logits.  Only DATA is written: inputs, the two losses, the two counts and the two
gradients (d ce / d logits and d nl / d logits, so a test can weight them).

Cases (output pixel counts are multiples of 16, where ATen's softmax has no scalar tail):
  K = 19 / 16 (templated kernels) and 7 (the generic one); int64 / int32 / uint8 labels; x4 (12 x 24 -> 48 x 96) and
  non-integer (13 x 27 -> 64 x 128) scales; an active mask (about 95 % 255) and dense labels; one image with no labelled
  pixel (ce NaN, zero gradient); and one label map holding a class in K..254, for which torch raises IndexError (only the
  inputs and that expectation are stored).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("HALO_FIXTURE_OUT", HERE)
sys.path.insert(0, HERE)
from make_fixtures import REF  # noqa: E402  (the reference's tree: $HALO_REFERENCE)

CASES = [  # name, K, label dtype, B, low-res (h, w), output (H, W), labelled fraction
    ("k19_i64_x4_active", 19, np.int64, 2, (12, 24), (48, 96), 0.05),
    ("k19_u8_frac_dense", 19, np.uint8, 1, (13, 27), (64, 128), 0.9),
    ("k16_i32_x4_dense", 16, np.int32, 2, (12, 24), (48, 96), 0.9),
    ("k16_i64_frac_active", 16, np.int64, 1, (13, 27), (64, 128), 0.05),
    ("k7_i64_x4_dense", 7, np.int64, 2, (12, 24), (48, 96), 0.9),
    ("k7_u8_frac_active", 7, np.uint8, 1, (13, 27), (64, 128), 0.05),
    ("k19_i32_unlabelled", 19, np.int32, 1, (12, 24), (48, 96), 0.0),
]
BAD_CASE = ("k7_i64_bad_label", 7, np.int64, 1, (12, 24), (48, 96), 0.9)


def reference_nl():
    sys.path.insert(0, REF)
    from core.loss.negative_learning_loss import NegativeLearningLoss
    return NegativeLearningLoss()


def make_case(K, dtype, B, hl, wl, H, W, frac, seed):
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((B, K, hl, wl), dtype=np.float32) * np.float32(2.5)
    lg[0, :, 1, :] *= np.float32(30.0)                     # a saturated row: the general softmax statement
    label = rng.integers(0, K, (B, H, W)).astype(np.int64)
    label[rng.random((B, H, W)) >= frac] = 255
    return lg, label.astype(dtype)


def run_reference(nl_module, lg, label, H, W):
    x = torch.from_numpy(lg.copy()).requires_grad_(True)
    y = torch.from_numpy(label.astype(np.int64))
    up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
    ce = nn.CrossEntropyLoss(ignore_index=255)(up, y)
    predict = torch.softmax(up, dim=1)
    nl = nl_module(predict)
    (g_ce,) = torch.autograd.grad(ce, x, retain_graph=True)
    (g_nl,) = torch.autograd.grad(nl, x)
    counts = np.array([int((y != 255).sum()), int((predict < nl_module.threshold).sum())], np.int64)
    return float(ce), float(nl), counts, g_ce.numpy(), g_nl.numpy()


def main():
    nl_module = reference_nl()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    for n, (name, K, dtype, B, (hl, wl), (H, W), frac) in enumerate(CASES):
        lg, label = make_case(K, dtype, B, hl, wl, H, W, frac, 300 + n)
        ce, nl, counts, g_ce, g_nl = run_reference(nl_module, lg, label, H, W)
        out[name + "/logits"] = lg
        out[name + "/label"] = label
        out[name + "/values"] = np.array([ce, nl], np.float64)          # float32 losses, stored exactly
        out[name + "/counts"] = counts                                  # ce_count, nl_count
        out[name + "/g_ce"] = g_ce
        out[name + "/g_nl"] = g_nl
        out[name + "/meta"] = np.array([K], np.int64)
        print(name, "ce", ce, "nl", nl, "counts", counts.tolist())
    name, K, dtype, B, (hl, wl), (H, W), frac = BAD_CASE
    lg, label = make_case(K, dtype, B, hl, wl, H, W, frac, 399)
    label.reshape(-1)[100] = K                                          # one label in K..254
    try:
        run_reference(nl_module, lg, label, H, W)
    except IndexError as exc:
        message = str(exc)
    else:
        raise AssertionError("torch accepted a label outside [0, K)")
    print(name, "torch:", message)
    out[name + "/logits"] = lg
    out[name + "/label"] = label
    out[name + "/meta"] = np.array([K], np.int64)
    out[name + "/torch_error"] = np.array(message)
    np.savez_compressed(os.path.join(OUT, "upsampled_loss.npz"), **out)
    print("wrote", os.path.join(OUT, "upsampled_loss.npz"), os.path.getsize(os.path.join(OUT, "upsampled_loss.npz")), "bytes")


if __name__ == "__main__":
    main()
