"""Inputs and a torch-CPU statement of the validation metric's chain (halo_amd.metrics, halo_eval.hip).

The chain is BaseLearner.inference + validation_step + intersectionAndUnionGPU (core/train_learners.py:57-128) written
out in plain torch on the CPU: upsample (align_corners=True), softmax over the classes, (view 0 + flipped view 1) / 2, the
first maximal class, then the reference's integer counts.  tests/golden/make_eval_fixtures.py pins it against the reference's
own code; the tests hold the HIP path to it.  The full-size inputs are rebuilt from a seed with numpy's PCG64 stream, so the
generator and the GPU box see the same arrays (`digest` says so).

`contract_pred` is the same chain stated with the CPU oracle (oracle/): torch's CPU softmax ends each thread's chunk with a scalar
exp tail off multiples of 16 pixels, so the RAGGED cases (sizes off the kernels' 1024 pixels per block, degenerate geometry, the
generic kernel's class counts) are held to it.  tests/test_eval_metrics.py ties it to the reference's fixture.
"""
import functools
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


def contract_pred(logits, size, flip=True):
    """The chain as the numeric contract states it, arg-max map (B, H, W) int64: per image and view the CPU
    oracle's float32 resize and its softmax (ATen's vector statement at every pixel, so no scalar tails at ragged sizes),
    (p0 + mirrored p1) / float32(2), then torch.max(dim)'s CPU rule from class 0 on: `if (!(v <= best)) { take; if NaN stop }`.
    logits: (B*views, K, h, w) float32 numpy array."""
    from oracle import halo_oracle as ho
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    views = 2 if flip else 1
    preds = []
    for i in range(lg.shape[0] // views):
        p = [ho.softmax(ho.bilinear(lg[views * i + v], size)) for v in range(views)]
        a = (p[0] + p[1][:, :, ::-1]) / np.float32(2) if flip else p[0]
        del p
        best = a[0].copy()
        am = np.zeros(best.shape, np.int64)
        stop = np.isnan(best)
        for c in range(1, a.shape[0]):
            take = ~stop & ~(a[c] <= best)
            am[take] = c
            best[take] = a[c][take]
            stop |= take & np.isnan(a[c])
        preds.append(am)
    return np.stack(preds)


# Sizes off the kernels' 1024 pixels per block, degenerate geometry and the generic kernel's class counts.
# name -> (seed, K, (h, w), (H, W), views, B, label dtype); rebuilt from the seed like FULLSIZE, nothing stored.
RAGGED = {
    "k19_identity_5x7": (201, 19, (5, 7), (5, 7), 2, 2, np.int64),         # 35 px: one partial wave, iterations 1-3 empty
    "k19_37x53": (202, 19, (13, 27), (37, 53), 2, 3, np.int32),            # 1961 px: block 1 ends mid-wave, one wave wholly empty; odd W
    "k16_33x31_noflip": (203, 16, (9, 17), (33, 31), 1, 2, np.uint8),      # 1023 px: one short of a block
    "k16_25x41": (204, 16, (9, 17), (25, 41), 2, 2, np.int64),             # 1025 px: a block holding one pixel
    "k16_33x31": (216, 16, (9, 17), (33, 31), 2, 2, np.int32),             # so that K = 16 meets all three label dtypes
    "k19_1x70": (205, 19, (3, 4), (1, 70), 2, 1, np.int32),                # H = 1: zero scale along y
    "k19_63x1": (206, 19, (3, 4), (63, 1), 2, 1, np.uint8),                # W = 1: zero scale along x, mirrors onto itself
    "k19_one_cell": (207, 19, (1, 1), (9, 13), 2, 1, np.int64),            # a single source cell
    "k19_down_5x7": (208, 19, (9, 11), (5, 7), 2, 1, np.int32),            # downsampling
    "k7_37x53": (209, 7, (12, 25), (37, 53), 2, 3, np.uint8),              # the generic kernel, ragged
    "k1_21x50": (210, 1, (4, 6), (21, 50), 2, 2, np.int64),                # generic kernel, 1050 px, from here on
    "k2_21x50_noflip": (211, 2, (4, 6), (21, 50), 1, 2, np.int32),
    "k20_21x50": (212, 20, (4, 6), (21, 50), 2, 2, np.uint8),              # the first class count past a templated kernel
    "k86_21x50": (213, 86, (4, 6), (21, 50), 2, 2, np.uint8),              # 3 K = 258 words: the histogram loops' second trip
    "k1024_21x50_noflip": (214, 1024, (4, 6), (21, 50), 1, 2, np.int32),   # the limit: 16-bit key halves, 12 KB of LDS
    "k1024_21x50": (215, 1024, (4, 6), (21, 50), 2, 2, np.int64),
}
# where ragged() puts make_eval_fixtures.make_case's plants, image indices modulo B
RAGGED_TIE_IMAGE, RAGGED_PLANES_IMAGE, RAGGED_NAN_IMAGE = 0, 1, 2


def ragged(name):
    """(logits (B*views, K, h, w) float32, label (B, H, W) of the case's dtype) with make_eval_fixtures.make_case's plants: all
    classes tied at image 0's top-left pixel in both views (pred 0), classes 3 and 5 identical and dominant in image 1 % B where
    K > 5 (the lower wins), one NaN logit at the centre of image 2 % B's view 0 (pred 0 wherever it is a tap) and that view's
    row 1 scaled by 40 (the general softmax).  A single source cell is the whole image, so it carries only the identical
    planes: the tie and the NaN would each decide every pixel.  Where K > 19 each source cell also favours one class and half
    of the labels follow it, so the intersection row is populated at the high classes.  Labels hold 255, values outside
    [0, K) and, for signed dtypes, -1; each image's last pixel, which the kernels' tail lanes recompute, has a label that
    counts."""
    seed, K, (h, w), (H, W), views, B, dtype = RAGGED[name]
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((B * views, K, h, w), dtype=np.float32) * np.float32(2.5)
    fav = rng.integers(0, K, (B, h, w))
    if K > 19:
        for b in range(B):
            for v in range(views):
                cells = fav[b] if v == 0 else fav[b][:, ::-1]                # view 1 is the flipped image
                np.put_along_axis(lg[views * b + v], cells[None], np.float32(9.0), axis=0)
    one_cell = h * w == 1
    if K > 5:
        i = views * (RAGGED_PLANES_IMAGE % B)
        same = lg[i:i + views, 3] + np.float32(6.0 if K <= 19 else 16.0)   # above the favoured classes too
        lg[i:i + views, 3] = same
        lg[i:i + views, 5] = same
    if not one_cell:
        i = views * (RAGGED_NAN_IMAGE % B)
        lg[i, :, min(1, h - 1), :] *= np.float32(40.0)
        i = views * (RAGGED_TIE_IMAGE % B)
        lg[i:i + views, :, 0, 0] = np.float32(0.75)
        if views == 2:                                                       # view 1 is read mirrored: column W-1-0
            lg[i + 1, :, 0, (slice(0, 1) if W == 1 else slice(max(w - 2, 0), w))] = np.float32(-1.25)
        ny, nx = (h // 2, w // 2) if W > 1 else (h - 1, 0)                   # W = 1 reads column 0 alone; clear of the tied pixel
        lg[views * (RAGGED_NAN_IMAGE % B), min(1, K - 1), ny, nx] = np.float32("nan")
    label = rng.integers(0, K, (B, H, W)).astype(np.int64)
    if K > 19:                                                               # nearest source cell's favoured class
        ys = np.rint(np.arange(H) * ((h - 1) / max(H - 1, 1))).astype(np.int64)
        xs = np.rint(np.arange(W) * ((w - 1) / max(W - 1, 1))).astype(np.int64)
        follow = rng.random((B, H, W)) < 0.5
        label[follow] = fav[:, ys][:, :, xs][follow]
    r = rng.random((B, H, W))
    label[r < 0.10] = 255
    outside = (r >= 0.10) & (r < 0.14)
    if K < 254:
        label[outside] = rng.integers(K, 255, int(outside.sum()))
    elif dtype != np.uint8:
        label[outside] = rng.integers(K, K + 1000, int(outside.sum()))
    if dtype != np.uint8:
        label[(r >= 0.14) & (r < 0.17)] = -1
    flat = label.reshape(B, H * W)                                           # the smallest images get one of each as well
    flat[:, -1] = min(K - 1, 200)              # the pixel that tail lanes recompute is one that counts: a mask lost there shows
    flat[:, 1] = 255
    if K < 254 or dtype != np.uint8:
        flat[:, H * W // 2] = K + 5
    if dtype != np.uint8:
        flat[:, H * W // 3] = -1
    return lg, label.astype(dtype)


@functools.lru_cache(maxsize=None)
def ragged_case(name):
    """(K, views, logits, label, contract_pred's map) of a RAGGED case, computed once and read-only"""
    _, K, _, size, views, _, _ = RAGGED[name]
    lg, label = ragged(name)
    pred = contract_pred(lg, size, views == 2)
    for a in (lg, label, pred):
        a.setflags(write=False)
    return K, views, lg, label, pred


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
