#!/usr/bin/env python3
"""Generate tests/golden/eval.npz by RUNNING the reference's own validation code.

Run where the reference's tree exists (it never travels to the GPU box):

    python tests/golden/make_eval_fixtures.py         # writes tests/golden/eval.npz

What runs is the reference's code:
  core/utils/misc.py          intersectionAndUnionGPU (imported through tests/golden/_shims for yacs)
  core/train_learners.py      BaseLearner.inference and BaseLearner.intersectionAndUnionGPU: the module imports
                              pytorch_lightning, geoopt's optimiser and the dataset stack, none of which exists here, so the two
                              methods are compiled out of the file with `ast` at generation time and bound to a stand-in
                              learner whose head returns the case's logits
with torch.Tensor.cuda neutralised (no GPU here).  Only DATA is written: inputs, the arg-max maps and the reference's arrays.

Cases (small: H x W = 64 x 128, a multiple of 16 pixels, so ATen's softmax has no scalar tail; B = 3 images each):
  K = 19 / 16 (templated kernels) and 7 (the generic one), flip on and off, int64 / int32 / uint8 labels holding 255, values
  in K..254 and (signed labels) -1; one pixel with all classes tied in both views (pred 0), two identical class planes that
  dominate (the lower index wins), a NaN logit (its pixels are NaN after the softmax: pred 0).
Full size (tests/eval_inputs.FULLSIZE): only the seed, the reference's counts and a sha256 of its arg-max map.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("HALO_FIXTURE_OUT", HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import eval_inputs as ei  # noqa: E402
from make_fixtures import REF  # noqa: E402  (the reference's tree: $HALO_REFERENCE)

H, W, B = 64, 128, 3
CASES = [  # name, K, flip, label dtype, low-res (h, w)
    ("k19_flip_i64", 19, True, np.int64, (16, 32)),
    ("k19_noflip_i32", 19, False, np.int32, (13, 27)),
    ("k19_flip_u8", 19, True, np.uint8, (11, 20)),
    ("k16_flip_i32", 16, True, np.int32, (16, 32)),
    ("k16_noflip_u8", 16, False, np.uint8, (9, 17)),
    ("k7_flip_i64", 7, True, np.int64, (16, 32)),
    ("k7_noflip_i32", 7, False, np.int32, (12, 25)),
]


def reference():
    sys.path.insert(0, os.path.join(HERE, "_shims"))
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self
    import core.utils.misc as misc
    tree = ast.parse(open(os.path.join(REF, "core", "train_learners.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BaseLearner")
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("inference", "intersectionAndUnionGPU")]
    ns = {"torch": torch, "F": F, "os": os, "np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "train_learners.py", "exec"), ns)
    return misc, ns["inference"], ns["intersectionAndUnionGPU"]


class StandIn(object):
    """A learner whose head returns the logits it was given (inference runs it on cat([x, flip(x)]))."""

    def __init__(self, logits):
        self.feature_extractor = lambda image: image
        self.classifier = lambda feat: (logits, None)


def make_case(K, flip, dtype, hl, wl, seed):
    rng = np.random.default_rng(seed)
    views = 2 if flip else 1
    lg = rng.standard_normal((B * views, K, hl, wl), dtype=np.float32) * np.float32(2.5)
    lg[views * 0:views * 0 + views, :, 0, 0] = np.float32(0.75)            # image 0: all classes tied at the top-left corner...
    if flip:
        lg[1, :, 0, wl - 2:] = np.float32(-1.25)                           # ...in both views (view 1 is read mirrored)
    if K > 5:
        same = lg[views:2 * views, 3] + np.float32(6.0)                    # image 1: classes 3 and 5 identical and dominant
        lg[views:2 * views, 3] = same
        lg[views:2 * views, 5] = same
    lg[2 * views, 1, hl // 2, wl // 2] = np.float32("nan")                  # image 2: one NaN logit
    lg[2 * views, :, 1, :] *= np.float32(40.0)                              # image 2: a saturated row (the general softmax)
    signed = dtype != np.uint8
    label = rng.integers(0, K, (B, H, W)).astype(np.int64)
    r = rng.random((B, H, W))
    label[r < 0.10] = 255
    label[(r >= 0.10) & (r < 0.14)] = rng.integers(K, 255, int(((r >= 0.10) & (r < 0.14)).sum()))
    if signed:
        label[(r >= 0.14) & (r < 0.17)] = -1
    return lg, label.astype(dtype)


def run_reference(misc, inference, iou_method, lg, label, K, flip):
    views = 2 if flip else 1
    preds, arrays = [], []
    for i in range(label.shape[0]):
        y = torch.from_numpy(label[i:i + 1].copy())
        me = StandIn(torch.from_numpy(lg[views * i: views * i + views].copy()))
        x = torch.zeros((1, 3, 4, 4))
        pred = inference(me, x, y, flip=flip)                    # validation_step (train_learners.py:108-112)
        output = pred.max(1)[1]
        preds.append(output[0].numpy().copy())
        a = misc.intersectionAndUnionGPU(output.clone(), y.clone(), K, 255)
        b = iou_method(me, output.clone(), y.clone(), K, 255)
        for u, v in zip(a, b):
            assert np.array_equal(np.asarray(u), np.asarray(v)), "misc / learner intersectionAndUnionGPU disagree"
        arrays.append(np.stack([np.asarray(t, dtype=np.float32) for t in a]))
    return np.stack(preds).astype(np.int64), np.stack(arrays)


def main():
    misc, inference, iou_method = reference()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    for n, (name, K, flip, dtype, (hl, wl)) in enumerate(CASES):
        lg, label = make_case(K, flip, dtype, hl, wl, 100 + n)
        pred, arrays = run_reference(misc, inference, iou_method, lg, label, K, flip)
        out[name + "/logits"] = lg
        out[name + "/label"] = label
        out[name + "/pred"] = pred
        out[name + "/ref"] = arrays                                  # (B, 3, K) float32: intersection, union, target
        out[name + "/meta"] = np.array([K, 1 if flip else 0], np.int64)
        print(name, "pred classes", np.bincount(pred.reshape(-1), minlength=K)[:K].tolist())
    for name, (seed, K, hl, wl, Hf, Wf) in ei.FULLSIZE.items():
        lg, label = ei.fullsize(name)
        pred, arrays = run_reference(misc, inference, iou_method, lg, label[None], K, True)
        out["full_" + name + "/ref"] = arrays[0]
        out["full_" + name + "/pred_sha256"] = np.array(ei.digest(pred[0]))
        print(name, "mIoU-ish", float((arrays[0, 0] / (arrays[0, 1] + 1e-10)).mean()))
    np.savez_compressed(os.path.join(OUT, "eval.npz"), **out)
    print("wrote", os.path.join(OUT, "eval.npz"))


if __name__ == "__main__":
    main()
