#!/usr/bin/env python3
"""Generate tests/golden/hfr.npz by RUNNING the reference's own DepthwiseSeparableASPP_Hyper (HFR on) on the CPU under autograd.

Run where the reference's tree exists (it never travels to the GPU box):

    python tests/golden/make_hfr_fixtures.py         # writes tests/golden/hfr.npz

What runs: core/models/classifier.py's DepthwiseSeparableASPP_Hyper(hfr=True), imported under its package name without
core/models/__init__.py (which needs torchvision), with the _shims of make_fixtures.py.  A forward hook on conv_reduce replaces
its output by the case's input x (a leaf tensor); a wrapper on mapper.expmap captures the weighted-normalisation output y.
torch.autograd.grad of sum(g * y) gives d x and the gradients of wn_mlp's six parameters; the BatchNorm's running statistics
after the step are recorded.  Every case runs twice: the float32 module and input, and a .double() copy of both (the
"float64 evaluation" the tests hold both the float32 reference and the device to).  Only DATA is written.

Cases: C = 64 in training (momentum=None, one all-zero channel of x, some w_b < 1e-5 so the clamp is active) and in evaluation
(running statistics, clamp active); C = 10 (training, momentum 0.1) and a small C = 256 (training), both reaching the generic arm.
W1 and W2 are multiples of 1/256 stored exactly as float16; d W1 and d W2 keep their first ROWS rows; the per-channel vectors
(bias, BatchNorm and running-statistic values and gradients) are float64, the rest float32.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("HALO_FIXTURE_OUT", HERE)
sys.path.insert(0, HERE)
from make_fixtures import REF  # noqa: E402  (the reference's tree: $HALO_REFERENCE)

CASES = [  # name, C, B, (h, w), training, momentum, zero channel, clamped channels
    ("c64_train", 64, 2, (6, 8), True, None, 5, (3, 17, 40)),
    ("c64_eval", 64, 2, (6, 8), False, 0.1, None, (2, 9)),
    ("c10_train", 10, 2, (5, 12), True, 0.1, None, (4,)),
    ("c256_train", 256, 1, (4, 4), True, 0.1, None, (7, 100)),
]
PARAMS = ("W1", "b1", "gamma", "beta", "W2", "b2")
ROWS = 16           # rows of d W1 / d W2 stored (the size limit of a committed file); the tests compare those rows


def import_head():
    sys.path.insert(0, os.path.join(HERE, "_shims"))
    sys.path.insert(0, REF)
    if "matplotlib" not in sys.modules:                      # classifier.py imports pyplot at the top and never uses it here
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    import core.configs  # noqa: F401
    import core.utils.hyperbolic  # noqa: F401
    if "core.models" not in sys.modules:                     # the package object without executing its __init__
        pkg = types.ModuleType("core.models")
        pkg.__path__ = [os.path.join(REF, "core", "models")]
        sys.modules["core.models"] = pkg
    spec = importlib.util.spec_from_file_location("core.models.classifier", os.path.join(REF, "core", "models", "classifier.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["core.models.classifier"] = mod
    spec.loader.exec_module(mod)
    return mod.DepthwiseSeparableASPP_Hyper


def build(Head, C, seed, training, momentum, clamped):
    torch.manual_seed(seed)
    head = Head(32, [1, 6], [0, 6], 5, torch.nn.BatchNorm2d, C, True)
    lin1, bn, _, lin2 = head.wn_mlp
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        lin1.weight.copy_(torch.round(torch.randn(C, C, generator=g) / C ** 0.5 * 256) / 256)   # exact in float16
        lin1.bias.copy_(torch.randn(C, generator=g) * 0.3 + 0.5)
        bn.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
        lin2.weight.copy_(torch.round(torch.randn(C, C, generator=g) / C ** 0.5 * 256) / 256)
        lin2.bias.copy_(torch.rand(C, generator=g) + 0.5)
        for c in clamped:
            lin2.bias[c] = -20.0                                     # w_b < 1e-5 in every image: the clamp holds
        bn.running_mean.copy_(0.5 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
        bn.num_batches_tracked.fill_(2)
    bn.momentum = momentum
    head.train(training)
    for child_name, child in head.named_children():             # the layers in front of conv_reduce only feed the replaced output
        if child_name != "wn_mlp":
            child.eval()
    return head


def run(head, x, gy):
    """(y, d x, parameter gradients, running mean, running var) of one forward / backward of the reference head"""
    x = x.clone().requires_grad_(True)
    lin1, bn, _, lin2 = head.wn_mlp
    captured = {}
    hook = head.conv_reduce.register_forward_hook(lambda mod, inp, out: x)
    expmap = head.mapper.expmap

    def capture(t, *a, **k):
        captured["y"] = t
        return expmap(t, *a, **k)
    head.mapper.expmap = capture
    try:
        low = torch.zeros(x.shape[0], 256, 2, 2, dtype=x.dtype)
        top = torch.zeros(x.shape[0], 32, 1, 1, dtype=x.dtype)
        head({"low": low, "out": top})
    finally:
        hook.remove()
        head.mapper.expmap = expmap
    y = captured["y"]
    params = [lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias]
    grads = torch.autograd.grad((y * gy).sum(), [x] + params)
    return y.detach(), grads[0], grads[1:], bn.running_mean.clone(), bn.running_var.clone()


def main():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    Head = import_head()
    out = {}
    for n, (name, C, B, (h, w), training, momentum, zero, clamped) in enumerate(CASES):
        seed = 500 + n
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((B, C, h, w)).astype(np.float32)
        if zero is not None:
            x[:, zero] = 0.0
        gy = rng.standard_normal((B, C, h, w)).astype(np.float32)
        head32 = build(Head, C, seed, training, momentum, clamped)
        head64 = build(Head, C, seed, training, momentum, clamped).double()
        lin1, bn, _, lin2 = head32.wn_mlp
        params = [lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias]
        out[name + "/x"] = x
        out[name + "/g"] = gy
        for p, t in zip(PARAMS, params):
            out[name + "/" + p] = t.detach().numpy().astype(np.float16 if p in ("W1", "W2") else np.float32)
        out[name + "/running_mean_in"] = bn.running_mean.numpy().copy()
        out[name + "/running_var_in"] = bn.running_var.numpy().copy()
        out[name + "/meta"] = np.array([C, B, h, w, int(training), -1 if momentum is None else 0, 2], np.int64)
        out[name + "/momentum"] = np.array(np.nan if momentum is None else momentum, np.float64)
        for tag, head, dt in (("f32", head32, torch.float32), ("f64", head64, torch.float64)):
            y, dx, grads, rm, rv = run(head, torch.from_numpy(x).to(dt), torch.from_numpy(gy).to(dt))
            out["%s/%s/y" % (name, tag)] = y.numpy().astype(np.float32)
            out["%s/%s/dx" % (name, tag)] = dx.numpy().astype(np.float32)
            for p, gp in zip(PARAMS, grads):
                gp = gp.numpy()
                if p in ("W1", "W2"):
                    gp = gp[:ROWS]
                out["%s/%s/d%s" % (name, tag, p)] = gp.astype(np.float64 if gp.ndim == 1 else np.float32)
            out["%s/%s/running_mean" % (name, tag)] = rm.numpy().astype(np.float64)
            out["%s/%s/running_var" % (name, tag)] = rv.numpy().astype(np.float64)
        print(name, "y max", float(np.abs(out[name + "/f64/y"]).max()), "dx max", float(np.abs(out[name + "/f64/dx"]).max()))
    path = os.path.join(OUT, "hfr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
