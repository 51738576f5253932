"""numpy float64 evaluation of the depthwise conv + frozen norm + ReLU statements and of the derived error bounds of
tests/test_gpu_dwconv.py, over the cases of tests/golden/dwconv.npz (written by tests/golden/make_dwconv_fixtures.py from the
reference's own modules; tests/test_dwconv_host.py holds this evaluator to the stored channels)."""
import os

import numpy as np

from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "dwconv.npz")
U = 2.0 ** -24
FROZEN, BATCHNORM = 0, 1


def case_names():
    z = np.load(FIX)
    return sorted({k.split("/")[0] for k in z.files})


def load(name):
    z = np.load(FIX)
    d = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
    d["x"] = d["x_q"].astype(np.float32) / 4
    d["g"] = d["g_q"].astype(np.float32) / 4
    d["B"], d["C"], d["H"], d["W"], d["d"], d["kind"] = (int(v) for v in d["meta"])
    return d


def shifted(a, dy, dx):
    """out[..., i, j] = a[..., i + dy, j + dx], zero outside the plane"""
    H, W = a.shape[-2:]
    out = np.zeros_like(a)
    i0, i1 = max(0, -dy), min(H, H - dy)
    j0, j1 = max(0, -dx), min(W, W - dx)
    if i0 < i1 and j0 < j1:
        out[..., i0:i1, j0:j1] = a[..., i0 + dy:i1 + dy, j0 + dx:j1 + dx]
    return out


def scale_shift64(c):
    var = c["running_var"].astype(np.float64)
    if c["kind"] == BATCHNORM:
        var = var + float(c["eps"])
    scale = c["weight"].astype(np.float64) / np.sqrt(var)
    return scale, c["bias"].astype(np.float64) - c["running_mean"].astype(np.float64) * scale


def taps(c):
    d = c["d"]
    w = c["w"].astype(np.float64).reshape(c["C"], 9)
    return [(k, (k // 3 - 1) * d, (k % 3 - 1) * d, w[None, :, k, None, None]) for k in range(9)]


def forward(c):
    """(pre, bound): the float64 pre-activation and 15u (|scale| sum_k |w_k| |x_k| + |bias| + |running_mean scale|)"""
    x = c["x"].astype(np.float64)
    scale, shift = scale_shift64(c)
    conv, mag = np.zeros_like(x), np.zeros_like(x)
    for _, dy, dx, wk in taps(c):
        xs = shifted(x, dy, dx)
        conv += wk * xs
        mag += np.abs(wk) * np.abs(xs)
    v = lambda t: t[None, :, None, None]
    pre = conv * v(scale) + v(shift)
    bound = 15 * U * (np.abs(v(scale)) * mag + np.abs(v(c["bias"].astype(np.float64))) + np.abs(v(c["running_mean"].astype(np.float64) * scale)))
    return pre, bound


def grad_x(c, mask):
    """(g_x, bound) with the given ReLU mask: g_x[p] = sum_k w_k gp[p - k d], 15u |scale| sum_k |w_k| |g mask| at the same positions"""
    scale, _ = scale_shift64(c)
    gm = c["g"].astype(np.float64) * mask
    gp = gm * scale[None, :, None, None]
    gx, mag = np.zeros_like(gp), np.zeros_like(gp)
    for _, dy, dx, wk in taps(c):
        gx += wk * shifted(gp, -dy, -dx)
        mag += np.abs(wk) * shifted(np.abs(gm), -dy, -dx)
    return gx, 15 * U * np.abs(scale)[None, :, None, None] * mag


def grad_w(c, mask):
    """(g_w (C, 1, 3, 3), bound) with the given mask: g_w[c, k] = sum_{b,p} gp x[p + k d], 8u sum |gp| |x|"""
    scale, _ = scale_shift64(c)
    x = c["x"].astype(np.float64)
    gp = c["g"].astype(np.float64) * mask * scale[None, :, None, None]
    gw, mag = np.zeros((c["C"], 9)), np.zeros((c["C"], 9))
    for k, dy, dx, _ in taps(c):
        xs = shifted(x, dy, dx)
        gw[:, k] = (gp * xs).sum(axis=(0, 2, 3))
        mag[:, k] = (np.abs(gp) * np.abs(xs)).sum(axis=(0, 2, 3))
    return gw.reshape(c["C"], 1, 3, 3), (8 * U * mag).reshape(c["C"], 1, 3, 3)


def modules(c, device="cpu", dtype=None):
    """(conv, bn) torch modules of the case: a stand-in FrozenBatchNorm2d with the reference's buffer names, or eval BatchNorm2d"""
    import torch
    import torch.nn as nn
    C, d = c["C"], c["d"]
    conv = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False)
    if c["kind"] == FROZEN:
        bn = FrozenBatchNorm2d(C)
    else:
        bn = nn.BatchNorm2d(C, eps=float(c["eps"])).eval()
        for p in bn.parameters():
            p.requires_grad_(False)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(c["w"]))
        for n in ("weight", "bias", "running_mean", "running_var"):
            getattr(bn, n).copy_(torch.from_numpy(c[n]))
    conv, bn = conv.to(device), bn.to(device)
    if dtype is not None:
        conv, bn = conv.to(dtype), bn.to(dtype)
    return conv, bn


def _frozen_class():
    import torch
    import torch.nn as nn

    class FrozenBatchNorm2d(nn.Module):
        """a stand-in with the reference's class name, buffer names and forward statements (core/models/layers.py)"""

        def __init__(self, n):
            super().__init__()
            for name, v in (("weight", torch.ones(n)), ("bias", torch.zeros(n)), ("running_mean", torch.zeros(n)), ("running_var", torch.ones(n))):
                self.register_buffer(name, v)

        def forward(self, x):
            scale = self.weight * self.running_var.rsqrt()
            bias = self.bias - self.running_mean * scale
            return x * scale.reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)
    return FrozenBatchNorm2d


FrozenBatchNorm2d = _frozen_class()
