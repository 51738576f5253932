#!/usr/bin/env python3
"""Generate tests/golden/dwconv.npz by RUNNING the reference's own DepthwiseSeparableConv2d and FrozenBatchNorm2d on the CPU.

Run where the reference's tree exists (it never travels to the GPU box):

    python tests/golden/make_dwconv_fixtures.py         # writes tests/golden/dwconv.npz

What runs: core/models/classifier.py's DepthwiseSeparableConv2d(C, C, 3, 1, d, d, False, norm_layer) (imported as
make_hfr_fixtures.py imports the head) with norm_layer = core/models/layers.py's FrozenBatchNorm2d, or an eval-mode
torch.nn.BatchNorm2d for the one case of that kind.  Its depthwise half -- depthwise_conv, depthwise_bn, depthwise_activate --
is evaluated on a .double() copy (pre = bn(conv(x)), y = relu(pre), torch.autograd.grad of sum(g * y) for x and conv.weight: the
"float64 evaluation" the tests hold the device to) and, forward only, as the stock float32 modules.  Only DATA is written.

Cases (name, d, shape): the dilations of the v3+ head at small planes, the 560-channel decoder width, a W that is no multiple
of 4, a plane smaller than d, and eval-mode BatchNorm2d.  Buffers are non-trivial: weight in [0.25, 1.75], running_var in
[0.3, 1.8], non-zero running_mean and bias.

A committed file stays below 1 MiB, so: x and g are multiples of 1/4 in [-3, 3], stored as int8 (`x_q`, `g_q`: x = x_q / 4); the
per-element float64 results (pre, g_x) and the stock float32 forward are stored for the channels listed in `chans` only; g_w
(float64, with the float64 ReLU mask) is stored for every channel.  tests/dwconv_ref.py evaluates the same statements in numpy
float64 for every channel; tests/test_dwconv_host.py holds that evaluator to the stored channels.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("HALO_FIXTURE_OUT", HERE)
sys.path.insert(0, HERE)
from make_fixtures import REF  # noqa: E402  (the reference's tree: $HALO_REFERENCE)
from make_hfr_fixtures import import_head  # noqa: E402

FROZEN, BATCHNORM = 0, 1
CASES = [  # name, d, (B, C, H, W), kind, stored channels
    ("d1", 1, (2, 24, 20, 36), FROZEN, 4),
    ("d6", 6, (2, 16, 24, 40), FROZEN, 3),
    ("d12", 12, (1, 16, 40, 44), FROZEN, 3),
    ("d18", 18, (1, 8, 40, 48), FROZEN, 3),
    ("d1_c560", 1, (2, 560, 12, 20), FROZEN, 8),
    ("w13_d2", 2, (2, 8, 11, 13), FROZEN, 8),
    ("tiny_d5", 5, (2, 8, 3, 4), FROZEN, 8),
    ("bn_eval_d3", 3, (2, 12, 10, 16), BATCHNORM, 4),
]


def import_blocks():
    import_head()                                            # leaves the reference's classifier module in sys.modules
    block = sys.modules["core.models.classifier"].DepthwiseSeparableConv2d
    spec = importlib.util.spec_from_file_location("core.models.layers", os.path.join(REF, "core", "models", "layers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return block, mod.FrozenBatchNorm2d


def build(Block, norm, C, d, seed):
    torch.manual_seed(seed)
    blk = Block(C, C, 3, 1, d, d, False, norm_layer=norm)
    g = torch.Generator().manual_seed(seed + 1)
    bn = blk.depthwise_bn
    with torch.no_grad():
        bn.weight.copy_(0.25 + 1.5 * torch.rand(C, generator=g))
        bn.bias.copy_(0.4 * torch.randn(C, generator=g) + 0.1)
        bn.running_mean.copy_(0.5 * torch.randn(C, generator=g) + 0.2)
        bn.running_var.copy_(0.3 + 1.5 * torch.rand(C, generator=g))
    return blk.eval()


def depthwise_half(blk, x, g=None):
    """(pre, y, g_x, g_w) of the block's first three statements"""
    x = x.clone().requires_grad_(g is not None)
    pre = blk.depthwise_bn(blk.depthwise_conv(x))
    y = blk.depthwise_activate(pre.clone())
    if g is None:
        return pre.detach(), y.detach(), None, None
    gx, gw = torch.autograd.grad((y * g).sum(), [x, blk.depthwise_conv.weight])
    return pre.detach(), y.detach(), gx, gw


def main():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    Block, Frozen = import_blocks()
    out = {}
    for n, (name, d, (B, C, H, W), kind, nstored) in enumerate(CASES):
        seed = 800 + n
        rng = np.random.default_rng(seed)
        xq = np.clip(np.round(rng.standard_normal((B, C, H, W)) * 4), -12, 12).astype(np.int8)
        gq = np.clip(np.round(rng.standard_normal((B, C, H, W)) * 4), -12, 12).astype(np.int8)
        norm = Frozen if kind == FROZEN else torch.nn.BatchNorm2d
        blk32 = build(Block, norm, C, d, seed)
        blk64 = build(Block, norm, C, d, seed).double()
        bn = blk32.depthwise_bn
        chans = np.unique(np.linspace(0, C - 1, min(nstored, C)).round().astype(np.int64))
        x32, g32 = torch.from_numpy(xq.astype(np.float32) / 4), torch.from_numpy(gq.astype(np.float32) / 4)
        pre64, y64, gx64, gw64 = depthwise_half(blk64, x32.double(), g32.double())
        _, y32, _, _ = depthwise_half(blk32, x32)
        assert torch.equal(y64, pre64.clamp(min=0))
        out[name + "/x_q"], out[name + "/g_q"] = xq, gq
        out[name + "/w"] = blk32.depthwise_conv.weight.detach().numpy().copy()
        for p in ("weight", "bias", "running_mean", "running_var"):
            out[name + "/" + p] = getattr(bn, p).detach().numpy().copy()
        out[name + "/eps"] = np.array(np.nan if kind == FROZEN else bn.eps, np.float64)
        out[name + "/meta"] = np.array([B, C, H, W, d, kind], np.int64)
        out[name + "/chans"] = chans
        out[name + "/pre64"] = pre64.numpy()[:, chans].copy()
        out[name + "/gx64"] = gx64.numpy()[:, chans].copy()
        out[name + "/y32"] = y32.numpy()[:, chans].copy()
        out[name + "/gw64"] = gw64.numpy().copy()
        print(name, "pre max", float(pre64.abs().max()), "positive", float((pre64 > 0).double().mean()), "g_w max", float(gw64.abs().max()))
    path = os.path.join(OUT, "dwconv.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
