"""Wide acquisition windows (size = 2 RADIUS_K + 1 up to the module's default 33) without a GPU:

  * the route query -- halo_window_route / floating_region.window_route say which kernels serve a window pass, and the library's
    launchers branch on the same function;
  * the numeric contract at wide windows -- the oracle's box sum is nn.Conv2d's with an all-ones kernel and its window impurity is
    the one-hot / grouped-convolution / torch.sum statement of compute_region_impurity, bit for bit, at 5 x 5, 17 x 17 and 33 x 33.
    The device kernels are compared with the oracle (tests/test_gpu_wide_windows.py); this file ties the oracle to ATen, so that a
    failure here after a torch upgrade reads as "ATen changed", not as a kernel bug.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.halo_oracle as ho
from conftest import ROOT

PADS = ("zeros", "reflect", "replicate", "circular")


def bits_differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((~((a == b) | ((a != a) & (b != b)))).sum())


# ------------------------------------------------------------------ route query
def test_header_declares_and_library_exports_the_route_query():
    from halo_amd import _build, _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+halo_window_route\s*\(\s*int what,\s*int ksize,\s*int pad_mode,\s*int64_t bins,\s*int64_t H,\s*int64_t W\)", text)
    assert "#define HALO_WINDOW_BOX 0" in text and "#define HALO_WINDOW_HIST 1" in text
    assert hasattr(ctypes.CDLL(_build.build()), "halo_window_route")
    assert "halo_window_route" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 13 and _lib.lib().halo_version() == 13 and "#define HALO_ABI_VERSION 13" in text


def test_window_route_table():
    from halo_amd import _lib
    from halo_amd.core.active.floating_region import window_route
    for what in ("box", "hist"):
        for k in (5, 7, 9, 17, 33):
            for pad in PADS:
                for bins in (16, 19):
                    assert window_route(what, k, pad, bins) == "tiled", (what, k, pad, bins)
                    assert window_route(what, k, pad, bins, shape=(70, 130)) == "tiled"
        assert window_route(what, 3, "zeros") == "tile3"
        for pad in PADS[1:]:                                   # 3 x 3 under the other padding modes stays on the generic kernels
            assert window_route(what, 3, pad) == "generic"
        assert window_route(what, 35) == "generic" and window_route(what, 101, "replicate") == "generic"
        assert window_route(what, 1) == "generic"
        for even in (4, 32):
            with pytest.raises(_lib.HaloHipError, match="odd"):
                window_route(what, even)
    assert window_route("hist", 5, bins=32) == "tiled" and window_route("hist", 33, bins=2) == "tiled"
    assert window_route("hist", 5, bins=33) == "generic" and window_route("hist", 5, bins=100) == "generic"
    assert window_route("box", 5, bins=100) == "tiled"                    # the box sum has no bins
    assert window_route("box", 3, shape=(64, 130)) == "generic"           # the 3 x 3 box kernels need a width that is a multiple of 4
    assert window_route("hist", 3, shape=(64, 130)) == "tile3"
    L = _lib.lib()                                                         # the C entry itself
    assert L.halo_window_route(_lib.WINDOW["hist"], 33, _lib.PAD["circular"], 19, 1024, 2048) == 2
    assert L.halo_window_route(_lib.WINDOW["box"], 3, _lib.PAD["zeros"], 19, 1024, 2048) == 1
    assert L.halo_window_route(7, 5, 0, 19, 8, 8) < 0 and L.halo_window_route(0, 5, 9, 19, 8, 8) < 0 and L.halo_window_route(0, 5, 0, 19, 0, 8) < 0
    with pytest.raises(ValueError):
        window_route("box", 5, "mirror")


# ------------------------------------------------------------------ the contract at wide windows
H, W = 128, 192                     # above the 20 480 pixels at which ATen's convolution takes the path the reference's sizes take


@pytest.mark.parametrize("k", [5, 17, 33])
@pytest.mark.parametrize("pad", PADS)
def test_oracle_box_sum_is_atens_conv_at_wide_windows(k, pad):
    assert H * W > 20480
    g = torch.Generator().manual_seed(k)
    x = torch.rand(H, W, generator=g)
    conv = torch.nn.Conv2d(1, 1, k, stride=1, padding=k // 2, bias=False, padding_mode=pad)
    conv.weight.data.fill_(1.0)
    with torch.no_grad():
        want = conv(x[None, None])[0, 0].numpy()
    assert bits_differ(ho.box_sum(x.numpy(), k, pad), want) == 0


def _label_maps(K):
    rng = np.random.default_rng(K)
    noisy = rng.integers(0, K, (H, W)).astype(np.int64)
    blocky = np.kron(rng.integers(0, K, (H // 16, W // 16)), np.ones((16, 16), np.int64)).astype(np.int64)
    return {"noisy": noisy, "blocky": blocky}


@pytest.mark.parametrize("k", [5, 17, 33])
@pytest.mark.parametrize("kind", ["noisy", "blocky"])
def test_oracle_region_impurity_is_the_one_hot_conv_statement_at_wide_windows(k, kind):
    """compute_region_impurity as the reference states it: one-hot planes, a depthwise all-ones k x k convolution, the count as
    torch.sum over the planes, the fractions, torch.sum of -d log(d + 1e-6) over the planes, / log K -- every op torch's own except
    the logarithm, which is the contract's correctly rounded one (MKL's differs between instruction sets, tests/test_aten_exact.py)."""
    K = 19
    pred = torch.from_numpy(_label_maps(K)[kind])
    one_hot = F.one_hot(pred, num_classes=K).float().permute(2, 0, 1)[None]
    conv = torch.nn.Conv2d(K, K, k, stride=1, padding=k // 2, bias=False, groups=K)
    conv.weight.data.fill_(1.0)
    with torch.no_grad():
        summary = conv(one_hot)
        count = torch.sum(summary, dim=1, keepdim=True)
        dist = summary / count
        log = torch.from_numpy(ho.logf((dist + 1e-6).numpy()))
        want = torch.sum(-dist * log, dim=1, keepdim=True) / math.log(K)
    imp, cnt = ho.region_impurity(pred.numpy(), K, k)
    assert bits_differ(cnt, count.numpy()) == 0
    assert bits_differ(imp, want.numpy()) == 0
