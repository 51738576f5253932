"""CPU checks of the differentiable bilinear resize (halo_resize.hip, halo_amd.resize, halo_amd.hooks.use_device_resize): the new
entry point is exported, declared and bound at ABI 10; the argument checks refuse before any launch; the Python surface raises
the stated error types before touching a device; and the yardstick of tests/test_gpu_resize.py -- a numpy statement of the
adjoint built from make_taps, float32 arithmetic restated with np.float32 -- is pinned to torch's CPU autograd of
F.interpolate(mode='bilinear', align_corners=True).  The kernel itself is held to that operator in tests/test_gpu_resize.py."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resize_ref import make_taps, numpy_adjoint, scale_of, terms_bound, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "halo_bilinear_upsample_bwd"


def test_entry_point_is_exported_declared_and_bound_at_abi_10():
    from halo_amd import _build, _lib
    h = ctypes.CDLL(_build.build())
    assert hasattr(h, SYMBOL)
    assert SYMBOL in _lib.SIGNATURES and _lib.SIGNATURES[SYMBOL] == _lib.SIGNATURES["halo_bilinear_upsample"]
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    assert "int %s(const void *grad_out, void *grad_in, int dtype, int64_t planes" % SYMBOL in text
    assert "#define HALO_ABI_VERSION %d" % _lib.ABI_VERSION in text
    assert _lib.ABI_VERSION >= 10 and _lib.lib().halo_version() == _lib.ABI_VERSION
    assert callable(getattr(_lib.lib(), SYMBOL))


def test_argument_checks_refuse_before_launching():
    """null pointers, empty shapes, an unknown dtype and a downsampling geometry return HALO_E_ARG with host addresses that are
    never dereferenced: nothing is launched"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    f = L.halo_bilinear_upsample_bwd
    ok = dict(dtype=0, planes=2, h=4, w=8, H=16, W=32)

    def call(go=a, gi=a, **kw):
        k = dict(ok, **kw)
        return f(go, gi, k["dtype"], k["planes"], k["h"], k["w"], k["H"], k["W"], None)

    assert call(go=None) == -1 and call(gi=None) == -1
    for kw in ({"planes": 0}, {"h": 0}, {"w": 0}, {"H": 0}, {"W": 0}, {"dtype": 2}, {"dtype": -1}, {"H": 3}, {"W": 7},
               {"H": 1 << 31}, {"W": 1 << 31}):
        assert call(**kw) == -1, kw                                  # HALO_E_ARG
    call(H=3)
    assert "smaller" in L.halo_last_error().decode()


def test_python_surface_raises_before_the_library():
    from halo_amd.resize import bilinear_resize, resize_or_interpolate
    x = torch.zeros((1, 2, 4, 8))
    with pytest.raises(ValueError):
        bilinear_resize(x, (16, 32))                                 # a CPU tensor: no CPU route
    with pytest.raises(TypeError):
        bilinear_resize(x.half(), (16, 32))
    with pytest.raises(TypeError):
        bilinear_resize(x.long(), (16, 32))
    with pytest.raises(TypeError):
        bilinear_resize(x.numpy(), (16, 32))
    with pytest.raises(ValueError):
        bilinear_resize(x, (3, 32))
    # the callers' form never raises over an unserved operand: it is F.interpolate then
    want = F.interpolate(x + 1.0, size=(16, 32), mode="bilinear", align_corners=True)
    assert torch.equal(resize_or_interpolate(x + 1.0, (16, 32)), want)
    assert resize_or_interpolate(x, (2, 4)).shape == (1, 2, 2, 4)   # downsampling: F.interpolate serves it


def test_size_refusal_is_decided_on_the_host_for_device_like_operands():
    """H < h / W < w are refused by the same host-side predicate whatever the device: exercised directly"""
    from halo_amd.resize import _refusal

    class Dev(object):                                              # what _refusal reads of a device tensor
        dtype, is_cuda, shape, device = torch.float32, True, (2, 3, 4, 8), "cuda:0"

        def dim(self):
            return 4

    import unittest.mock as mock
    with mock.patch("torch.is_tensor", lambda t: True):
        assert _refusal(Dev(), (16, 32)) is None
        assert _refusal(Dev(), (4, 8)) is None
        assert _refusal(Dev(), (3, 32))[0] is ValueError and _refusal(Dev(), (16, 7))[0] is ValueError
        assert _refusal(Dev(), 16)[0] is ValueError


def test_bilinear_align_corners_still_refuses_gradients_with_its_message():
    from halo_amd.core.utils.hyperbolic import _no_grad_only, bilinear_align_corners
    with pytest.raises(NotImplementedError, match="inference-only"):
        _no_grad_only(torch.zeros(1, requires_grad=True))
    assert "bilinear_resize" in bilinear_align_corners.__doc__


def test_use_device_resize_marks_heads_and_learners():
    import torch.nn as nn
    from halo_amd.core.models.classifier import device_resize, v2_hyper_forward, v3plus_hyper_forward
    from halo_amd.hooks import fused_v3plus_hyper_forward, use_device_resize, use_fused_feature_reweighting, use_fused_training_losses
    from halo_amd.resize import resize_or_interpolate

    class Plain(nn.Module):
        def forward(self, x, size=None):
            return x

    with pytest.raises(TypeError, match="install"):
        use_device_resize(Plain)
    assert not hasattr(Plain, "_halo_device_resize")
    with pytest.raises(TypeError):
        use_device_resize(Plain())

    for fwd in (v2_hyper_forward, v3plus_hyper_forward, fused_v3plus_hyper_forward):
        head = type("Head", (nn.Module,), {"forward": fwd})
        assert device_resize(head()) is None
        assert use_device_resize(head) is head and use_device_resize(head) is head          # idempotent
        assert head._halo_device_resize is True and head.__dict__["forward"] is fwd
        assert device_resize(head()) is resize_or_interpolate
        assert device_resize(type("Sub", (head,), {})()) is resize_or_interpolate

    # either order with the other hooks
    first = use_fused_feature_reweighting(use_device_resize(type("A", (nn.Module,), {"forward": v3plus_hyper_forward})))
    second = use_device_resize(use_fused_feature_reweighting(type("B", (nn.Module,), {"forward": v3plus_hyper_forward})))
    for cls in (first, second):
        assert cls.forward is fused_v3plus_hyper_forward and cls._halo_device_resize is True

    class SourceTargetLearner(object):
        def training_step(self, batch, batch_idx):
            return None

    a = use_fused_training_losses(use_device_resize(type("L1", (SourceTargetLearner,), {})))
    b = use_device_resize(use_fused_training_losses(type("L2", (SourceTargetLearner,), {})))
    assert a._halo_device_resize is True and b._halo_device_resize is True
    assert not hasattr(SourceTargetLearner, "_halo_device_resize")                          # the base class is untouched


def test_unmarked_tail_keeps_todays_training_statements():
    """resize=None: hyper_head_tail's training branch is F.interpolate, literally (read from the source, no device needed)"""
    import inspect
    from halo_amd.core.models import classifier
    src = inspect.getsource(classifier.hyper_head_tail)
    assert src.count('F.interpolate(out, size=size, mode="bilinear", align_corners=True)') == 1
    assert src.count('F.interpolate(embed, size=size, mode="bilinear", align_corners=True)') == 1
    assert inspect.signature(classifier.hyper_head_tail).parameters["resize"].default is None


# ---------------------------------------------------------------- the yardstick: numpy adjoint from make_taps
def cpu_adjoint(g, h, w):
    t = torch.from_numpy(g)
    x = torch.zeros((1, g.shape[0], h, w), dtype=t.dtype, requires_grad=True)
    y = F.interpolate(x, size=g.shape[-2:], mode="bilinear", align_corners=True)
    (gx,) = torch.autograd.grad(y, x, t[None])
    return gx[0].numpy()


CASES = [(1, 1, 5, 9), (5, 7, 11, 20), (3, 4, 3, 17), (9, 16, 36, 65), (1, 6, 7, 6)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("h,w,H,W", CASES)
def test_numpy_adjoint_equals_torch_cpu_autograd(h, w, H, W, dtype):
    """h == 1, h == H (identity rows), border-coincident taps (every case's last row / column) and non-integer ratios"""
    rng = np.random.default_rng(h * 1000 + W)
    g = rng.standard_normal((3, H, W)).astype(dtype)
    got, want = numpy_adjoint(g, h, w), cpu_adjoint(g, h, w)
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    bound = 2 * (terms_bound(h, w, H, W) + 8) * u * cpu_adjoint(np.abs(g), h, w).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("%dx%d -> %dx%d %s: max err / bound = %.3g" % (h, w, H, W, np.dtype(dtype).name, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    ones = numpy_adjoint(np.ones((1, H, W), dtype=dtype), h, w)
    assert abs(float(ones.sum(dtype=np.float64)) - H * W) <= 2 * (terms_bound(h, w, H, W) + 8) * u * H * W


def test_kernel_ranges_cover_exactly_the_nonzero_weights():
    """The kernel sums a cell's rows over [first_at_least(i - 1), first_at_least(i + 1)) (halo_resize.hip): restated here, that
    range holds every output coordinate with a non-zero weight on the cell, and is contiguous"""
    for T in (np.float32, np.float64):
        for n_in, n_out in ((1, 1), (1, 9), (4, 4), (5, 11), (7, 20), (40, 160), (180, 720), (80, 1024), (33, 129)):
            s = scale_of(n_in, n_out, T)
            i0 = np.array([make_taps(o, s, n_in, T)[0] for o in range(n_out)])
            assert (np.diff(i0) >= 0).all()
            A = weights(n_in, n_out, T)
            for i in range(n_in):
                lo, hi = int(np.searchsorted(i0, i - 1, "left")), int(np.searchsorted(i0, i + 1, "left"))
                nz = np.nonzero(A[:, i])[0]
                assert nz.size and lo <= nz.min() and nz.max() < hi
                assert hi - lo <= 2 * math.ceil((n_out - 1) / max(n_in - 1, 1)) + 1
