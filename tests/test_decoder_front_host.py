"""CPU checks of the fused front of the v3+ decoder (halo_upcat_* of halo_dwconv.hip, halo_amd.dwconv.upsample_cat_depthwise_bn_relu,
halo_amd.hooks.use_fused_decoder_front): the entry points are declared, listed and exported under ABI >= 12, the argument checks
refuse before any launch, the envelope decisions, and the composition that CPU tensors run."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT
import dwconv_ref as R

SYMBOLS = ("halo_upcat_dwconv3x3_affine_relu_fwd", "halo_upcat_dwconv3x3_affine_relu_bwd_data", "halo_upcat_dwconv3x3_affine_relu_bwd_weight")
E_ARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(halo_upcat_\w+)\s*\(", code)) == set(SYMBOLS)
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
    version = int(re.search(r"#define HALO_ABI_VERSION (\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 12 and _lib.lib().halo_version() == version
    # pointers, then sizes, then (workspace and) the stream: the argument counts of the three declarations
    assert [len(_lib.SIGNATURES[s][1]) for s in SYMBOLS] == [14, 12, 16]


def test_argument_checks_refuse_before_any_launch():
    """every pointer is one HOST buffer: a check that went missing would end in a launch error or worse, never in these codes"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd, wgt = (getattr(L, s) for s in SYMBOLS)

    def refused(rc, code, word):
        msg = L.halo_last_error().decode()
        assert rc == code and word in msg and "halo_upcat_dwconv3x3_affine_relu" in msg, (rc, msg)

    refused(fwd(None, p, p, p, p, p, 1, 2, 1, 2, 2, 4, 4, None), E_ARG, "null")               # no a
    refused(fwd(p, None, p, p, p, p, 1, 2, 1, 2, 2, 4, 4, None), E_ARG, "null")               # no s
    refused(fwd(p, p, p, p, None, p, 1, 2, 1, 2, 2, 4, 4, None), E_ARG, "null")               # no shift
    refused(fwd(p, p, p, p, p, None, 1, 2, 1, 2, 2, 4, 4, None), E_ARG, "null")               # no y
    refused(fwd(p, p, p, p, p, p, 1, 2, 1, 5, 2, 4, 4, None), E_ARG, "smaller")               # H < h
    refused(fwd(p, p, p, p, p, p, 1, 2, 1, 2, 5, 4, 4, None), E_ARG, "smaller")               # W < w
    refused(fwd(p, p, p, p, p, p, 1, 0, 0, 2, 2, 4, 4, None), E_ARG, "empty")                 # Ca + Cs = 0
    refused(fwd(p, p, p, p, p, p, 0, 2, 1, 2, 2, 4, 4, None), E_ARG, "empty")
    refused(fwd(p, p, p, p, p, p, 1, 2, 1, 0, 2, 4, 4, None), E_ARG, "empty")                 # h = 0
    refused(fwd(p, p, p, p, p, p, 1, 2, 1, 2, 2, 1 << 25, 4, None), E_UNSUPPORTED, "planes")
    refused(bwd(None, p, p, p, p, p, 1, 2, 1, 4, 4, None), E_ARG, "null")                     # no g
    refused(bwd(p, None, p, p, p, p, 1, 2, 1, 4, 4, None), E_ARG, "null")                     # no y
    refused(bwd(p, p, p, p, p, p, 1, 0, 0, 4, 4, None), E_ARG, "empty")
    assert bwd(p, p, p, p, None, None, 1, 2, 1, 4, 4, None) == 0                              # no gradient wanted: nothing is launched
    n = L.halo_dwconv_workspace_bytes(1, 3, 4, 4, 1)
    assert n >= 3 * 9 * 8
    refused(wgt(p, p, p, p, p, p, 1, 2, 1, 2, 2, 4, 4, p, n - 1, None), E_WORKSPACE, "workspace")    # short
    refused(wgt(p, p, p, p, p, p, 1, 2, 1, 2, 2, 4, 4, None, n, None), E_WORKSPACE, "workspace")     # none
    refused(wgt(p, p, p, p, p, None, 1, 2, 1, 2, 2, 4, 4, p, n, None), E_ARG, "null")                # no g_w
    refused(wgt(p, p, p, p, p, p, 1, 2, 1, 5, 2, 4, 4, p, n, None), E_ARG, "smaller")
    refused(wgt(p, p, p, p, p, p, 1, 0, 0, 2, 2, 4, 4, p, n, None), E_ARG, "empty")


class _OnDevice:
    """describes a float32 ROCm tensor without one: upcat_fallback_reason reads attributes only"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)


def _modules(C=5, d=1, bias=False):
    return nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=bias), R.FrozenBatchNorm2d(C)


def test_envelope_decisions(monkeypatch):
    from halo_amd.dwconv import upcat_fallback_reason as why
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    a, s = _OnDevice(2, 3, 4, 5), _OnDevice(2, 2, 8, 10)
    conv, bn = _modules()
    assert why(a, s, conv, bn) is None                                                     # the served configuration
    assert why(_OnDevice(2, 3, 8, 10), s, conv, bn) is None                                # h = H, w = W
    assert "dilation" in why(a, s, *_modules(d=2))
    assert "bias" in why(a, s, _modules(bias=True)[0], bn)
    assert "batch statistics" in why(a, s, conv, nn.BatchNorm2d(5))
    assert why(a, s, conv, nn.BatchNorm2d(5, affine=False).eval()) is None
    assert "images" in why(_OnDevice(1, 3, 4, 5), s, conv, bn)                             # mismatched B
    assert "smaller" in why(_OnDevice(2, 3, 9, 5), s, conv, bn)                            # H < h
    assert "smaller" in why(_OnDevice(2, 3, 4, 11), s, conv, bn)                           # W < w
    assert "channels" in why(a, _OnDevice(2, 3, 8, 10), conv, bn)                          # Ca + Cs is not the conv's C
    assert "empty" in why(_OnDevice(2, 0, 4, 5), _OnDevice(2, 5, 8, 10), conv, bn)
    assert "(B, C, H, W)" in why(_OnDevice(3, 4, 5), s, conv, bn)
    assert "plane" in why(_OnDevice(2, 3, 1, 1), _OnDevice(2, 2, 1 << 25, 1), conv, bn)    # dw_check's size limits
    assert "planes to resize" in why(_OnDevice(1 << 20, (1 << 20) + 1, 1, 1), _OnDevice(1 << 20, 1, 1, 1), *_modules((1 << 20) + 2))
    half = _OnDevice(2, 3, 4, 5)
    half.dtype = torch.float64
    assert "float32" in why(half, s, conv, bn)
    elsewhere = _OnDevice(2, 2, 8, 10)
    elsewhere.device = torch.device("meta")
    assert " on " in why(a, elsewhere, conv, bn)                                           # two devices
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert "autocast" in why(a, s, conv, bn)
    monkeypatch.undo()
    assert "device" in why(torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 8, 10), conv, bn)    # CPU tensors
    assert "float32" in why(torch.zeros(2, 3, 4, 5, dtype=torch.float64), torch.zeros(2, 2, 8, 10, dtype=torch.float64), conv, bn)


@pytest.mark.parametrize("kind", ["frozen", "train_bn", "dilated"])
def test_cpu_tensors_run_the_composition(kind):
    """outside the envelope the operator is the statements the head runs today, written out here"""
    from halo_amd.dwconv import upsample_cat_depthwise_bn_relu
    torch.manual_seed(4)
    d = 2 if kind == "dilated" else 1
    conv = nn.Conv2d(5, 5, 3, 1, d, d, groups=5, bias=False)
    if kind == "train_bn":
        bn = nn.BatchNorm2d(5)
    else:
        bn = R.FrozenBatchNorm2d(5)
        bn.weight.copy_(torch.rand(5) + 0.5), bn.bias.copy_(torch.randn(5)), bn.running_mean.copy_(torch.randn(5)), bn.running_var.copy_(torch.rand(5) + 0.5)
    a = torch.randn(2, 3, 4, 5, requires_grad=True)
    s = torch.randn(2, 2, 9, 10, requires_grad=True)
    g = torch.randn(2, 5, 9, 10)
    act = nn.ReLU(inplace=True)
    y = upsample_cat_depthwise_bn_relu(a, s, conv, bn, act)
    got = torch.autograd.grad(y, [a, s, conv.weight], g)
    if kind == "train_bn":
        bn = nn.BatchNorm2d(5)                                                             # fresh running statistics, as the first call saw them
    x = torch.cat([F.interpolate(a, size=(9, 10), mode="bilinear", align_corners=True), s], dim=1)
    want = act(bn(conv(x)))
    assert torch.equal(y, want)
    for t1, t2 in zip(got, torch.autograd.grad(want, [a, s, conv.weight], g)):
        assert torch.equal(t1, t2)


def test_hook_marks_only_classes_with_a_package_forward():
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import fused_v3plus_hyper_forward, use_fused_decoder_front

    class Plain(nn.Module):
        def forward(self, x):
            return x

    class Head(nn.Module):
        forward = v3plus_hyper_forward

    class Reweighting(nn.Module):
        forward = fused_v3plus_hyper_forward

    class Child(Head):
        pass

    for bad in (Plain, nn.Conv2d, Plain(), "Head"):
        with pytest.raises(TypeError):
            use_fused_decoder_front(bad)
    assert not hasattr(Head, "_halo_fused_decoder_front")
    assert use_fused_decoder_front(Head) is Head and use_fused_decoder_front(Head) is Head and Head._halo_fused_decoder_front is True
    assert use_fused_decoder_front(Reweighting) is Reweighting and use_fused_decoder_front(Child) is Child
    assert Head.forward is v3plus_hyper_forward and Reweighting.forward is fused_v3plus_hyper_forward      # the forwards stay bound
