"""CPU checks of the joint depthwise backward (halo_joint_* of halo_dwconv.hip, the joint_backward keyword of halo_amd.dwconv,
halo_amd.hooks.use_joint_depthwise_backward): the two entries are declared, listed and exported under ABI 13 beside the unchanged
symbol sets of the older host tests, every argument check refuses before a launch, the fallback reasons and the speed rule, the
torch statements outside the envelope, the keyword's default, and the hook's class checks."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import dwconv_ref as R

PLAIN, UPCAT = "halo_joint_dwconv3x3_affine_relu_bwd", "halo_joint_upcat_dwconv3x3_affine_relu_bwd"
E_ARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\b(halo_joint_\w+)\s*\(", code) == [PLAIN, UPCAT]
    assert "#define HALO_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13
    h = ctypes.CDLL(_build.build())
    for s in (PLAIN, UPCAT):
        assert s in _lib.SIGNATURES and hasattr(h, s), s
    assert _lib.lib().halo_version() == 13
    assert [len(_lib.SIGNATURES[s][1]) for s in (PLAIN, UPCAT)] == [15, 19]
    assert "HALO_E_ARG = -1, HALO_E_UNSUPPORTED = -2, HALO_E_WORKSPACE = -3" in text


def test_the_older_host_tests_still_see_their_symbol_sets():
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(halo_dwconv\w+)\s*\(", text)) == {
        "halo_dwconv_workspace_bytes", "halo_dwconv3x3_affine_relu_fwd", "halo_dwconv3x3_affine_relu_bwd_data",
        "halo_dwconv3x3_affine_relu_bwd_weight"}
    assert set(re.findall(r"\b(halo_upcat_\w+)\s*\(", code)) == {
        "halo_upcat_dwconv3x3_affine_relu_fwd", "halo_upcat_dwconv3x3_affine_relu_bwd_data", "halo_upcat_dwconv3x3_affine_relu_bwd_weight"}
    assert set(re.findall(r"\b(halo_multi_\w+)\s*\(", code)) == {
        "halo_multi_dwconv_max_plane", "halo_multi_dwconv3x3_affine_relu_fwd", "halo_multi_dwconv3x3_affine_relu_bwd_data"}
    assert re.findall(r"\b(halo_fan_\w+)\s*\(", code) == ["halo_fan_dwconv3x3_affine_relu_bwd_data"]


def test_argument_checks_refuse_before_any_launch():
    """every pointer is one HOST buffer: a check that went missing would end in a launch error or worse, never in these codes"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 14)
    base = ctypes.cast(buf, ctypes.c_void_p).value
    base += -base % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    plain, upcat = getattr(L, PLAIN), getattr(L, UPCAT)
    need = L.halo_dwconv_workspace_bytes(1, 2, 4, 4, 1)
    assert 0 < need <= 1 << 13

    def refused(rc, code, word, who):
        msg = L.halo_last_error().decode()
        assert rc == code and word in msg and msg.startswith(who + ":"), (rc, msg)

    shape = (1, 2, 4, 4, 1)
    for missing in range(7):                                                        # g, y, x, w, scale, g_x, g_w
        args = [p] * 7
        args[missing] = None
        refused(plain(*args, *shape, p, need, None), E_ARG, "null", PLAIN)
    for i in range(5):                                                              # B, C, H, W, d
        bad = list(shape)
        bad[i] = 0
        refused(plain(*[p] * 7, *bad, p, need, None), E_ARG, "empty shape or dilation < 1", PLAIN)
    refused(plain(*[p] * 7, 1, 2, 1 << 25, 4, 1, p, need, None), E_UNSUPPORTED, "planes", PLAIN)
    refused(plain(*[p] * 7, *shape, p, need - 1, None), E_WORKSPACE, "%d needed" % need, PLAIN)
    refused(plain(*[p] * 7, *shape, None, need, None), E_WORKSPACE, "workspace", PLAIN)
    refused(plain(*[p] * 7, *shape, odd, need, None), E_WORKSPACE, "8-byte aligned", PLAIN)
    refused(plain(None, *[p] * 6, 0, 2, 4, 4, 1, None, 0, None), E_ARG, "empty", PLAIN)   # the shape comes first, as in the parents

    front = (1, 1, 1, 2, 2, 4, 4)                                                   # B, Ca, Cs, h, w, H, W
    for missing in range(9):                                                        # g, y, a, s, w, scale, g_up, g_s, g_w
        args = [p] * 9
        args[missing] = None
        refused(upcat(*args, *front, p, need, None), E_ARG, "null", UPCAT)
    refused(upcat(*[p] * 9, 0, 1, 1, 2, 2, 4, 4, p, need, None), E_ARG, "empty", UPCAT)
    refused(upcat(*[p] * 9, 1, 0, 0, 2, 2, 4, 4, p, need, None), E_ARG, "empty", UPCAT)
    refused(upcat(*[p] * 9, 1, 1, 1, 0, 2, 4, 4, p, need, None), E_ARG, "empty", UPCAT)
    refused(upcat(*[p] * 9, 1, 1, 1, 5, 2, 4, 4, p, need, None), E_ARG, "an upsampling only", UPCAT)     # H < h
    refused(upcat(*[p] * 9, 1, 1, 1, 2, 5, 4, 4, p, need, None), E_ARG, "an upsampling only", UPCAT)     # W < w
    refused(upcat(*[p] * 9, *front, p, need - 1, None), E_WORKSPACE, "%d needed" % need, UPCAT)
    refused(upcat(*[p] * 9, *front, None, need, None), E_WORKSPACE, "workspace", UPCAT)
    refused(upcat(*[p] * 9, *front, odd, need, None), E_WORKSPACE, "8-byte aligned", UPCAT)


class _OnDevice:
    """describes a float32 ROCm tensor without one: the fallback reasons read attributes only"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)


def _block(C=5, d=1, bias=False):
    return nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=bias), R.FrozenBatchNorm2d(C)


def test_fallback_reasons_and_the_speed_rule(monkeypatch):
    from halo_amd import dwconv
    from halo_amd.dwconv import joint_fallback_reason as why, upcat_joint_fallback_reason as upwhy
    assert sorted(dwconv.JOINT_MIN_ELEMENTS) == ["column", "d1", "dilated", "upcat"]
    assert all(v is None or (isinstance(v, int) and v > 0) for v in dwconv.JOINT_MIN_ELEMENTS.values())
    conv, bn = _block()
    # the block's own reasons come first, on real CPU tensors and modules
    assert why(torch.zeros(2, 5, 8, 8), conv, bn) == "x is not on a ROCm device" == dwconv.fallback_reason(torch.zeros(2, 5, 8, 8), conv, bn)
    assert why(torch.zeros(2, 5, 8, 8), _block(bias=True)[0], bn) == "conv has a bias"
    assert why(torch.zeros(2, 5, 8, 8), conv, nn.BatchNorm2d(5)) == "BatchNorm with batch statistics"
    a, s = torch.zeros(2, 3, 4, 4), torch.zeros(2, 2, 8, 8)
    assert upwhy(a, s, conv, bn) == "a is not on a ROCm device" == dwconv.upcat_fallback_reason(a, s, conv, bn)
    assert upwhy(a, s, _block(bias=True)[0], bn) == "conv has a bias"
    assert upwhy(a, s, conv, nn.BatchNorm2d(5)) == "BatchNorm with batch statistics"
    # the speed rule, on descriptions of device tensors
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    # as shipped (profiles/r25_time_joint_depthwise.txt): the d = 1 route and the front from the smallest shape that won, the dilated
    # route, which lost everywhere, and the one-column route, which was not timed, not at all
    assert dwconv.JOINT_MIN_ELEMENTS == {"d1": 512 * 160 * 320, "dilated": None, "column": None, "upcat": 560 * 160 * 320}
    big = _block(C=512)
    assert why(_OnDevice(1, 512, 160, 320), *big) is None and why(_OnDevice(2, 512, 160, 320), *big) is None
    assert "fewer than JOINT_MIN_ELEMENTS['d1']" in why(_OnDevice(1, 512, 159, 320), *big)
    assert "'dilated' route is not served" in why(_OnDevice(2, 2048, 80, 160), *_block(C=2048, d=18))
    assert "'column' route is not served" in why(_OnDevice(2, 512, 160, 321), *big)
    front = _block(C=560)
    assert upwhy(_OnDevice(1, 512, 80, 160), _OnDevice(1, 48, 160, 320), *front) is None
    assert "fewer than JOINT_MIN_ELEMENTS['upcat']" in upwhy(_OnDevice(1, 512, 80, 160), _OnDevice(1, 48, 159, 320), *front)
    x, xc = _OnDevice(2, 5, 8, 8), _OnDevice(2, 5, 8, 9)
    ad, sd = _OnDevice(2, 3, 4, 4), _OnDevice(2, 2, 8, 8)
    monkeypatch.setattr(dwconv, "JOINT_MIN_ELEMENTS", {"d1": 1000, "dilated": None, "column": 0, "upcat": 641})
    assert dwconv.fallback_reason(x, conv, bn) is None and dwconv.upcat_fallback_reason(ad, sd, conv, bn) is None
    assert why(x, conv, bn) == "640 elements, fewer than JOINT_MIN_ELEMENTS['d1'] = 1000 (a speed rule: nothing smaller won)"
    assert why(_OnDevice(4, 5, 8, 8), conv, bn) is None                               # 1280 elements
    assert "'dilated' route is not served (a speed rule" in why(x, *_block(d=2))
    assert why(xc, conv, bn) is None and why(xc, *_block(d=2)) is None                # W % 4 != 0: the one-column route, whatever d
    assert "640 elements, fewer than JOINT_MIN_ELEMENTS['upcat'] = 641" in upwhy(ad, sd, conv, bn)
    assert upwhy(ad, _OnDevice(2, 2, 8, 9), conv, bn) is None                         # the front's one-column route
    monkeypatch.setattr(dwconv, "JOINT_MIN_ELEMENTS", {k: 0 for k in dwconv.JOINT_MIN_ELEMENTS})
    assert why(x, conv, bn) is None and why(x, *_block(d=2)) is None and upwhy(ad, sd, conv, bn) is None
    assert upwhy(ad, sd, *_block(d=2)) == dwconv.upcat_fallback_reason(ad, sd, *_block(d=2)) != None    # noqa: E711
    monkeypatch.setattr(dwconv, "JOINT_MIN_ELEMENTS", {k: None for k in dwconv.JOINT_MIN_ELEMENTS})
    assert "not served" in why(x, conv, bn) and "not served" in upwhy(ad, sd, conv, bn)


def _filled(C, d=1):
    conv, bn = _block(C, d)
    gen = torch.Generator().manual_seed(C + d)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=gen) + 0.5), bn.bias.copy_(torch.randn(C, generator=gen))
        bn.running_mean.copy_(torch.randn(C, generator=gen)), bn.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
    return conv, bn


def test_outside_the_envelope_the_torch_statements_run_and_the_default_is_off(monkeypatch):
    import inspect
    from halo_amd import dwconv
    assert inspect.signature(dwconv.depthwise_bn_relu).parameters["joint_backward"].default is False
    assert inspect.signature(dwconv.upsample_cat_depthwise_bn_relu).parameters["joint_backward"].default is False
    assert dwconv.joint_launches == {"plain": 0, "upcat": 0} or sorted(dwconv.joint_launches) == ["plain", "upcat"]
    assert sorted(dwconv.launches) == ["multi_bwd", "multi_fwd"]
    monkeypatch.setattr(dwconv, "JOINT_MIN_ELEMENTS", {k: 0 for k in dwconv.JOINT_MIN_ELEMENTS})
    before, before_multi = dict(dwconv.joint_launches), dict(dwconv.launches)
    gen = torch.Generator().manual_seed(3)
    conv, bn = _filled(5, 2)
    x = torch.randn(2, 5, 9, 10, generator=gen, requires_grad=True)
    g = torch.randn(2, 5, 9, 10, generator=gen)
    want = torch.autograd.grad(torch.relu(bn(conv(x))), [x, conv.weight], g)
    for kw in ({}, {"joint_backward": False}, {"joint_backward": True}):
        y = dwconv.depthwise_bn_relu(x, conv, bn, nn.ReLU(inplace=True), **kw)
        assert torch.equal(y, torch.relu(bn(conv(x))))
        got = torch.autograd.grad(y, [x, conv.weight], g)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    conv, bn = _filled(5, 1)
    a = torch.randn(2, 3, 4, 5, generator=gen, requires_grad=True)
    s = torch.randn(2, 2, 9, 10, generator=gen, requires_grad=True)
    g = torch.randn(2, 5, 9, 10, generator=gen)
    xs = torch.cat([nn.functional.interpolate(a, size=(9, 10), mode="bilinear", align_corners=True), s], 1)
    want = torch.autograd.grad(torch.relu(bn(conv(xs))), [a, s, conv.weight], g)
    for kw in ({}, {"joint_backward": True}):
        got = torch.autograd.grad(dwconv.upsample_cat_depthwise_bn_relu(a, s, conv, bn, **kw), [a, s, conv.weight], g)
        assert all(torch.equal(p, q) for p, q in zip(got, want))
    assert dwconv.joint_launches == before and dwconv.launches == before_multi


def test_hook_checks_its_class_and_sets_the_mark():
    import inspect
    import halo_amd
    from euclid_head_standin import Block, EuclidHead
    from halo_amd import hooks
    from halo_amd.core.models.classifier import v2_hyper_forward, v3plus_decoder, v3plus_forward, v3plus_hyper_forward
    use = hooks.use_joint_depthwise_backward

    class Plain(nn.Module):
        def forward(self, x):
            return x

    class V2(nn.Module):
        forward = v2_hyper_forward

    for bad in (Plain(), "Block", 3, None):
        with pytest.raises(TypeError, match="use_joint_depthwise_backward: expected a class"):
            use(bad)
    for bad in (Plain, V2, nn.Conv2d, EuclidHead, dict):                             # EuclidHead carries its own forward, not the package's
        with pytest.raises(TypeError, match="use_joint_depthwise_backward: .* is neither"):
            use(bad)
    MyBlock = type("MyBlock", (Block,), {})
    assert not hasattr(MyBlock, "_halo_joint_depthwise_backward")
    forward = MyBlock.forward
    assert use(MyBlock) is MyBlock and use(MyBlock) is MyBlock and MyBlock._halo_joint_depthwise_backward is True
    assert MyBlock.forward is forward and not hasattr(Block, "_halo_joint_depthwise_backward")      # the mark binds no forward
    assert hooks.use_fused_depthwise(MyBlock).forward is hooks.fused_dwsep_forward and MyBlock._halo_joint_depthwise_backward is True
    Other = use(hooks.use_fused_depthwise(type("Other", (Block,), {})))                # the other order
    assert Other.forward is hooks.fused_dwsep_forward and Other._halo_joint_depthwise_backward is True
    for f in (v3plus_hyper_forward, hooks.fused_v3plus_hyper_forward, v3plus_forward):
        Head = type("Head", (nn.Module,), {"forward": f})
        assert use(Head) is Head and use(Head) is Head and Head._halo_joint_depthwise_backward is True and Head.forward is f
    Bound = hooks.use_v3plus_forward(type("Bound", (EuclidHead,), {}))
    assert use(Bound) is Bound and not hasattr(EuclidHead, "_halo_joint_depthwise_backward")
    assert "use_joint_depthwise_backward" not in inspect.getsource(halo_amd.install)
    assert "_halo_joint_depthwise_backward" in inspect.getsource(hooks.fused_dwsep_forward)
    assert "_halo_joint_depthwise_backward" in inspect.getsource(v3plus_decoder)
    # parameters, module names and state_dict() are untouched, and CPU tensors run as before
    torch.manual_seed(2)
    with torch.no_grad():
        m, k = MyBlock(4, 6, 2), Block(4, 6, 2)
    k.load_state_dict(m.state_dict())
    assert list(m.state_dict()) == list(k.state_dict())
    x = torch.randn(1, 4, 6, 7)
    assert torch.equal(m(x), k(x))
