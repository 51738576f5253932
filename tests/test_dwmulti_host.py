"""CPU checks of the multi-dilation depthwise passes (halo_multi_dwconv3x3_* of halo_dwconv.hip, halo_amd.dwconv.multi_depthwise_bn_relu,
halo_amd.hooks.use_fused_aspp_depthwise): the entries are declared, listed and exported under ABI 13, every argument check refuses
before a launch, the envelope query and decisions, the composition that CPU tensors run, the hook's class checks, and the cases of
tests/dwmulti_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import dwconv_ref as R
import dwmulti_cases as K

SYMBOLS = ("halo_multi_dwconv_max_plane", "halo_multi_dwconv3x3_affine_relu_fwd", "halo_multi_dwconv3x3_affine_relu_bwd_data")
E_ARG, E_UNSUPPORTED = -1, -2


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(halo_multi_\w+)\s*\(", code)) == set(SYMBOLS)
    assert "#define HALO_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
    assert _lib.lib().halo_version() == 13
    assert [len(_lib.SIGNATURES[s][1]) for s in SYMBOLS] == [0, 12, 12]


def test_max_plane_holds_the_heads_planes_and_fits_the_lds_twice():
    from halo_amd import _lib, dwconv
    limit = _lib.lib().halo_multi_dwconv_max_plane()
    assert 14400 <= limit <= 160 * 1024 // 8 and dwconv.multi_max_plane() == limit
    inside, outside = K.edge_shapes(limit)
    assert inside[2] * inside[3] == limit and outside[2] * outside[3] > limit and inside[3] == outside[3] and outside[2] == inside[2] + 1


def test_argument_checks_refuse_before_any_launch():
    """every pointer is one HOST buffer: a check that went missing would end in a launch error or worse, never in these codes"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = L.halo_multi_dwconv3x3_affine_relu_fwd, L.halo_multi_dwconv3x3_affine_relu_bwd_data
    limit = L.halo_multi_dwconv_max_plane()
    d3, d5 = (ctypes.c_int64 * 3)(6, 12, 18), (ctypes.c_int64 * 5)(1, 2, 3, 4, 5)
    g3 = (ctypes.c_void_p * 3)(p.value, None, p.value)
    none3 = (ctypes.c_void_p * 3)(None, None, None)

    def refused(rc, code, word):
        msg = L.halo_last_error().decode()
        assert rc == code and word in msg and "halo_multi_dwconv3x3_affine_relu" in msg, (rc, msg)

    refused(fwd(p, p, p, p, p, 1, 2, 4, 4, 1, d3, None), E_ARG, "dilations")                     # n = 1
    refused(fwd(p, p, p, p, p, 1, 2, 4, 4, 5, d5, None), E_ARG, "dilations")                     # n = 5
    refused(fwd(p, p, p, p, p, 1, 2, 4, 4, 3, None, None), E_ARG, "null")                        # no d
    for missing in range(5):
        args = [p] * 5
        args[missing] = None
        refused(fwd(*args, 1, 2, 4, 4, 3, d3, None), E_ARG, "null")
    refused(fwd(p, p, p, p, p, 0, 2, 4, 4, 3, d3, None), E_ARG, "empty")
    refused(fwd(p, p, p, p, p, 1, 2, 4, 4, 3, (ctypes.c_int64 * 3)(6, 0, 18), None), E_ARG, "dilation")
    refused(fwd(p, p, p, p, p, 1, 2, 1 << 25, 4, 3, d3, None), E_UNSUPPORTED, "planes")
    refused(fwd(p, p, p, p, p, 1, 2, limit + 1, 1, 3, d3, None), E_UNSUPPORTED, "plane of %d x 1" % (limit + 1))
    refused(fwd(p, p, p, p, p, 1, 2, 1, limit + 1, 3, d3, None), E_UNSUPPORTED, str(limit))
    refused(bwd(g3, p, p, p, p, 1, 2, 4, 4, 1, d3, None), E_ARG, "dilations")
    refused(bwd(g3, p, p, p, p, 1, 2, 4, 4, 5, d5, None), E_ARG, "dilations")
    refused(bwd(g3, p, p, p, p, 1, 2, 4, 4, 3, None, None), E_ARG, "null")
    refused(bwd(None, p, p, p, p, 1, 2, 4, 4, 3, d3, None), E_ARG, "null")
    for missing in range(1, 5):
        args = [g3, p, p, p, p]
        args[missing] = None
        refused(bwd(*args, 1, 2, 4, 4, 3, d3, None), E_ARG, "null")
    refused(bwd(none3, p, p, p, p, 1, 2, 4, 4, 3, d3, None), E_ARG, "every gradient")
    refused(bwd(g3, p, p, p, p, 1, 0, 4, 4, 3, d3, None), E_ARG, "empty")
    refused(bwd(g3, p, p, p, p, 1, 2, limit + 1, 1, 3, d3, None), E_UNSUPPORTED, "plane of %d x 1" % (limit + 1))


class _OnDevice:
    """describes a float32 ROCm tensor without one: the fallback reasons read attributes only"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)


def _block(C=5, d=1, bias=False):
    return nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=bias), R.FrozenBatchNorm2d(C)


def test_every_fallback_reason(monkeypatch):
    from halo_amd import dwconv
    from halo_amd.dwconv import multi_fallback_reason as why, multi_max_plane
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    x = _OnDevice(2, 5, 8, 10)
    three = [_block(d=6), _block(d=12) + (nn.ReLU(),), _block(d=18)]
    # the speed rule: the smallest input timed is served, anything smaller is not; off for the rest of the test
    assert dwconv.MULTI_MIN_ELEMENTS in (1 * 2048 * 80 * 160, 2 * 2048 * 80 * 160)
    assert "800 elements, fewer than MULTI_MIN_ELEMENTS = %d" % dwconv.MULTI_MIN_ELEMENTS in why(x, three)
    big = [_block(C=2048, d=6), _block(C=2048, d=12)]
    assert why(_OnDevice(2, 2048, 80, 160), big) is None and "speed rule" in why(_OnDevice(1, 2048, 80, 159), big)
    monkeypatch.setattr(dwconv, "MULTI_MIN_ELEMENTS", 0)
    assert why(x, three) is None
    assert why(x, three[:2]) is None and why(x, three + [_block(d=1)]) is None
    assert "1 blocks, 2 to 4" in why(x, three[:1]) and "5 blocks, 2 to 4" in why(x, three + three[:2]) and "0 blocks" in why(x, [])
    assert "(conv, bn)" in why(x, [three[0], three[1][:1]])
    assert "channel counts differ" in why(x, [three[0], _block(C=6)])
    assert why(x, [three[0], (nn.ReLU(), three[0][1])]).startswith("the blocks' channel counts differ")      # no conv at all
    assert why(x, [three[0], _block(bias=True)]) == "block 1: conv has a bias"
    assert why(x, [(three[0][0], nn.BatchNorm2d(5)), three[1]]) == "block 0: BatchNorm with batch statistics"
    assert why(_OnDevice(2, 6, 8, 10), three).startswith("block 0: x has 6 channels")
    assert why(_OnDevice(5, 8, 10), three) == "block 0: x is not a (B, C, H, W) tensor"
    limit = multi_max_plane()
    inside, outside = K.edge_shapes(limit)
    two = [_block(C=2, d=6), _block(C=2, d=12)]
    assert why(_OnDevice(*inside), two) is None
    reason = why(_OnDevice(*outside), two)
    assert "plane of %d x %d = %d elements" % (outside[2], outside[3], outside[2] * outside[3]) in reason and str(limit) in reason
    monkeypatch.undo()
    assert why(torch.zeros(2, 5, 8, 10), three) == "block 0: x is not on a ROCm device"


@pytest.mark.parametrize("kind", ["frozen", "train_bn"])
def test_cpu_tensors_run_the_composition(kind):
    from halo_amd import dwconv
    torch.manual_seed(5)
    blocks = []
    for d in (1, 2, 3):
        conv = nn.Conv2d(5, 5, 3, 1, d, d, groups=5, bias=False)
        if kind == "train_bn":
            bn = nn.BatchNorm2d(5)
        else:
            bn = R.FrozenBatchNorm2d(5)
            bn.weight.copy_(torch.rand(5) + 0.5), bn.bias.copy_(torch.randn(5)), bn.running_mean.copy_(torch.randn(5)), bn.running_var.copy_(torch.rand(5) + 0.5)
        blocks.append((conv, bn, nn.ReLU(inplace=True)))
    x = torch.randn(2, 5, 9, 10, requires_grad=True)
    gs = [torch.randn(2, 5, 9, 10) for _ in blocks]
    before = dict(dwconv.launches)
    ys = dwconv.multi_depthwise_bn_relu(x, blocks)
    assert isinstance(ys, tuple) and len(ys) == 3 and dwconv.launches == before and sorted(before) == ["multi_bwd", "multi_fwd"]
    wanted = [x] + [b[0].weight for b in blocks]
    got = torch.autograd.grad(ys, wanted, gs)
    if kind == "train_bn":
        blocks = [(c, nn.BatchNorm2d(5), a) for c, _, a in blocks]                                # fresh running statistics
    want = [a(bn(conv(x))) for conv, bn, a in blocks]
    assert all(torch.equal(a, b) for a, b in zip(ys, want))
    # g_x is the contract's ((gx_0 + gx_1) + gx_2) on the fallback too: one backward per block, added in list order
    parts = [torch.autograd.grad(y, [x, b[0].weight], g) for y, b, g in zip(want, blocks, gs)]
    assert torch.equal(got[0], (parts[0][0] + parts[1][0]) + parts[2][0])
    assert all(torch.equal(a, p[1]) for a, p in zip(got[1:], parts))


def test_hook_marks_only_classes_with_a_v3plus_forward_and_unmarked_classes_keep_the_statement():
    from halo_amd.core.models.classifier import aspp_pyramid, v2_hyper_forward, v3plus_forward, v3plus_hyper_forward
    from halo_amd.hooks import fused_v3plus_hyper_forward, use_fused_aspp_depthwise

    class Plain(nn.Module):
        def forward(self, x):
            return x

    class V2(nn.Module):
        forward = v2_hyper_forward

    heads = [type("Head%d" % i, (nn.Module,), {"forward": f}) for i, f in enumerate((v3plus_hyper_forward, fused_v3plus_hyper_forward, v3plus_forward))]
    for bad in (Plain, V2, nn.Conv2d, Plain(), "Head"):
        with pytest.raises(TypeError, match="use_fused_aspp_depthwise: "):
            use_fused_aspp_depthwise(bad)
    with pytest.raises(TypeError, match="V2 does not carry one of halo_amd's v3\\+ forwards; bind one first with"):
        use_fused_aspp_depthwise(V2)
    for Head, f in zip(heads, (v3plus_hyper_forward, fused_v3plus_hyper_forward, v3plus_forward)):
        assert not hasattr(Head, "_halo_fused_aspp_depthwise")
        assert use_fused_aspp_depthwise(Head) is Head and use_fused_aspp_depthwise(Head) is Head and Head._halo_fused_aspp_depthwise is True
        assert Head.forward is f
    Child = type("Child", (heads[0],), {})
    assert use_fused_aspp_depthwise(Child) is Child
    import halo_amd
    import inspect
    assert "use_fused_aspp_depthwise" not in inspect.getsource(halo_amd.install)

    # the pyramid helper: an unmarked class calls every branch once, in order; a marked class whose branches are no blocks under
    # use_fused_depthwise does the same
    calls = []

    class Branch(nn.Module):
        def __init__(self, k):
            super().__init__()
            self.k = k

        def forward(self, x):
            calls.append(self.k)
            return x + self.k

    class Unmarked(nn.Module):
        forward = v3plus_forward

        def __init__(self):
            super().__init__()
            self.parallel_branches = nn.ModuleList([Branch(k) for k in range(4)])

    x = torch.zeros(1, 2, 3, 3)
    for cls in (Unmarked, use_fused_aspp_depthwise(type("MarkedPlain", (Unmarked,), {}))):
        calls.clear()
        out = aspp_pyramid(cls(), x)
        assert calls == [0, 1, 2, 3] and [float(o[0, 0, 0, 0]) for o in out] == [0.0, 1.0, 2.0, 3.0]
    assert not hasattr(Unmarked, "_halo_fused_aspp_depthwise")
    for f in (v3plus_hyper_forward, fused_v3plus_hyper_forward, v3plus_forward):
        src = inspect.getsource(f)
        assert "aspp_pyramid(self, top)" in src and "for branch in self.parallel_branches" not in src


def test_marked_head_on_cpu_tensors_is_the_unmarked_head():
    """blocks under use_fused_depthwise on a marked head, CPU tensors: multi_fallback_reason is not None, every branch is called"""
    from euclid_head_standin import Block, EuclidHead
    from halo_amd import dwconv, hooks
    Fused = hooks.use_fused_depthwise(type("Fused", (Block,), {}))
    Base = hooks.use_v3plus_forward(type("Base", (EuclidHead,), {}))
    Marked = hooks.use_fused_aspp_depthwise(hooks.use_v3plus_forward(type("Marked", (EuclidHead,), {})))
    torch.manual_seed(3)
    with torch.no_grad():
        base, marked = Base(Fused, p=0.5).eval(), Marked(Fused, p=0.5).eval()
    marked.load_state_dict(base.state_dict())
    gen = torch.Generator().manual_seed(4)
    feats = {"out": torch.randn(2, 24, 9, 13, generator=gen), "low": torch.randn(2, 12, 33, 49, generator=gen)}
    before = dict(dwconv.launches)
    with torch.no_grad():
        a, b = base(feats), marked(feats)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and dwconv.launches == before


def test_cases_are_the_recipe_per_dilation():
    assert list(K.CASES)[0] == K.OFFSET[0] == K.FLOAT64[0] and K.FLOAT64[1] == list(K.CASES)[2]
    for name, ((B, C, H, W, dil), _) in K.CASES.items():
        cs = K.case(name)
        assert len(cs) == len(dil) and 2 <= len(dil) <= 4 and [c["d"] for c in cs] == list(dil)
        assert B * C * H * W <= 30000
        for c in cs:
            assert c["x"] is cs[0]["x"] and c["x"].shape == (B, C, H, W) and c["g"].shape == (B, C, H, W)
            assert c["weight"][0] == np.float32(-0.75) and c["bias"][C - 1] == np.float32(-1e4)
            assert (c["x"] * 4 == np.round(c["x"] * 4)).all() and (c["g"] * 4 == np.round(c["g"] * 4)).all()
        assert not np.array_equal(cs[0]["w"], cs[1]["w"]) and not np.array_equal(cs[0]["g"], cs[1]["g"])
