"""CPU checks of the fused frozen norm + residual add + ReLU (halo_norm.hip, halo_amd.norm, halo_amd.hooks.use_fused_frozen_norm,
fuse_norm_relu_pairs): the entry points are declared and refuse bad arguments before any launch, every envelope decision, the
fallback to the stock statements, the scale / shift cache, and both hooks on stand-in blocks, stems and heads."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import norm_ref as N
from dwconv_ref import FrozenBatchNorm2d

SYMBOLS = ("halo_affine_relu_fwd", "halo_affine_relu_bwd")
E_ARG = -1                # HALO_E_ARG of include/halo_hip.h


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    assert set(re.findall(r"\b(halo_affine_relu\w+)\s*\(", text)) == set(SYMBOLS)
    assert "halo_norm.hip" in _build.SOURCES
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s


def test_argument_checks_are_host_code():
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = L.halo_affine_relu_fwd, L.halo_affine_relu_bwd
    assert fwd(a, a, None, None, None, None, a, 1, 2, 16, None) == E_ARG             # no shift
    assert fwd(a, a, a, None, None, None, None, 1, 2, 16, None) == E_ARG            # no y
    assert fwd(a, a, a, a, a, None, a, 1, 2, 16, None) == E_ARG                     # r_scale without r_shift
    assert fwd(a, a, a, a, None, a, a, 1, 2, 16, None) == E_ARG                     # r_shift without r_scale
    assert fwd(a, a, a, None, a, a, a, 1, 2, 16, None) == E_ARG                     # r_scale without r
    assert fwd(a, a, a, None, None, None, a, 0, 2, 16, None) == E_ARG               # empty shape
    assert fwd(a, a, a, None, None, None, a, 1, 2, 0, None) == E_ARG
    assert fwd(a, a, a, None, None, None, a, 1, 2, 1 << 31, None) == _lib.E_UNSUPPORTED   # plane offsets are 32-bit inside a plane
    assert fwd(a, a, a, None, None, None, a, 1 << 20, 1 << 20, 4096, None) == _lib.E_UNSUPPORTED   # more workgroups than a grid holds
    assert bwd(a, a, a, None, None, None, 1, 2, 16, None) == E_ARG                  # neither gradient asked for
    assert bwd(a, None, a, None, a, None, 1, 2, 16, None) == E_ARG                  # no y
    assert bwd(a, a, None, None, a, None, 1, 2, 16, None) == E_ARG                  # g_x without scale
    assert bwd(a, a, a, None, a, a, 1, 0, 16, None) == E_ARG
    assert "halo_affine_relu" in L.halo_last_error().decode()


class _OnDevice:
    """describes a contiguous float32 ROCm tensor without one: fallback_reason reads attributes only"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, *shape, contiguous=True, dtype=torch.float32, device="cpu"):
        self.shape, self._c, self.dtype, self.device = torch.Size(shape), contiguous, dtype, torch.device(device)

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def is_contiguous(self):
        return self._c


def test_envelope_decisions(monkeypatch):
    from halo_amd.norm import fallback_reason
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    x, r = _OnDevice(2, 8, 5, 7), _OnDevice(2, 8, 5, 7)
    bn, rbn = FrozenBatchNorm2d(8), FrozenBatchNorm2d(8)
    assert fallback_reason(x, bn) is None and fallback_reason(x, bn, r) is None and fallback_reason(x, bn, r, rbn) is None
    assert "(B, C, H, W)" in fallback_reason(_OnDevice(8, 5, 7), bn)
    assert "(B, C, H, W)" in fallback_reason([1.0], bn)
    assert "float32" in fallback_reason(_OnDevice(2, 8, 5, 7, dtype=torch.float16), bn)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert "autocast" in fallback_reason(x, bn)
    assert "device" in fallback_reason(torch.zeros(2, 8, 5, 7), bn)                               # CPU tensors: the torch statements
    assert "empty" in fallback_reason(_OnDevice(0, 8, 5, 7), bn)
    assert "contiguous" in fallback_reason(_OnDevice(2, 8, 5, 7, contiguous=False), bn)           # channels-last, slices
    assert "plane" in fallback_reason(_OnDevice(1, 8, 1 << 16, 1 << 15), bn)
    for other in (nn.BatchNorm2d(8).eval(), nn.BatchNorm2d(8), nn.GroupNorm(2, 8), nn.Identity()):
        assert "FrozenBatchNorm2d" in fallback_reason(x, other)
        assert "residual_bn is not" in fallback_reason(x, bn, r, other)
    assert "channels" in fallback_reason(x, FrozenBatchNorm2d(6))
    assert "channels" in fallback_reason(x, bn, r, FrozenBatchNorm2d(6))
    assert "float32 on" in fallback_reason(x, FrozenBatchNorm2d(8).double())
    assert "float32 on" in fallback_reason(_OnDevice(2, 8, 5, 7, device="meta"), bn)              # the norm lives elsewhere
    assert "without a residual" in fallback_reason(x, bn, None, rbn)
    assert "shape" in fallback_reason(x, bn, _OnDevice(2, 8, 5, 6))
    assert "shape" in fallback_reason(x, bn, 1.0)
    assert "residual is not" in fallback_reason(x, bn, _OnDevice(2, 8, 5, 7, dtype=torch.float64))
    assert "residual is not" in fallback_reason(x, bn, _OnDevice(2, 8, 5, 7, device="meta"))
    assert "residual is not contiguous" in fallback_reason(x, bn, _OnDevice(2, 8, 5, 7, contiguous=False))


def test_small_tensors_that_need_a_gradient_run_the_stock_statements(monkeypatch):
    from halo_amd import norm
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))

    def operand(*shape, grad=True):
        t = _OnDevice(*shape)
        t.requires_grad = grad
        return t
    bn, rbn = FrozenBatchNorm2d(512), FrozenBatchNorm2d(512)
    small, large = (2, 512, 80, 160), (4, 512, 80, 160)
    assert "autograd" in norm.fallback_reason(operand(*small), bn)                                       # measured slower: DESIGN section 15
    assert "autograd" in norm.fallback_reason(operand(*small, grad=False), bn, operand(*small))
    assert norm.fallback_reason(operand(*small), bn, operand(*small), rbn) is None                       # with a residual_bn it wins there
    assert "autograd" in norm.fallback_reason(operand(2, 512, 80, 159), bn, operand(2, 512, 80, 159), rbn)
    assert norm.fallback_reason(operand(*large), bn) is None and norm.fallback_reason(operand(*large), bn, operand(*large)) is None
    assert norm.fallback_reason(operand(*small, grad=False), bn, operand(*small, grad=False)) is None    # no gradient: every size
    with torch.no_grad():
        assert norm.fallback_reason(operand(*small), bn) is None
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0})                        # a speed rule only
    assert norm.fallback_reason(operand(2, 512, 5, 7), bn) is None


@pytest.mark.parametrize("variant", ["none", "plain", "affine", "eval_bn"])
def test_cpu_tensors_run_the_stock_statements(variant):
    from halo_amd.norm import norm_relu, torch_statement
    torch.manual_seed(3)
    bn = N.randomize_norms(FrozenBatchNorm2d(6), 1) if variant != "eval_bn" else nn.BatchNorm2d(6).eval()
    rbn = N.randomize_norms(FrozenBatchNorm2d(6), 2) if variant == "affine" else None
    x0, r0, g = torch.randn(2, 6, 7, 9), torch.randn(2, 6, 7, 9), torch.randn(2, 6, 7, 9)
    results = []
    for fn in (norm_relu, torch_statement, N.stock_chain):
        x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
        y = fn(x, bn) if variant in ("none", "eval_bn") else fn(x, bn, r, rbn)
        results.append((y.detach(),) + torch.autograd.grad(y, [x] if variant in ("none", "eval_bn") else [x, r], g))
        assert torch.equal(x.detach(), x0)                                                       # x itself is never written
    for other in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(results[0], other))


def test_scale_shift_cache_follows_the_buffers():
    from halo_amd.dwconv import scale_shift
    from halo_amd.norm import cached_scale_shift, forget

    def fresh(bn):
        pair, want = cached_scale_shift(bn), scale_shift(bn)
        assert torch.equal(pair[0], want[0]) and torch.equal(pair[1], want[1])
        return pair
    bn = N.randomize_norms(FrozenBatchNorm2d(5), 4)
    a = fresh(bn)
    b = cached_scale_shift(bn)
    assert a[0] is b[0] and a[1] is b[1]                                                         # reused: the same tensor objects
    other = N.randomize_norms(FrozenBatchNorm2d(5), 5)
    v = bn.running_var._version
    bn.load_state_dict(other.state_dict())
    assert bn.running_var._version > v                                                           # what the key relies on
    c = fresh(bn)
    assert c[0] is not a[0] and not torch.equal(c[0], a[0])
    with torch.no_grad():
        bn.running_var.mul_(4.0)
    d = fresh(bn)
    assert torch.equal(d[0], c[0] * 0.5) and d[0] is not c[0]
    bn.running_mean = bn.running_mean + 1.0                                                      # a new tensor object, version 0
    e = fresh(bn)
    assert e[1] is not d[1] and not torch.equal(e[1], d[1]) and cached_scale_shift(bn)[1] is e[1]
    moved = bn.to(torch.float64).to(torch.float32)                                               # .to() replaces every buffer
    assert moved is bn and fresh(bn)[0] is not e[0]
    twin = copy.deepcopy(bn)
    with torch.no_grad():
        twin.weight.neg_()
    assert torch.equal(fresh(twin)[0], -fresh(bn)[0])                                            # per instance
    f = cached_scale_shift(bn)
    forget(bn)
    assert cached_scale_shift(bn)[0] is not f[0]


def test_block_hook_binds_an_opt_in_forward_and_keeps_the_previous_one():
    import halo_amd
    from halo_amd.hooks import fused_residual_forward, use_fused_frozen_norm
    for Block in (N.Bottleneck, N.BasicBlock):
        Sub = type("Sub", (Block,), {})
        assert use_fused_frozen_norm(Sub) is Sub
        assert Sub.forward is fused_residual_forward and Sub._unfused_forward is Block.__dict__["forward"]
        assert use_fused_frozen_norm(Sub)._unfused_forward is Block.__dict__["forward"]          # idempotent
        assert Block.forward is not fused_residual_forward
    Named = type("Bottleneck", (nn.Module,), {"forward": lambda self, x: x})                     # the reference's name is enough
    assert use_fused_frozen_norm(Named).forward is fused_residual_forward
    for bad in (nn.Conv2d, nn.Sequential, N.Head, type("NoModule", (), {}), N.BasicBlock(4, 4)):
        with pytest.raises(TypeError):
            use_fused_frozen_norm(bad)
    init = open(os.path.join(os.path.dirname(halo_amd.__file__), "__init__.py")).read() + open(
        os.path.join(os.path.dirname(halo_amd.__file__), "_install.py")).read()
    for name in ("use_fused_frozen_norm", "fuse_norm_relu_pairs", "fused_residual_forward"):
        assert name not in init                                                                  # install() binds neither hook


def _blocks():
    odd = nn.Sequential(nn.AvgPool2d(1), nn.Conv2d(6, 12, 1, bias=False), FrozenBatchNorm2d(12))
    return {
        "bottleneck_seq_downsample": lambda: N.Bottleneck(6, 4, 12, stride=2, downsample=N.down(6, 12, 2)),
        "bottleneck_other_downsample": lambda: N.Bottleneck(6, 4, 12, downsample=copy.deepcopy(odd)),
        "bottleneck_no_downsample": lambda: N.Bottleneck(12, 4, 12, dilation=2),
        "bottleneck_batchnorm": lambda: N.Bottleneck(6, 4, 12, downsample=N.down(6, 12, norm=nn.BatchNorm2d), norm=nn.BatchNorm2d),
        "bottleneck_gelu": lambda: N.Bottleneck(12, 4, 12, act=nn.GELU()),
        "basic_seq_downsample": lambda: N.BasicBlock(6, 12, 2, downsample=N.down(6, 12, 2)),
        "basic_no_downsample": lambda: N.BasicBlock(6, 6),
    }


@pytest.mark.parametrize("kind", sorted(_blocks()))
def test_hooked_block_equals_the_unhooked_block_on_cpu(kind):
    torch.manual_seed(5)
    plain = N.randomize_norms(_blocks()[kind](), 6)
    hooked, pairs = N.hooked_copy(plain)
    assert pairs == 0 and type(hooked) is not type(plain)               # a block's own (norm, ReLU) is no container's pair
    x = torch.randn(2, plain.conv1.in_channels, 9, 11)
    g_of = lambda outs: [torch.ones_like(o) * 0.5 for o in outs]
    (y1,), g1 = N.run_with_grads(plain, x, g_of)
    (y2,), g2 = N.run_with_grads(hooked, x, g_of)
    assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    if kind == "bottleneck_batchnorm":                                  # batch statistics: the running averages moved alike
        assert torch.equal(plain.bn3.running_mean, hooked.bn3.running_mean)
        assert torch.equal(plain.downsample[1].running_var, hooked.downsample[1].running_var)


def test_pair_fusion_counts_names_and_undo():
    from halo_amd.hooks import fuse_norm_relu_pairs, unfuse_norm_relu_pairs
    torch.manual_seed(7)
    net = N.randomize_norms(N.Net(), 8)
    plain = copy.deepcopy(net)
    keys, names = list(net.state_dict().keys()), [n for n, _ in net.named_modules()]
    assert fuse_norm_relu_pairs(net.feature_extractor) == 1            # the stem inside the IntermediateLayerGetter, no block
    assert fuse_norm_relu_pairs(net.classifier) == 4                   # parallel_branches[0], global_branch, bottleneck, shortcut
    assert fuse_norm_relu_pairs(net) == 0                              # a second call finds nothing
    for block in list(net.feature_extractor["layer1"]) + list(net.feature_extractor["layer2"]):
        assert all("forward" not in m.__dict__ for m in block.modules())
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_modules()] == names
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), plain.state_dict().values()))
    x = torch.randn(2, 3, 33, 47)
    g_of = lambda outs: [torch.full_like(o, 0.25) for o in outs]
    o1, g1 = N.run_with_grads(plain, x, g_of)
    o2, g2 = N.run_with_grads(net, x, g_of)
    assert all(torch.equal(a, b) for a, b in zip(o1 + g1, o2 + g2))
    other = N.randomize_norms(N.Net(), 9)                              # a checkpoint loaded afterwards takes effect
    net.load_state_dict(other.state_dict())
    o3, _ = N.run_with_grads(other, x, g_of)
    o4, _ = N.run_with_grads(net, x, g_of)
    assert all(torch.equal(a, b) for a, b in zip(o3, o4)) and not torch.equal(o4[0], o2[0])
    twin = copy.deepcopy(net)                                          # a copy's pairs refer to the copy's norms
    assert twin.classifier.shortcut[1].forward.norm is twin.classifier.shortcut[1]
    assert unfuse_norm_relu_pairs(net) == 5 and unfuse_norm_relu_pairs(net) == 0
    assert all("forward" not in m.__dict__ for m in net.modules())
    o5, _ = N.run_with_grads(net, x, g_of)
    assert all(torch.equal(a, b) for a, b in zip(o3, o5))


def test_pair_fusion_leaves_shared_and_returned_modules_alone():
    from halo_amd.hooks import fuse_norm_relu_pairs
    act = nn.ReLU(inplace=True)
    shared = nn.Sequential(nn.Conv2d(3, 4, 1), FrozenBatchNorm2d(4), act, nn.Conv2d(4, 4, 1), act)       # one ReLU object, two places
    assert fuse_norm_relu_pairs(shared) == 0 and "forward" not in act.__dict__
    getter = N.IntermediateLayerGetter({"conv1": nn.Conv2d(3, 4, 1), "bn1": FrozenBatchNorm2d(4), "relu": nn.ReLU()}, {"bn1": "pre"})
    assert fuse_norm_relu_pairs(getter) == 0                                                              # bn1's own output is returned
    plain = nn.ModuleDict({"bn1": FrozenBatchNorm2d(4), "relu": nn.ReLU()})                               # no container that calls in order
    assert fuse_norm_relu_pairs(plain) == 0
    others = nn.Sequential(nn.BatchNorm2d(4).eval(), nn.ReLU(), FrozenBatchNorm2d(4), nn.ReLU6(), FrozenBatchNorm2d(4), nn.Identity(), nn.ReLU())
    assert fuse_norm_relu_pairs(others) == 0
