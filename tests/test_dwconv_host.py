"""CPU checks of the fused depthwise conv + frozen norm + ReLU (halo_dwconv.hip, halo_amd.dwconv, halo_amd.hooks.use_fused_depthwise):
the entry points are declared, listed and exported, the argument checks refuse before any launch, the envelope and the fallback,
the hook binding, and the fixture: the numpy evaluator of tests/dwconv_ref.py agrees with the reference modules' stored float64
results, and the reference's own float32 chain stays inside the conditions the device is held to in tests/test_gpu_dwconv.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import dwconv_ref as R

SYMBOLS = ("halo_dwconv_workspace_bytes", "halo_dwconv3x3_affine_relu_fwd", "halo_dwconv3x3_affine_relu_bwd_data",
           "halo_dwconv3x3_affine_relu_bwd_weight")


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    assert set(re.findall(r"\b(halo_dwconv\w+)\s*\(", text)) == set(SYMBOLS)
    assert "#define HALO_ABI_VERSION %d" % _lib.ABI_VERSION in text
    assert "halo_dwconv.hip" in _build.SOURCES
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
    assert _lib.ABI_VERSION >= 10 and _lib.lib().halo_version() == _lib.ABI_VERSION


def test_workspace_query_and_argument_checks_are_host_code():
    from halo_amd import _lib
    L = _lib.lib()
    q = L.halo_dwconv_workspace_bytes
    assert q(2, 512, 160, 320, 1) >= 2 * 512 * 9 * 8 and q(2, 512, 160, 320, 1) % 8 == 0
    assert q(2, 8, 11, 13, 2) >= 2 * 8 * 9 * 8
    assert q(0, 8, 4, 4, 1) == 0 and q(2, 8, 4, 4, 0) == 0 and q(2, 8, 1 << 25, 4, 1) == 0
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    assert L.halo_dwconv3x3_affine_relu_fwd(a, a, a, None, a, 1, 2, 4, 4, 1, None) != 0                  # no shift
    assert L.halo_dwconv3x3_affine_relu_fwd(a, a, a, a, a, 1, 2, 4, 4, 0, None) != 0                     # d < 1
    assert L.halo_dwconv3x3_affine_relu_fwd(a, a, a, a, a, 1, 2, 1 << 25, 4, 1, None) == _lib.E_UNSUPPORTED
    assert L.halo_dwconv3x3_affine_relu_bwd_data(a, None, a, a, a, 1, 2, 4, 4, 1, None) != 0             # no y
    assert L.halo_dwconv3x3_affine_relu_bwd_data(a, a, a, a, a, 0, 2, 4, 4, 1, None) != 0                # empty shape
    n = q(1, 2, 4, 4, 1)
    assert L.halo_dwconv3x3_affine_relu_bwd_weight(a, a, a, a, a, 1, 2, 4, 4, 1, a, n - 1, None) != 0    # short workspace
    assert L.halo_dwconv3x3_affine_relu_bwd_weight(a, a, a, a, a, 1, 2, 4, 4, 1, None, n, None) != 0     # no workspace
    assert "halo_dwconv" in L.halo_last_error().decode()


def _pair(C=8, d=2):
    return nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False), R.FrozenBatchNorm2d(C)


class _OnDevice:
    """describes a float32 ROCm tensor without one: fallback_reason reads attributes only"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)


def test_envelope_decisions(monkeypatch):
    from halo_amd import dwconv
    from halo_amd.dwconv import fallback_reason
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    x = _OnDevice(2, 8, 5, 7)
    conv, bn = _pair()
    assert fallback_reason(x, conv, bn) is None                                              # in the envelope
    ev = nn.BatchNorm2d(8).eval()
    with torch.no_grad():
        assert fallback_reason(x, conv, ev) is None                                          # kind (b), no gradient asked
    assert "gradient" in fallback_reason(x, conv, ev)
    for p in ev.parameters():
        p.requires_grad_(False)
    assert fallback_reason(x, conv, ev) is None
    assert fallback_reason(x, conv, nn.BatchNorm2d(8, affine=False).eval()) is None
    assert fallback_reason(x, conv, nn.SyncBatchNorm(8, affine=False).eval()) is None
    assert "batch statistics" in fallback_reason(x, conv, nn.BatchNorm2d(8))                 # training mode
    assert "batch statistics" in fallback_reason(x, conv, nn.BatchNorm2d(8, track_running_stats=False).eval())
    assert "neither" in fallback_reason(x, conv, nn.GroupNorm(2, 8))
    assert "neither" in fallback_reason(x, conv, nn.Identity())
    assert "bias" in fallback_reason(x, nn.Conv2d(8, 8, 3, 1, 2, 2, groups=8, bias=True), bn)
    assert "depthwise" in fallback_reason(x, nn.Conv2d(8, 8, 3, 1, 2, 2, groups=4, bias=False), bn)
    assert "depthwise" in fallback_reason(x, nn.Conv2d(8, 16, 3, 1, 2, 2, groups=8, bias=False), bn)
    assert "kernel" in fallback_reason(x, nn.Conv2d(8, 8, 5, 1, 2, 1, groups=8, bias=False), bn)
    assert "stride" in fallback_reason(x, nn.Conv2d(8, 8, 3, 2, 2, 2, groups=8, bias=False), bn)
    assert "padding" in fallback_reason(x, nn.Conv2d(8, 8, 3, 1, 1, 2, groups=8, bias=False), bn)
    assert "padding" in fallback_reason(x, nn.Conv2d(8, 8, 3, 1, (2, 1), (2, 1), groups=8, bias=False), bn)
    assert "padding" in fallback_reason(x, nn.Conv2d(8, 8, 3, 1, "same", 1, groups=8, bias=False), bn)
    assert "padding_mode" in fallback_reason(x, nn.Conv2d(8, 8, 3, 1, 2, 2, groups=8, bias=False, padding_mode="reflect"), bn)
    assert "not nn.Conv2d" in fallback_reason(x, nn.Conv1d(8, 8, 3), bn)
    assert "channels" in fallback_reason(_OnDevice(2, 6, 5, 7), conv, bn)
    assert "channels" in fallback_reason(x, conv, R.FrozenBatchNorm2d(6))
    assert "(B, C, H, W)" in fallback_reason(_OnDevice(8, 5, 7), conv, bn)
    assert "empty" in fallback_reason(_OnDevice(0, 8, 5, 7), conv, bn)
    half = _OnDevice(2, 8, 5, 7)
    half.dtype = torch.float16
    assert "float32" in fallback_reason(half, conv, bn)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert "autocast" in fallback_reason(x, conv, bn)
    assert "float32 on" in fallback_reason(x, conv.double(), bn)
    monkeypatch.undo()
    assert "device" in fallback_reason(torch.zeros(2, 8, 5, 7), *_pair())                    # CPU tensors: the torch statements
    assert "float32" in fallback_reason(torch.zeros(2, 8, 5, 7, dtype=torch.float64), *_pair())
    assert dwconv.torch_statement is not None


@pytest.mark.parametrize("kind", ["frozen", "eval_bn", "train_bn"])
def test_cpu_tensors_run_the_stock_statements(kind):
    from halo_amd.dwconv import depthwise_bn_relu
    torch.manual_seed(3)
    conv = nn.Conv2d(6, 6, 3, 1, 2, 2, groups=6, bias=False)
    bn = {"frozen": R.FrozenBatchNorm2d(6), "eval_bn": nn.BatchNorm2d(6).eval(), "train_bn": nn.BatchNorm2d(6)}[kind]
    with torch.no_grad():
        bn.running_var.copy_(0.5 + torch.rand(6))
        bn.running_mean.copy_(torch.randn(6))
    twin = nn.BatchNorm2d(6)
    if kind == "train_bn":
        twin.load_state_dict(bn.state_dict())
    act = nn.ReLU(inplace=True)
    x1, x2 = (torch.randn(2, 6, 7, 9).requires_grad_(True) for _ in range(2))
    with torch.no_grad():
        x2.copy_(x1)
    g = torch.randn(2, 6, 7, 9)
    y1 = depthwise_bn_relu(x1, conv, bn, act)
    gx1, gw1 = torch.autograd.grad(y1, [x1, conv.weight], g)
    y2 = act((twin if kind == "train_bn" else bn)(conv(x2)))
    gx2, gw2 = torch.autograd.grad(y2, [x2, conv.weight], g)
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2) and torch.equal(gw1, gw2)
    if kind == "train_bn":
        assert torch.equal(bn.running_mean, twin.running_mean) and int(bn.num_batches_tracked) == 1


class Block(nn.Module):
    """a stand-in with the reference block's attribute names"""

    def __init__(self, cin=6, cout=10, d=2, norm=R.FrozenBatchNorm2d, act=nn.ReLU):
        super().__init__()
        self.depthwise_conv = nn.Conv2d(cin, cin, 3, 1, d, d, groups=cin, bias=False)
        self.depthwise_bn = norm(cin)
        self.depthwise_activate = act()
        self.pointwise_conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.pointwise_bn = norm(cout)
        self.pointwise_activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.depthwise_activate(self.depthwise_bn(self.depthwise_conv(x)))
        return self.pointwise_activate(self.pointwise_bn(self.pointwise_conv(x)))


def test_hook_binds_an_opt_in_forward_and_keeps_the_previous_one():
    import halo_amd
    from halo_amd.hooks import fused_dwsep_forward, use_fused_depthwise
    Sub = type("Sub", (Block,), {})
    assert use_fused_depthwise(Sub) is Sub
    assert Sub.forward is fused_dwsep_forward and Sub._unfused_forward is Block.__dict__["forward"]
    assert use_fused_depthwise(Sub)._unfused_forward is Block.__dict__["forward"]              # idempotent
    assert Block.forward is not fused_dwsep_forward
    Named = type("DepthwiseSeparableConv2d", (nn.Module,), {"forward": lambda self, x: x})      # the reference's name is enough
    assert use_fused_depthwise(Named).forward is fused_dwsep_forward
    for bad in (nn.Conv2d, nn.Sequential, type("NoModule", (), {}), Block()):
        with pytest.raises(TypeError):
            use_fused_depthwise(bad)
    init = open(os.path.join(os.path.dirname(halo_amd.__file__), "__init__.py")).read() + open(
        os.path.join(os.path.dirname(halo_amd.__file__), "_install.py")).read()
    assert "use_fused_depthwise" not in init and "fused_dwsep_forward" not in init             # install() does not bind it


def _same_as_unhooked(make):
    from halo_amd.hooks import use_fused_depthwise
    torch.manual_seed(5)
    plain = make()
    Hooked = use_fused_depthwise(type(type(plain).__name__, (type(plain),), {}))
    hooked = make()
    hooked.__class__ = Hooked
    hooked.load_state_dict(plain.state_dict())
    cin = plain.depthwise_conv.in_channels
    x1 = torch.randn(2, cin, 9, 11).requires_grad_(True)
    x2 = x1.detach().clone().requires_grad_(True)
    y1, y2 = plain(x1), hooked(x2)
    g = torch.randn_like(y1)
    p1 = [p for p in plain.parameters() if p.requires_grad]
    p2 = [p for p in hooked.parameters() if p.requires_grad]
    for a, b in zip(torch.autograd.grad(y1, [x1] + p1, g), torch.autograd.grad(y2, [x2] + p2, g)):
        assert torch.equal(a, b)
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("norm,act", [(R.FrozenBatchNorm2d, nn.ReLU), (nn.BatchNorm2d, nn.ReLU), (R.FrozenBatchNorm2d, nn.GELU)])
def test_hooked_block_equals_the_unhooked_block_on_cpu(norm, act):
    _same_as_unhooked(lambda: Block(norm=norm, act=act))


REF = os.environ.get("HALO_REFERENCE", "/root/reference")          # as tests/golden/make_fixtures.py


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "core")), reason="the reference's tree is not present")
def test_hooked_reference_block_equals_the_unhooked_one_on_cpu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_dwconv_fixtures import import_blocks
    Ref, Frozen = import_blocks()
    _same_as_unhooked(lambda: Ref(6, 10, 3, 1, 2, 2, False, norm_layer=Frozen))
    assert "forward" in Ref.__dict__ and Ref.__dict__["forward"].__name__ == "forward"          # the reference class itself is untouched


def test_fixture_covers_the_listed_cases():
    cs = {n: R.load(n) for n in R.case_names()}
    shapes = {(c["d"], c["B"], c["C"], c["H"], c["W"]) for c in cs.values()}
    assert {(1, 2, 24, 20, 36), (6, 2, 16, 24, 40), (12, 1, 16, 40, 44), (18, 1, 8, 40, 48), (1, 2, 560, 12, 20)} <= shapes
    assert any(c["W"] % 4 for c in cs.values()) and any(c["H"] < c["d"] and c["W"] < c["d"] for c in cs.values())
    assert any(c["kind"] == R.BATCHNORM for c in cs.values())
    for c in cs.values():
        assert 0.25 <= c["weight"].min() and c["weight"].max() <= 1.75 and 0.3 <= c["running_var"].min() and c["running_var"].max() <= 1.8
        assert np.abs(c["running_mean"]).min() > 0 and np.abs(c["bias"]).min() > 0
    assert os.path.getsize(R.FIX) < 1 << 20


@pytest.mark.parametrize("name", R.case_names())
def test_evaluator_agrees_with_the_reference_modules(name):
    """the numpy float64 statements against what the reference's modules gave in float64: a few float64 roundings apart"""
    c = R.load(name)
    ch = c["chans"]
    pre, bound = R.forward(c)
    assert np.abs(pre[:, ch] - c["pre64"]).max() <= 1e-13
    mask = pre > 0
    gx, _ = R.grad_x(c, mask)
    assert np.abs(gx[:, ch] - c["gx64"]).max() <= 1e-12
    gw, _ = R.grad_w(c, mask)
    assert np.abs(gw - c["gw64"]).max() <= 1e-10 * max(1.0, np.abs(c["gw64"]).max())


@pytest.mark.parametrize("name", R.case_names())
def test_fixture_self_check(name):
    """the stock float32 forward lies within the forward bound of the float64 pre-activation (through y: ReLU is 1-Lipschitz), and
    the near-zero band |pre_64| <= bound holds at most 1e-4 of the elements"""
    c = R.load(name)
    ch = c["chans"]
    pre, bound = R.forward(c)
    assert (np.abs(c["y32"].astype(np.float64) - np.maximum(c["pre64"], 0)) <= bound[:, ch]).all()
    assert (np.abs(pre) <= bound).mean() <= 1e-4


def test_float32_reference_chain_stays_inside_both_conditions():
    """CPU torch, inputs drawn as the fixture's: the float32 chain reaches at most 0.30 of the bound, the band holds at most 4e-6 of
    the elements, and the float32 and float64 ReLU masks never disagree"""
    rng = np.random.default_rng(11)
    worst, band, n, disagree = 0.0, 0, 0, 0
    for d, shape in ((1, (2, 24, 20, 36)), (6, (2, 16, 24, 40)), (12, (1, 16, 40, 44)), (18, (1, 8, 40, 48)), (1, (2, 560, 12, 20))):
        B, C, H, W = shape
        c = {"B": B, "C": C, "H": H, "W": W, "d": d, "kind": R.FROZEN, "eps": np.array(np.nan),
             "x": (np.clip(np.round(rng.standard_normal(shape) * 4), -12, 12) / 4).astype(np.float32),
             "w": ((rng.random((C, 1, 3, 3)) * 2 - 1) / 3).astype(np.float32),
             "weight": (0.25 + 1.5 * rng.random(C)).astype(np.float32), "bias": (0.4 * rng.standard_normal(C) + 0.1).astype(np.float32),
             "running_mean": (0.5 * rng.standard_normal(C) + 0.2).astype(np.float32), "running_var": (0.3 + 1.5 * rng.random(C)).astype(np.float32)}
        conv, bn = R.modules(c)
        with torch.no_grad():
            pre32 = bn(conv(torch.from_numpy(c["x"]))).numpy().astype(np.float64)
        pre, bound = R.forward(c)
        worst = max(worst, float((np.abs(pre32 - pre) / bound).max()))
        band += int((np.abs(pre) <= bound).sum())
        n += pre.size
        disagree += int(((pre32 > 0) != (pre > 0)).sum())
    assert worst <= 0.30 and band <= 4e-6 * n and disagree == 0, (worst, band, n, disagree)
