"""CPU checks of the depthwise half under autocast (halo_half_dwconv3x3_* of halo_dwconv.hip, halo_amd.dwconv.depthwise_bn_relu_autocast,
halo_amd.hooks.use_autocast_depthwise): the statements the kernels run, restated in tests/dwconv_autocast_ref.py, are
torch.autocast + autograd's bits for float16 and bfloat16 and for a float32 and a half x; the one stated deviation; few elements of
the generated cases are excused; header, binding and library agree; the entry points refuse bad arguments before any launch; every
clause of the envelope; the hook; and with autocast off nothing changes."""
import contextlib
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT
import dwconv_autocast_ref as R
import dwconv_cases as K
from dwconv_ref import FrozenBatchNorm2d

SYMBOLS = ("halo_half_dwconv3x3_affine_relu_fwd", "halo_half_dwconv3x3_affine_relu_bwd_data", "halo_half_dwconv3x3_affine_relu_bwd_weight")
E_ARG, E_WORKSPACE = -1, -3                # HALO_E_ARG, HALO_E_WORKSPACE of include/halo_hip.h
IDS = ["float16", "bfloat16"]
SHAPE = (2, 3, 50, 44, 3)                  # the shape the chain was first checked at


def _autocast_chain(x, w, scale, shift, d, dt, g16):
    """the stock statements under torch.autocast("cpu", dt), the cast in front of the next conv, and autograd"""
    xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=dt):
        c = F.conv2d(xs, ws, None, 1, d, d, x.shape[1])
        y = torch.relu(c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
        y16 = y.to(dt)
    assert c.dtype == dt and y.dtype == torch.float32
    gx, gw = torch.autograd.grad(y16, [xs, ws], g16)
    return y16.detach(), gx, gw


@pytest.mark.parametrize("half_x", [False, True], ids=["x32", "x16"])
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("dt", R.HALVES, ids=IDS)
def test_statements_equal_autocast_and_autograd(dt, kind, half_x):
    x, w, g, scale, shift = (R.exact_case if kind == "exact" else R.random_case)(3, *SHAPE)
    x = x.to(dt) if half_x else x
    g16 = g.to(dt)
    y16, gx, gw = _autocast_chain(x, w, scale, shift, SHAPE[4], dt, g16)
    f = R.forward(x, w, scale, shift, SHAPE[4], dt)
    assert f.y16.dtype == dt and torch.equal(f.y16, y16)
    assert int(((f.y32 > 0) & (f.y16 == 0)).sum()) == 0                          # no element at which the gate deviates (below)
    b = R.backward(g16, f.y16, x, w, scale, SHAPE[4], dt)
    assert b.g_x.dtype == gx.dtype == x.dtype and torch.equal(b.g_x, gx)
    assert b.g_w.dtype == gw.dtype == torch.float32 and torch.equal(b.g_w, gw)
    assert torch.equal(b.g_x.float(), b.g_x.float().to(dt).float()) and torch.equal(gw, gw.to(dt).float())     # half values
    assert 0 < int((f.y16 > 0).sum()) < f.y16.numel()


def test_the_gate_is_read_off_y16_the_one_deviation():
    """scale 2^-20, shift 0, x = 2^-10 under a centre tap of 1: c16 = 2^-10, y32 = 2^-30 > 0 and the float16 y16 is 0.  autograd's
    gradient passes there; the pass, whose gate is y16, writes 0 -- where the next conv saw 0 on both sides"""
    dt = torch.float16
    x = torch.full((1, 1, 3, 3), 2.0 ** -10)
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0, 1, 1] = 1.0
    scale, shift = torch.tensor([2.0 ** -20]), torch.zeros(1)
    g16 = torch.full((1, 1, 3, 3), 1024.0, dtype=dt)
    y16, gx, gw = _autocast_chain(x, w, scale, shift, 1, dt, g16)
    f = R.forward(x, w, scale, shift, 1, dt)
    assert bool((f.y32 > 0).all()) and bool((f.y16 == 0).all()) and torch.equal(f.y16, y16)
    b = R.backward(g16, f.y16, x, w, scale, 1, dt)
    assert bool((gx > 0).all()) and bool((b.g_x == 0).all()) and bool((b.g_w == 0).all())
    # with the gate off y32 the same statements are autograd's again: the deviation is the gate alone
    open_gate = R.backward(g16, torch.ones_like(f.y16), x, w, scale, 1, dt)
    assert torch.equal(open_gate.g_x, gx) and torch.equal(open_gate.g_w, gw)


@pytest.mark.parametrize("dt", R.HALVES, ids=IDS)
@pytest.mark.parametrize("name", list(R.RANDOM_TIER))
def test_few_elements_of_a_generated_case_are_excused(name, dt):
    """a condition on the inputs, from the float64 evaluation alone: at most 1 % of y16, of g_x and of g_w"""
    shape = K.PLAIN[name][0]
    x, w, g, scale, shift = R.random_case(R.RANDOM_TIER[name], *shape)
    f = R.forward(x, w, scale, shift, shape[4], dt)
    b = R.backward(g.to(dt), f.y16, x, w, scale, shape[4], dt)
    for excused in (f.excused, b.gx_excused, b.gw_excused):
        assert float(excused.float().mean()) <= 0.01
    if f.y16.numel() > 100:
        assert 0.1 < float((f.y16 > 0).float().mean()) < 0.9                     # both sides of the gate


def test_the_excuse_is_the_rounding_band_of_a_half():
    for dt, step in ((torch.float16, 2.0 ** -10), (torch.bfloat16, 2.0 ** -7)):
        s = torch.tensor([1.0 + step / 2, 1.0 + step / 2 + 1e-6, 1.0 + step / 2 - 1e-6, 1.0 + step / 4, 1.0, -1.0 - 1.5 * step], dtype=torch.float64)
        r, alt, exc = R.round_with_excuse(s, torch.full_like(s, 2e-6), dt)
        assert exc.tolist() == [True, True, True, False, False, True]
        assert r.double().tolist() == [1.0, 1.0 + step, 1.0, 1.0, 1.0, -1.0 - 2 * step]
        assert alt.double().tolist() == [1.0 + step, 1.0, 1.0 + step, 1.0, 1.0, -1.0 - step]
    big = torch.tensor([65519.0, 65521.0, 70000.0], dtype=torch.float64)                        # the overflow boundary of float16
    r, alt, exc = R.round_with_excuse(big, torch.full_like(big, 2.0), torch.float16)
    assert exc.tolist() == [True, True, False] and r.double().tolist() == [65504.0, float("inf"), float("inf")]
    assert alt.double().tolist() == [float("inf"), 65504.0, float("inf")]


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    assert set(re.findall(r"\b(halo_half_\w+)\s*\(", text)) == set(SYMBOLS)
    assert "#define HALO_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13
    assert "halo_dwconv.hip" in _build.SOURCES and "halo_half_dev.hpp" in _build.HEADERS
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
    assert h.halo_version() == 13


def test_argument_checks_are_host_code():
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd, bww = L.halo_half_dwconv3x3_affine_relu_fwd, L.halo_half_dwconv3x3_affine_relu_bwd_data, L.halo_half_dwconv3x3_affine_relu_bwd_weight
    n = L.halo_dwconv_workspace_bytes(1, 2, 4, 4, 1)
    dims = (1, 2, 4, 4, 1)
    for dt in (_lib.F16, _lib.BF16):
        for xd in (_lib.F32, dt):
            for i in (0, 2, 3, 4, 5):                                                    # every pointer of the forward
                args = [a, xd, a, a, a, a, dt, *dims, None]
                args[i] = None
                assert fwd(*args) == E_ARG
            for i in (0, 1, 2, 3, 4):
                args = [a, a, a, a, a, xd, dt, *dims, None]
                args[i] = None
                assert bwd(*args) == E_ARG
            for i in (0, 1, 2, 4, 5):
                args = [a, a, a, xd, a, a, dt, *dims, a, n, None]
                args[i] = None
                assert bww(*args) == E_ARG
            for bad in ((0, 2, 4, 4, 1), (1, 0, 4, 4, 1), (1, 2, 0, 4, 1), (1, 2, 4, 0, 1), (1, 2, 4, 4, 0)):      # empty shapes, d < 1
                assert fwd(a, xd, a, a, a, a, dt, *bad, None) == E_ARG
                assert bwd(a, a, a, a, a, xd, dt, *bad, None) == E_ARG
                assert bww(a, a, a, xd, a, a, dt, *bad, a, n, None) == E_ARG
            for big in ((1, 2, 1 << 25, 4, 1), (1, 2, 4, 1 << 25, 1), (1, 2, 4, 4, 1 << 25), (1, 2, 1 << 16, 1 << 16, 1), (1 << 21, 1 << 20, 4, 4, 1)):
                assert fwd(a, xd, a, a, a, a, dt, *big, None) == _lib.E_UNSUPPORTED                              # section 14's limits
                assert bwd(a, a, a, a, a, xd, dt, *big, None) == _lib.E_UNSUPPORTED
                assert bww(a, a, a, xd, a, a, dt, *big, a, n, None) == _lib.E_UNSUPPORTED
            assert bww(a, a, a, xd, a, a, dt, *dims, a, n - 1, None) == E_WORKSPACE
            assert bww(a, a, a, xd, a, a, dt, *dims, None, n, None) == E_WORKSPACE
        other = _lib.BF16 if dt == _lib.F16 else _lib.F16
        for xd in (other, _lib.F64, _lib.U8, 7, -1):                                     # x_dtype / gx_dtype outside {F32, half_dtype}
            assert fwd(a, xd, a, a, a, a, dt, *dims, None) == E_ARG
            assert bwd(a, a, a, a, a, xd, dt, *dims, None) == E_ARG
            assert bww(a, a, a, xd, a, a, dt, *dims, a, n, None) == E_ARG
    for dt in (_lib.F32, _lib.F64, _lib.U8, 7, -1):                                      # half_dtype outside {F16, BF16}
        assert fwd(a, _lib.F32, a, a, a, a, dt, *dims, None) == E_ARG
        assert bwd(a, a, a, a, a, _lib.F32, dt, *dims, None) == E_ARG
        assert bww(a, a, a, _lib.F32, a, a, dt, *dims, a, n, None) == E_ARG
    assert "halo_half_dwconv3x3" in L.halo_last_error().decode()


class _OnDevice:
    """describes a contiguous ROCm tensor without one: autocast_fallback_reason reads attributes only"""
    is_cuda = True

    def __init__(self, *shape, contiguous=True, dtype=torch.float32, device="cpu"):
        self.shape, self._c, self.dtype, self.device = torch.Size(shape), contiguous, dtype, torch.device(device)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c


@contextlib.contextmanager
def _device_autocast(dtype):
    """the device's autocast state as torch.autocast("cuda", dtype) sets it, on a host that may have no device"""
    was, dt = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    torch.set_autocast_enabled("cuda", True)
    torch.set_autocast_dtype("cuda", dtype)
    try:
        yield
    finally:
        torch.set_autocast_enabled("cuda", was)
        torch.set_autocast_dtype("cuda", dt)


def _dw(C=8, d=2, **kw):
    args = dict(kernel_size=3, stride=1, padding=d, dilation=d, groups=C, bias=False)
    args.update(kw)
    return nn.Conv2d(C, C, **args)


def test_envelope_decisions(monkeypatch):
    from halo_amd.dwconv import autocast_fallback_reason as reason, fallback_reason
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    conv, bn = _dw(), FrozenBatchNorm2d(8)
    x32 = _OnDevice(2, 8, 5, 7)
    assert "autocast is not enabled" in reason(x32, conv, bn) and fallback_reason(x32, conv, bn) is None         # autocast off
    for dt, other in ((torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16)):
        x16 = _OnDevice(2, 8, 5, 7, dtype=dt)
        with _device_autocast(dt):
            assert reason(x32, conv, bn) is None and reason(x16, conv, bn) is None
            assert fallback_reason(x32, conv, bn) == "autocast is enabled"                                        # as before
            assert "neither float32 nor" in reason(_OnDevice(2, 8, 5, 7, dtype=other), conv, bn)
            assert "neither float32 nor" in reason(_OnDevice(2, 8, 5, 7, dtype=torch.float64), conv, bn)
            # section 14's module envelope
            assert "nn.Conv2d" in reason(x32, nn.Identity(), bn)
            assert "depthwise" in reason(x32, nn.Conv2d(8, 8, 3, padding=1, bias=False), bn)
            assert "kernel size" in reason(x32, _dw(kernel_size=5), bn)
            assert "stride" in reason(x32, _dw(stride=2), bn)
            assert "dilation" in reason(x32, _dw(padding=1), bn) and "dilation" in reason(x32, _dw(padding="same"), bn)
            assert "padding_mode" in reason(x32, _dw(padding_mode="reflect"), bn)
            assert "bias" in reason(x32, _dw(bias=True), bn)
            assert "BatchNorm with batch statistics" in reason(x32, conv, nn.BatchNorm2d(8))
            assert "neither a FrozenBatchNorm2d" in reason(x32, conv, nn.GroupNorm(2, 8))
            assert "channels" in reason(x32, conv, FrozenBatchNorm2d(6))
            # an eval-mode BatchNorm2d is in section 14's envelope, but on a half input it is the library's batch norm, not these statements
            assert "FrozenBatchNorm2d" in reason(x32, conv, nn.BatchNorm2d(8).eval().requires_grad_(False))
            # the operand
            assert "(B, C, H, W)" in reason(_OnDevice(8, 5, 7), conv, bn) and "(B, C, H, W)" in reason([1.0], conv, bn)
            assert "channels" in reason(_OnDevice(2, 6, 5, 7), conv, bn)
            assert "device" in reason(torch.zeros(2, 8, 5, 7), conv, bn)                                          # CPU tensors
            assert "contiguous" in reason(_OnDevice(2, 8, 5, 7, contiguous=False), conv, bn)
            assert "empty" in reason(_OnDevice(0, 8, 5, 7), conv, bn)
            assert "plane" in reason(_OnDevice(1, 8, 1 << 16, 1 << 15), conv, bn) and "plane" in reason(_OnDevice(1, 8, 2, (1 << 24) + 1), conv, bn)
            assert "float32 on" in reason(x32, _dw().double(), bn) and "float32 on" in reason(x32, conv, FrozenBatchNorm2d(8).double())
            assert "float32 on" in reason(_OnDevice(2, 8, 5, 7, device="meta"), conv, bn)
    with _device_autocast(torch.float32):
        assert "not float16 or bfloat16" in reason(x32, conv, bn)
    assert not torch.is_autocast_enabled("cuda")


@pytest.mark.parametrize("dt", R.HALVES, ids=IDS)
def test_cpu_tensors_run_the_stock_statements(dt):
    from halo_amd import dwconv
    x, w, g, scale, shift = R.random_case(5, 2, 3, 9, 11, 2)
    conv, bn = R.modules(w, scale, shift, 2)
    before = dict(dwconv.autocast_launches)
    assert set(before) == {"fwd", "bwd_data", "bwd_weight"}
    with torch.autocast("cpu", dtype=dt):
        got = dwconv.depthwise_bn_relu_autocast(x, conv, bn)
        want = dwconv.autocast_statement(x, conv, bn)
        stock = dwconv.torch_statement(x, conv, bn)
    assert got.dtype == want.dtype == torch.float32 and torch.equal(got, want) and torch.equal(got, stock)     # the DEVICE's autocast is off
    with torch.autocast("cpu", dtype=dt), _device_autocast(dt):
        half = dwconv.autocast_statement(x, conv, bn)
        got = dwconv.depthwise_bn_relu_autocast(x, conv, bn, nn.ReLU(inplace=True))
    assert half.dtype == dt and torch.equal(half, R.forward(x, w, scale, shift, 2, dt).y16) and torch.equal(got, half)
    assert dwconv.autocast_launches == before


class _Block(nn.Module):
    """a separable block with the reference's six attributes and forward"""

    def __init__(self, C=4, d=2):
        super().__init__()
        self.depthwise_conv = _dw(C, d)
        self.depthwise_bn = FrozenBatchNorm2d(C)
        self.depthwise_activate = nn.ReLU(inplace=True)
        self.pointwise_conv = nn.Conv2d(C, 6, 1, bias=False)
        self.pointwise_bn = FrozenBatchNorm2d(6)
        self.pointwise_activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.depthwise_activate(self.depthwise_bn(self.depthwise_conv(x)))
        return self.pointwise_activate(self.pointwise_bn(self.pointwise_conv(x)))


def _count_calls(block):
    calls = {}
    for name, m in block.named_children():
        m.register_forward_hook(lambda mod, a, out, name=name: calls.__setitem__(name, calls.get(name, 0) + 1))
    return calls


def test_the_hook_is_an_opt_in_mark_on_a_bound_class(monkeypatch):
    from halo_amd import dwconv, hooks, install
    class Unbound(_Block):
        pass
    class Bound(_Block):
        pass
    with pytest.raises(TypeError, match="use_fused_depthwise"):
        hooks.use_autocast_depthwise(Unbound)
    for junk in (nn.ReLU, object, 3, None, _Block()):
        with pytest.raises(TypeError):
            hooks.use_autocast_depthwise(junk)
    hooks.use_fused_depthwise(Bound)
    assert not getattr(Bound, "_halo_autocast_depthwise", False)                  # use_fused_depthwise alone does not set it
    assert hooks.use_autocast_depthwise(Bound) is Bound and hooks.use_autocast_depthwise(Bound) is Bound
    assert Bound._halo_autocast_depthwise is True and Bound.forward is hooks.fused_dwsep_forward and Bound._unfused_forward is _Block.forward
    assert not hasattr(Unbound, "_halo_autocast_depthwise") and not hasattr(_Block, "_halo_autocast_depthwise")
    assert "use_autocast_depthwise" not in open(os.path.join(ROOT, "halo_amd", "_install.py")).read()          # install() binds nothing

    # with autocast off, and on the CPU, a marked block calls its six modules once each and returns the unmarked block's bits
    torch.manual_seed(1)
    plain, marked = _Block(), Bound()
    marked.load_state_dict(plain.state_dict())
    x = torch.randn(2, 4, 7, 9)
    calls = _count_calls(marked)
    never = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the autocast operator ran"))
    monkeypatch.setattr(dwconv, "depthwise_bn_relu_autocast", never)
    assert torch.equal(marked(x), plain(x)) and calls == {n: 1 for n in hooks._DWSEP_ATTRS}
    with torch.autocast("cpu", dtype=torch.bfloat16):
        got, want = marked(x), plain(x)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(hooks.depthwise_half(marked, x), plain.depthwise_activate(plain.depthwise_bn(plain.depthwise_conv(x))))

    # where the envelope holds, the forward and depthwise_half hand the operator's result to the pointwise modules
    seen = []

    def operator(x, conv, bn, act=None):
        seen.append((conv, bn, act))
        return dwconv.torch_statement(x, conv, bn, act)
    monkeypatch.setattr(dwconv, "autocast_fallback_reason", lambda x, conv, bn: None)
    monkeypatch.setattr(dwconv, "depthwise_bn_relu_autocast", operator)
    calls.clear()
    assert torch.equal(marked(x), plain(x))
    assert seen == [(marked.depthwise_conv, marked.depthwise_bn, marked.depthwise_activate)]
    assert calls == {"depthwise_conv": 1, "depthwise_bn": 1, "depthwise_activate": 1, "pointwise_conv": 1, "pointwise_bn": 1, "pointwise_activate": 1}
    hooks.depthwise_half(marked, x)
    assert len(seen) == 2
    marked.depthwise_activate = nn.ReLU6()                                        # not an nn.ReLU: the stock statements
    marked(x)
    assert len(seen) == 2
    class Unmarked(_Block):
        pass
    hooks.use_fused_depthwise(Unmarked)
    Unmarked()(x)
    assert len(seen) == 2


def test_a_marked_pointwise_tail_asks_the_autocast_norm_first(monkeypatch):
    from halo_amd import hooks, norm
    class Tail(_Block):
        pass
    hooks.use_fused_pointwise_norm(hooks.use_fused_depthwise(Tail))
    torch.manual_seed(2)
    block, plain = Tail(), _Block()
    block.load_state_dict(plain.state_dict())
    x = torch.randn(2, 4, 7, 9)
    asked, ran = [], []
    stock_reason, stock = norm.autocast_fallback_reason, norm.norm_relu
    monkeypatch.setattr(norm, "autocast_fallback_reason", lambda *a, **k: asked.append(a[1]) or stock_reason(*a, **k))
    monkeypatch.setattr(norm, "norm_relu", lambda x, bn, *a: ran.append(bn) or stock(x, bn, *a))
    monkeypatch.setattr(norm, "norm_relu_autocast", lambda *a, **k: (_ for _ in ()).throw(AssertionError("autocast is off")))
    assert torch.equal(block(x), plain(x))
    assert asked == [block.pointwise_bn] and ran == [block.pointwise_bn]         # autocast off: norm_relu as before
    # where norm_relu_autocast's envelope holds, the tail runs it with the float32 output
    monkeypatch.setattr(norm, "autocast_fallback_reason", lambda *a, **k: None)
    got = []
    monkeypatch.setattr(norm, "norm_relu_autocast", lambda x, bn, r, rbn, outputs: got.append((bn, r, rbn, outputs)) or stock(x, bn))
    assert torch.equal(block(x), plain(x)) and got == [(block.pointwise_bn, None, None, "float")] and len(ran) == 1
