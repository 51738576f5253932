"""CPU checks of the frozen-norm passes under autocast (halo_norm_autocast.hip, halo_amd.norm.norm_relu_autocast): the statements
the kernels run, restated in tests/norm_autocast_ref.py, are torch.autocast + autograd's bits for float16 and bfloat16; every
envelope decision; the entry points refuse bad arguments before any launch; and with autocast off the hooks resolve as before."""
import contextlib
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import norm_autocast_ref as A
import norm_ref as N
from dwconv_ref import FrozenBatchNorm2d

SYMBOLS = ("halo_autocast_norm_relu_fwd", "halo_autocast_norm_relu_bwd")
E_ARG = -1                # HALO_E_ARG of include/halo_hip.h
HALVES = [torch.float16, torch.bfloat16]


def _norm(C, seed):
    """tests/test_gpu_norm_relu.py's: channel 0 scale -2 / shift +1, channel 1 scale +2 / shift -1, the rest random with both signs"""
    bn = N.randomize_norms(FrozenBatchNorm2d(C), seed)
    with torch.no_grad():
        bn.weight[0], bn.running_var[0], bn.bias[0], bn.running_mean[0] = -2.0, 1.0, 1.0, 0.0
        bn.weight[1], bn.running_var[1], bn.bias[1], bn.running_mean[1] = 2.0, 1.0, -1.0, 0.0
    return bn


@pytest.mark.parametrize("dt", HALVES, ids=["float16", "bfloat16"])
def test_statements_equal_autocast_and_autograd_between_two_convolutions(dt):
    """conv -> FrozenBatchNorm2d -> ReLU -> conv under torch.autocast("cpu", dt): the first conv returns half, the chain float32,
    the second conv reads autocast's cast of it.  The restated y32 is the chain's, the restated y16 gives the second conv the same
    result as that cast, and from the gradient that reaches y16 the restated g_x is what autograd hands the first conv's output."""
    torch.manual_seed(3)
    conv_a, conv_b = nn.Conv2d(3, 6, 3, padding=1, bias=False), nn.Conv2d(6, 4, 1, bias=False)
    bn = _norm(6, 5)
    x0 = torch.randn(2, 3, 9, 11)
    gz = torch.randn(2, 4, 9, 11)
    with torch.autocast("cpu", dtype=dt):
        a = conv_a(x0)
        assert a.dtype == dt
        a = a.detach().requires_grad_(True)
        y = N.stock_chain(a, bn)
        assert y.dtype == torch.float32
        z = conv_b(y)
        assert z.dtype == dt
        (ga,) = torch.autograd.grad(z, [a], gz.to(dt))
        s, y32, y16 = A.forward(a.detach(), bn)
        leaf = y16.clone().requires_grad_(True)
        z_ref = conv_b(leaf)
        (g16,) = torch.autograd.grad(z_ref, [leaf], gz.to(dt))
    assert torch.equal(y32, y.detach()) and y16.dtype == dt and torch.equal(z_ref.detach(), z.detach())
    assert g16.dtype == dt and ga.dtype == dt
    g_x, _ = A.backward(s, bn, None, dt, g16=g16)
    assert torch.equal(g_x, ga)
    assert int((y32 == 0).sum()) > 0 and int((y32 > 0).sum()) > 0


@pytest.mark.parametrize("residual", ["identity", "downsample"])
@pytest.mark.parametrize("dt", HALVES, ids=["float16", "bfloat16"])
def test_statements_equal_autocast_and_autograd_over_a_bottleneck_tail(dt, residual):
    """resnet.py's tail `out = bn3(conv3 output); out += identity; relu_(out)` under autocast, the identity float32 (the block's
    input) or the downsample norm of a half convolution output; the result goes on as float32 and, cast, to the next conv1.  Both
    gradients arrive: y32, y16, g_x and g_r are autograd's bits, the sum of the two gradients included."""
    gen = torch.Generator().manual_seed(11)
    shape = (2, 5, 7, 9)
    bn, rbn = _norm(5, 13), _norm(5, 17) if residual == "downsample" else None
    x = torch.randn(shape, generator=gen).to(dt)
    x[0, 0, 0, :3], x[0, 1, 0, :3] = 0.5, 0.5                                  # pre == 0 in channels 0 and 1
    r = torch.randn(shape, generator=gen)
    r = r.to(dt) if rbn is not None else r
    g32, g16 = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen).to(dt)
    xs, rs = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=dt):
        y = N.stock_chain(xs, bn, rs, rbn)
        yh = y.to(dt)
        gx, gr = torch.autograd.grad([y, yh], [xs, rs], [g32, g16])
    s, y32, y16 = A.forward(x, bn, r, rbn)
    assert y.dtype == torch.float32 and torch.equal(y32, y.detach()) and torch.equal(y16, yh.detach())
    g_x, g_r = A.backward(s, bn, rbn, dt, g32=g32, g16=g16)
    assert g_x.dtype == gx.dtype == dt and g_r.dtype == gr.dtype == r.dtype
    assert torch.equal(g_x, gx) and torch.equal(g_r, gr)
    for only in ({"g32": g32}, {"g16": g16}):                                 # one gradient alone
        with torch.autocast("cpu", dtype=dt):
            y = N.stock_chain(xs, bn, rs, rbn)
            yh = y.to(dt)
            gx, gr = torch.autograd.grad([y], [xs, rs], [g32]) if "g32" in only else torch.autograd.grad([yh], [xs, rs], [g16])
        g_x, g_r = A.backward(s, bn, rbn, dt, **only)
        assert torch.equal(g_x, gx) and torch.equal(g_r, gr)


def test_a_half_zero_does_not_close_the_gate():
    """scale 2^-20, shift 0, x = 2^-10: y32 = 2^-30 > 0 and the float16 y16 is 0; autograd's gradient passes there, which a gate
    read off y16 would stop"""
    bn = FrozenBatchNorm2d(1)
    with torch.no_grad():
        bn.weight[0] = 2.0 ** -20
    x = torch.full((1, 1, 2, 2), 2.0 ** -10, dtype=torch.float16)
    xs = x.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.float16):
        yh = N.stock_chain(xs, bn).to(torch.float16)
        (gx,) = torch.autograd.grad(yh, [xs], torch.full_like(yh, 1024.0))
    s, y32, y16 = A.forward(x, bn)
    assert bool((y32 > 0).all()) and bool((y16 == 0).all()) and torch.equal(y16, yh.detach())
    g_x, _ = A.backward(s, bn, None, torch.float16, g16=torch.full_like(y16, 1024.0))
    assert torch.equal(g_x, gx) and bool((gx > 0).all())


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    assert set(re.findall(r"\b(halo_autocast_\w+)\s*\(", text)) == set(SYMBOLS)
    assert "halo_norm_autocast.hip" in _build.SOURCES
    assert re.search(r"HALO_F16 = %d, HALO_BF16 = %d" % (_lib.F16, _lib.BF16), text)
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s


def test_argument_checks_are_host_code():
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = L.halo_autocast_norm_relu_fwd, L.halo_autocast_norm_relu_bwd
    for dt in (_lib.F16, _lib.BF16):
        #          x  scale shift r  r_scale r_shift y32 y16
        assert fwd(None, a, a, None, None, None, a, a, dt, 1, 2, 16, None) == E_ARG          # no x
        assert fwd(a, None, a, None, None, None, a, a, dt, 1, 2, 16, None) == E_ARG          # no scale
        assert fwd(a, a, None, None, None, None, a, a, dt, 1, 2, 16, None) == E_ARG          # no shift
        assert fwd(a, a, a, None, None, None, None, None, dt, 1, 2, 16, None) == E_ARG       # neither output
        assert fwd(a, a, a, a, a, None, a, None, dt, 1, 2, 16, None) == E_ARG                # r_scale without r_shift
        assert fwd(a, a, a, a, None, a, a, None, dt, 1, 2, 16, None) == E_ARG                # r_shift without r_scale
        assert fwd(a, a, a, None, a, a, a, None, dt, 1, 2, 16, None) == E_ARG                # r_scale without r
        for shape in ((0, 2, 16), (1, 0, 16), (1, 2, 0)):
            assert fwd(a, a, a, None, None, None, a, a, dt, *shape, None) == E_ARG           # empty shapes
        assert fwd(a, a, a, None, None, None, a, a, dt, 1, 2, 1 << 31, None) == _lib.E_UNSUPPORTED
        assert fwd(a, a, a, None, None, None, a, a, dt, 1 << 20, 1 << 20, 8192, None) == _lib.E_UNSUPPORTED
        #          g32 g16 y32 x  scale shift r_scale g_x g_r
        assert bwd(None, None, a, None, a, None, None, a, None, dt, 1, 2, 16, None) == E_ARG  # no gradient arrives
        assert bwd(a, None, None, None, a, a, None, a, None, dt, 1, 2, 16, None) == E_ARG    # no gate: neither y32 nor x
        assert bwd(a, None, a, a, a, a, None, a, None, dt, 1, 2, 16, None) == E_ARG          # two gates
        assert bwd(a, None, a, None, a, None, None, None, None, dt, 1, 2, 16, None) == E_ARG  # neither gradient asked for
        assert bwd(a, None, a, None, None, None, None, a, None, dt, 1, 2, 16, None) == E_ARG  # g_x without scale
        assert bwd(None, a, None, a, a, None, None, a, None, dt, 1, 2, 16, None) == E_ARG    # the gate off x without shift
        assert bwd(None, a, None, a, None, a, None, a, None, dt, 1, 2, 16, None) == E_ARG    # ... without scale
        assert bwd(None, a, None, a, a, a, None, a, a, dt, 1, 2, 16, None) == E_ARG          # the gate off x with a g_r
        for shape in ((0, 2, 16), (1, 0, 16), (1, 2, 0)):
            assert bwd(a, a, a, None, a, None, None, a, a, dt, *shape, None) == E_ARG
    for dt in (_lib.F32, _lib.F64, _lib.U8, 7, -1):                                          # not a half dtype
        assert fwd(a, a, a, None, None, None, a, a, dt, 1, 2, 16, None) == E_ARG
        assert bwd(a, None, a, None, a, None, None, a, None, dt, 1, 2, 16, None) == E_ARG
    assert "halo_autocast_norm_relu" in L.halo_last_error().decode()


class _OnDevice:
    """describes a contiguous ROCm tensor without one: autocast_fallback_reason reads attributes only"""
    is_cuda = True

    def __init__(self, *shape, contiguous=True, dtype=torch.float16, device="cpu", grad=False):
        self.shape, self._c, self.dtype, self.device, self.requires_grad = torch.Size(shape), contiguous, dtype, torch.device(device), grad

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

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


def test_envelope_decisions(monkeypatch):
    from halo_amd import norm
    from halo_amd.norm import autocast_fallback_reason as reason, fallback_reason
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    f32 = torch.float32
    bn, rbn = FrozenBatchNorm2d(8), FrozenBatchNorm2d(8)
    for dt, other in ((torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16)):
        x, r16, r32 = _OnDevice(2, 8, 5, 7, dtype=dt), _OnDevice(2, 8, 5, 7, dtype=dt), _OnDevice(2, 8, 5, 7, dtype=f32)
        assert "autocast is not enabled" in reason(x, bn)                                          # autocast off
        assert "float32" in fallback_reason(x, bn)                                                 # and norm_relu keeps its answer
        with _device_autocast(dt):
            for outputs in norm.OUTPUTS:
                assert reason(x, bn, outputs=outputs) is None
            for outputs in ("float", "both"):
                assert reason(x, bn, r32, None, outputs) is None and reason(x, bn, r16, rbn, outputs) is None
            assert "without a residual" in reason(x, bn, r32, None, "half") and "without a residual" in reason(x, bn, r16, rbn, "half")
            assert "outputs" in reason(x, bn, outputs="double")
            assert "float16 or bfloat16" in reason(_OnDevice(2, 8, 5, 7, dtype=f32), bn)            # a float32 x
            assert "autocast" in fallback_reason(_OnDevice(2, 8, 5, 7, dtype=f32), bn)             # ... which norm_relu turns away too
            assert "identity is float32" in reason(x, bn, r16)                                     # a half residual without residual_bn
            assert "downsample" in reason(x, bn, r32, rbn)                                         # a float32 residual with one
            assert "downsample" in reason(x, bn, _OnDevice(2, 8, 5, 7, dtype=other), rbn)
            assert "(B, C, H, W)" in reason(_OnDevice(8, 5, 7, dtype=dt), bn) and "(B, C, H, W)" in reason([1.0], bn)
            assert "device" in reason(torch.zeros(2, 8, 5, 7, dtype=dt), bn)                       # CPU tensors: the torch statements
            assert "empty" in reason(_OnDevice(0, 8, 5, 7, dtype=dt), bn)
            assert "contiguous" in reason(_OnDevice(2, 8, 5, 7, dtype=dt, contiguous=False), bn)
            assert "plane" in reason(_OnDevice(1, 8, 1 << 16, 1 << 15, dtype=dt), bn)
            for stock in (nn.BatchNorm2d(8).eval(), nn.BatchNorm2d(8), nn.GroupNorm(2, 8), nn.Identity()):
                assert "FrozenBatchNorm2d" in reason(x, stock)
                assert "residual_bn is not" in reason(x, bn, r16, stock)
            assert "channels" in reason(x, FrozenBatchNorm2d(6)) and "channels" in reason(x, bn, r16, FrozenBatchNorm2d(6))
            assert "float32 on" in reason(x, FrozenBatchNorm2d(8).double())
            assert "residual_bn without" in reason(x, bn, None, rbn)
            assert "shape" in reason(x, bn, _OnDevice(2, 8, 5, 6, dtype=f32)) and "shape" in reason(x, bn, 1.0)
            assert "residual is not on" in reason(x, bn, _OnDevice(2, 8, 5, 7, dtype=f32, device="meta"))
            assert "residual is not contiguous" in reason(x, bn, _OnDevice(2, 8, 5, 7, dtype=f32, contiguous=False))
        with _device_autocast(other):
            assert "autocast dtype" in reason(x, bn)                                               # autocast dtype != x.dtype
    assert not torch.is_autocast_enabled("cuda")


def test_the_speed_rule_is_a_constant_of_its_own(monkeypatch):
    from halo_amd import norm
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    reason = norm.autocast_fallback_reason
    f32 = torch.float32

    def operand(*shape, dtype=torch.float16, grad=True):
        return _OnDevice(*shape, dtype=dtype, grad=grad)
    with _device_autocast(torch.float16):
        assert sorted(norm.AUTOCAST_AUTOGRAD_MIN_ELEMENTS) == ["affine", "both", "float", "half"]
        for C in (128, 512, 1024):                                                   # the smallest sizes timed, and one element fewer
            bn, rbn = FrozenBatchNorm2d(C), FrozenBatchNorm2d(C)
            at, below = (2, C, 80, 160), (2, C, 80, 159)
            if C == 128:
                assert reason(operand(*at), bn, outputs="half") is None and "autograd" in reason(operand(*below), bn, outputs="half")
            if C == 512:
                assert reason(operand(*at), bn, operand(*at, dtype=f32)) is None and "autograd" in reason(operand(*below), bn, operand(*below, dtype=f32))
                assert reason(operand(*at), bn, operand(*at), rbn, "both") is None and "autograd" in reason(operand(*below), bn, operand(*below), rbn, "both")
                assert "autograd" in reason(operand(*at), bn, operand(*at, dtype=f32), None, "both")            # lost in one process
                assert "autograd" in reason(operand(*at, grad=False), bn, operand(*at, dtype=f32), None, "both")  # the residual wants one
            if C == 1024:
                assert reason(operand(*at), bn, operand(*at, dtype=f32), None, "both") is None
            assert reason(operand(*below, grad=False), bn, outputs="half") is None                              # no gradient: every size
            with torch.no_grad():
                assert reason(operand(*below), bn, outputs="half") is None
        monkeypatch.setattr(norm, "AUTOCAST_AUTOGRAD_MIN_ELEMENTS", {})                                      # a speed rule only
        assert reason(operand(2, 8, 5, 7), FrozenBatchNorm2d(8), outputs="both") is None
    assert "ac_fwd" in norm.launches and "ac_bwd" in norm.launches and list(norm.launches)[:3] == ["fwd", "bwd", "fork_bwd"]


@pytest.mark.parametrize("dt", HALVES, ids=["float16", "bfloat16"])
@pytest.mark.parametrize("outputs", ["float", "half", "both"])
def test_cpu_tensors_run_the_stock_statements(dt, outputs):
    from halo_amd import norm
    gen = torch.Generator().manual_seed(5)
    bn = _norm(4, 6)
    x = torch.randn(2, 4, 5, 6, generator=gen).to(dt)
    r = torch.randn(2, 4, 5, 6, generator=gen) if outputs != "half" else None
    before = dict(norm.launches)
    with torch.autocast("cpu", dtype=dt):
        got = norm.norm_relu_autocast(x, bn, r, None, outputs)
        want = norm.autocast_statement(x, bn, r, None, outputs)
    _, y32, y16 = A.forward(x, bn, r)
    want_ref = {"float": (y32,), "half": (y16,), "both": (y32, y16)}[outputs]
    got, want = (got, want) if outputs == "both" else ((got,), (want,))
    assert len(got) == len(want_ref)
    for g, w, ref in zip(got, want, want_ref):
        assert g.dtype == ref.dtype and torch.equal(g, w) and torch.equal(g, ref)
    assert norm.launches == before
    with pytest.raises(ValueError):
        norm.autocast_statement(x, bn, outputs="double")


def test_with_autocast_off_a_hooked_backbone_resolves_to_norm_relu_as_before(monkeypatch):
    from halo_amd import norm
    from halo_amd.hooks import fuse_residual_chains
    torch.manual_seed(7)
    plain = N.randomize_norms(N.backbone(), 8)
    hooked, pairs = N.hooked_copy(plain)
    assert pairs == 1 and fuse_residual_chains(hooked) == 1
    calls = []
    stock = norm.norm_relu

    def counted(x, bn, residual=None, residual_bn=None):
        calls.append((residual is not None, residual_bn is not None))
        return stock(x, bn, residual, residual_bn)

    def never(*a, **k):
        raise AssertionError("norm_relu_autocast was called with autocast off")
    monkeypatch.setattr(norm, "norm_relu", counted)
    monkeypatch.setattr(norm, "norm_relu_autocast", never)
    x = torch.randn(2, 3, 33, 47)
    before = dict(norm.launches)
    want, got = plain(x), hooked(x)
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want)
    assert len(calls) == 9 and calls.count((True, True)) == 2 and calls.count((True, False)) == 1       # three blocks, three norms each
    assert norm.launches == before
    # the same model under CPU autocast: not the device's autocast, so the stock statements as before, with the stock dtypes
    del calls[:]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        want, got = plain(x), hooked(x)
    assert all(torch.equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want) and len(calls) == 9


def test_integer_half_roundings_equal_numpy_and_torch(tmp_path):
    """halo_half_round.hpp, the float -> float16 / bfloat16 roundings of the kernels' one-element route, built for the host: every
    float32 whose low 13 bits sit on or next to a float16 tie (all 2^19 upper halves), every float32 on or next to a bfloat16 tie,
    random bit patterns, the float16 subnormal range, overflow, infinities and NaN -- numpy's float16 and torch's bfloat16 bits"""
    import shutil
    import subprocess
    import numpy as np
    from halo_amd import _build
    cxx = shutil.which("g++") or shutil.which("c++") or _build._hipcc()
    src = tmp_path / "round.cpp"
    src.write_text('#include <cstdio>\n#include <vector>\n#include "halo_half_round.hpp"\n'
                   'int main(int argc, char **argv)\n{\n'
                   '    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");\n    if (!in || !out) return 2;\n'
                   '    std::vector<float> f(1 << 16);\n    std::vector<unsigned short> h(2 << 16);\n    size_t n;\n'
                   '    while ((n = fread(f.data(), 4, f.size(), in)) > 0) {\n'
                   '        for (size_t i = 0; i < n; ++i) h[2 * i] = halo::f16_round_bits(f[i]), h[2 * i + 1] = halo::bf16_round_bits(f[i]);\n'
                   '        fwrite(h.data(), 2, 2 * n, out);\n    }\n    fclose(out);\n    return 0;\n}\n')
    exe = str(tmp_path / "round")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "halo_amd", "csrc"), str(src), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    rng = np.random.default_rng(0)
    upper = np.arange(1 << 19, dtype=np.uint32) << 13
    parts = [upper | low for low in (0x0000, 0x0001, 0x0fff, 0x1000, 0x1001, 0x1fff)]                       # float16 ties and neighbours
    upper = np.arange(1 << 16, dtype=np.uint32) << 16
    parts += [upper | low for low in (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)]                      # bfloat16 ties and neighbours
    parts.append(rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32))
    sub = rng.integers(0x31000000, 0x38800000, 1 << 20, dtype=np.uint64).astype(np.uint32)                  # 2^-29 .. 2^-14
    parts += [sub, sub | 0x80000000]
    parts.append(np.array([65504.0, 65519.99, 65520.0, 65536.0, 1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 2.0 ** -24, 2.0 ** -25,
                           1.5 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -149, 3.3895e38, 3.4e38], dtype=np.float32).view(np.uint32))
    bits = np.concatenate(parts)
    f = bits.view(np.float32)
    f.tofile(str(tmp_path / "in.bin"))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(str(tmp_path / "out.bin"), dtype=np.uint16).reshape(-1, 2)
    assert got.shape[0] == f.size
    nan = np.isnan(f)
    with np.errstate(over="ignore"):
        want16 = f.astype(np.float16).view(np.uint16)
    want_bf = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[~nan, 0], want16[~nan]) and np.array_equal(got[~nan, 1], want_bf[~nan])
    assert np.all(np.isnan(got[nan, 0].view(np.float16)))                                                   # a NaN stays a NaN, sign kept
    assert np.all((got[nan, 1] & 0x7f80) == 0x7f80) and np.all((got[nan, 1] & 0x007f) != 0)
    assert np.array_equal(got[nan, 0] & 0x8000, (bits[nan] >> 16).astype(np.uint16) & 0x8000)
    assert np.array_equal(got[nan, 1] & 0x8000, (bits[nan] >> 16).astype(np.uint16) & 0x8000)
