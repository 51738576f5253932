"""Every edge of halo_dwconv.hip's work split on the device, against float64 on the CPU.

The cases are tests/dwconv_cases.py's: the smallest planes at which a plane takes more than one 256-thread block, a chain more than
one 16-row segment at d > 1, an item an empty segment, a last block a handful of lanes -- on <4, true>, <4, false> and <1, false> --
and the degenerate planes (one row, one column, one pixel, W = 4, d beyond the plane).  tests/test_dwconv_geometry_host.py proves
under a model of dw_geom / dw_item that each case reaches what its name says, that tests/dwconv_ref.py holds a correct float32
chain, and that the operands put no element inside 4 x the forward bound of zero beyond the cap below.

The body is tests/test_gpu_dwconv.py::test_fixture's, through depthwise_bn_relu under autograd, with that module's derived bounds
(u = 2^-24): forward 15u (...), g_x 15u (...) with the device's mask, g_w 8u sum |gp| |x|; the mask equal to [pre_64 > 0] outside
the band |pre_64| <= bound, which may hold at most 1e-4 of the elements.  Nothing here is tuned.
"""
import numpy as np
import pytest
import torch

import dwconv_cases as K
import dwconv_ref as R

pytestmark = pytest.mark.gpu
ENTRIES = ("halo_dwconv3x3_affine_relu_fwd", "halo_dwconv3x3_affine_relu_bwd_data", "halo_dwconv3x3_affine_relu_bwd_weight")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_cases = {}


def case(name):
    """(the case, its float64 pre-activation, the forward bound): computed once on the CPU, shared, never written"""
    if name not in _cases:
        c = K.plain(name)
        _cases[name] = (c,) + R.forward(c)
    return _cases[name]


def offset_view(t):
    """the same values in storage that starts 4 bytes off a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 1, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def run(c, dev, view=lambda t: t):
    from halo_amd.dwconv import depthwise_bn_relu, fallback_reason
    conv, bn = R.modules(c, dev)
    x = view(torch.from_numpy(c["x"]).to(dev)).requires_grad_(True)
    assert fallback_reason(x, conv, bn) is None
    y = depthwise_bn_relu(x, conv, bn)
    assert type(y.grad_fn).__name__.startswith("_DepthwiseBnReluFn")
    gx, gw = torch.autograd.grad(y, [x, conv.weight], view(torch.from_numpy(c["g"]).to(dev)))
    return y.detach(), gx, gw


def ratio(err, bound):
    assert (err[bound == 0] == 0).all()                                          # exactly 0 where the bound is 0
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def check(name, got, which=("y", "g_x", "g_w")):
    """test_fixture's body for the quantities named, and the dead channel exactly 0 in each"""
    c, pre, bound = case(name)
    y, gx, gw = (t.cpu().numpy().astype(np.float64) for t in got)
    dead = c["C"] - 1
    band = np.abs(pre) <= bound
    print(name, "band fraction", float(band.mean()))
    assert band.mean() <= 1e-4
    mask = y > 0
    assert (mask == (pre > 0))[~band].all()
    if "y" in which:
        err = np.abs(y - np.maximum(pre, 0))
        print(name, "forward: max err / bound", ratio(err, bound))
        assert (err <= bound).all()
        assert (y[:, dead] == 0).all()
    if "g_x" in which:
        rx, bx = R.grad_x(c, mask)
        ex = np.abs(gx - rx)
        print(name, "g_x: max err / bound", ratio(ex, bx))
        assert (ex <= bx).all()
        assert (gx[:, dead] == 0).all()
    if "g_w" in which:
        rw, bw = R.grad_w(c, mask)
        ew = np.abs(gw - rw)
        print(name, "g_w: max err / bound", ratio(ew, bw))
        assert (ew <= bw).all()
        assert (gw[dead] == 0).all()


@pytest.mark.parametrize("name", list(K.PLAIN))
def test_case_against_float64(dev, name):
    check(name, run(case(name)[0], dev))


@pytest.mark.parametrize("name", list(K.PLAIN_OFFSET))
def test_offset_operands_run_the_one_column_route_with_the_same_bits(dev, name, monkeypatch):
    """x and g as contiguous views 4 bytes off a 16-byte boundary: the wrapper keeps them, so all three entries see an operand that
    fails dw_vec and run <1, false> with the block count of K.PLAIN_OFFSET (5, 5 and 4 against 2, 2 and 1).  y and g_x do not depend
    on the route: the aligned run's bits.  g_w's float64 partials are split differently: held to its 8u bound."""
    from halo_amd import _lib
    c = case(name)[0]
    aligned = run(c, dev)
    L = _lib.lib()
    seen = {}
    for entry in ENTRIES:
        real = getattr(L, entry)
        monkeypatch.setattr(L, entry, lambda *a, real=real, entry=entry: (seen.__setitem__(entry, [p.value % 16 for p in a[:3]]), real(*a))[1])
    got = run(c, dev, offset_view)
    # forward (x, w, scale), bwd_data (g, y, w), bwd_weight (g, y, x): an operand 4 bytes off in each
    assert seen[ENTRIES[0]][0] == 4 and seen[ENTRIES[1]][0] == 4 and seen[ENTRIES[2]][0] == 4 and seen[ENTRIES[2]][2] == 4, seen
    assert torch.equal(got[0], aligned[0]), "y"
    assert torch.equal(got[1], aligned[1]), "g_x"
    check(name, got, which=("g_w",))


def test_repeated_calls_and_a_side_stream_give_the_same_bits(dev):
    c = case("scalar_d4_two_blocks")[0]                                          # two blocks per plane, two segments, empty items
    a = run(c, dev)
    b = run(c, dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s = run(c, dev)
    side.synchronize()
    for t1, t2, t3 in zip(a, b, s):
        assert torch.equal(t1, t2) and torch.equal(t1, t3)

