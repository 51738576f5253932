"""The depthwise half under torch.autocast("cuda", dtype) on the device (halo_half_dwconv3x3_* of halo_dwconv.hip through
halo_amd.dwconv.depthwise_bn_relu_autocast and halo_amd.hooks.use_autocast_depthwise) against tests/dwconv_autocast_ref.py, the
statements in torch on the CPU with float64 sums.

Exact tier: small-integer operands, power-of-two scales, integer shifts -- every sum is exact whatever its order, so y16 and g_x are
torch.equal to the restatement AND to the stock statements under autocast on the device, g_w to the restatement.  Over every shape
of dwconv_cases.PLAIN (each edge of the work split, both routes) and the PLAIN_OFFSET views (the one-column route at W % 4 == 0).
Random tier: every element the float64 evaluation does not excuse equals the restatement, an excused one either of its candidates;
the backward is evaluated with the device's own y16 as the gate."""
import pytest
import torch
import torch.nn as nn

import dwconv_autocast_ref as R
import dwconv_cases as K
from euclid_head_standin import Block, EuclidHead, frozen

pytestmark = pytest.mark.gpu
HALVES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
XDTYPES = ("x32", "x16")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture()
def deterministic_convolutions():
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _at_offset(t, nbytes):
    """t's values in a contiguous tensor whose storage starts `nbytes` into its buffer"""
    off = nbytes // t.element_size()
    if off == 0:
        return t
    buf = torch.empty(t.numel() + off, device=t.device, dtype=t.dtype)
    out = buf[off:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == nbytes
    return out


def _device_run(fn, x, g16, conv, bn, dt, want=(True, True)):
    """(y16, g_x, g_w) of fn(x, conv, bn) under autocast on the device, the gradients that `want` asks for"""
    xs = x.detach().requires_grad_(want[0])                  # shares x's storage: an offset view stays one
    conv.weight.requires_grad_(want[1])
    with torch.autocast("cuda", dtype=dt):
        y16 = fn(xs, conv, bn)
    leaves = ([xs] if want[0] else []) + ([conv.weight] if want[1] else [])
    grads = list(torch.autograd.grad(y16, leaves, g16)) if leaves else []
    gx = grads.pop(0) if want[0] else None
    gw = grads.pop(0) if want[1] else None
    return y16.detach(), gx, gw


def _operands(case, dt, half_x, dev, offset=0):
    x, w, g, scale, shift = case
    x = x.to(dt) if half_x else x
    g16 = g.to(dt)
    return x, g16, _at_offset(x.to(dev), offset), _at_offset(g16.to(dev), offset)


@pytest.mark.parametrize("dname", list(HALVES))
@pytest.mark.parametrize("name", list(K.PLAIN) + [n + "@offset" for n in K.PLAIN_OFFSET])
def test_exact_tier_equals_the_restatement_and_the_stock_statements(name, dname, dev, deterministic_convolutions):
    from halo_amd import dwconv
    dt, offset = HALVES[dname], 4 if name.endswith("@offset") else 0
    name = name.split("@")[0]
    shape = K.PLAIN[name][0]
    d = shape[4]
    case = R.exact_case(100 + list(K.PLAIN).index(name), *shape)
    conv, bn = R.modules(case[1], case[3], case[4], d, dev)
    for half_x in (False, True):
        x, g16, xd, gd = _operands(case, dt, half_x, dev, offset)
        f = R.forward(x, case[1], case[3], case[4], d, dt)
        b = R.backward(g16, f.y16, x, case[1], case[3], d, dt)
        assert float(f.c16.float().abs().max()) <= 72 and torch.equal(f.c16.double(), f.sum)           # exact, below 256
        before = dict(dwconv.autocast_launches)
        with torch.autocast("cuda", dtype=dt):
            assert dwconv.autocast_fallback_reason(xd, conv, bn) is None
        y16, gx, gw = _device_run(dwconv.depthwise_bn_relu_autocast, xd, gd, conv, bn, dt)
        assert dwconv.autocast_launches == {k: v + 1 for k, v in before.items()}
        assert y16.dtype == dt and gx.dtype == x.dtype and gw.dtype == torch.float32
        assert torch.equal(y16.cpu(), f.y16), (name, dname, half_x)
        assert torch.equal(gx.cpu(), b.g_x), (name, dname, half_x)
        assert torch.equal(gw.cpu(), b.g_w), (name, dname, half_x)
        sy, sgx, _ = _device_run(dwconv.autocast_statement, xd, gd, conv, bn, dt)
        assert sy.dtype == dt and sgx.dtype == x.dtype and torch.equal(y16, sy) and torch.equal(gx, sgx), (name, dname, half_x)
        assert dwconv.autocast_launches == {k: v + 1 for k, v in before.items()}                       # the stock side launched none
    if shape[2] * shape[3] > 100:
        assert 0 < int((f.y16 > 0).sum()) < f.y16.numel() and float(b.g_x.float().abs().sum()) > 0


@pytest.mark.parametrize("xname", XDTYPES)
@pytest.mark.parametrize("dname", list(HALVES))
@pytest.mark.parametrize("name", list(R.RANDOM_TIER))
def test_random_tier_every_element_not_excused_equals_the_restatement(name, dname, xname, dev):
    from halo_amd import dwconv
    dt = HALVES[dname]
    shape = K.PLAIN[name][0]
    d = shape[4]
    case = R.random_case(R.RANDOM_TIER[name], *shape)
    conv, bn = R.modules(case[1], case[3], case[4], d, dev)
    x, g16, xd, gd = _operands(case, dt, xname == "x16", dev)
    y16, gx, gw = _device_run(dwconv.depthwise_bn_relu_autocast, xd, gd, conv, bn, dt)
    f = R.forward(x, case[1], case[3], case[4], d, dt)
    y16 = y16.cpu()
    wrong = ~(R.same(y16, f.y16) | (f.excused & R.same(y16, f.y16_alt)))
    print("%s %s %s: y16 excused %d of %d, taken %d, wrong %d" % (name, dname, xname, int(f.excused.sum()), y16.numel(),
                                                                 int((~R.same(y16, f.y16)).sum()), int(wrong.sum())))
    assert not bool(wrong.any())
    b = R.backward(g16, y16, x, case[1], case[3], d, dt)                               # the device's own y16 as the gate
    gx, gw = gx.cpu(), gw.cpu()
    print("    g_x excused %d, taken %d; g_w excused %d, taken %d" % (int(b.gx_excused.sum()), int((~R.same(gx, b.g_x)).sum()),
                                                                     int(b.gw_excused.sum()), int((~R.same(gw, b.g_w)).sum())))
    assert gx.dtype == x.dtype and R.matches(gx, b.g_x, b.g_x_alt, b.gx_excused)
    assert gw.dtype == torch.float32 and R.matches(gw, b.g_w, b.g_w_alt, b.gw_excused)
    assert float(b.gx_excused.float().mean()) <= 0.02 and float(f.excused.float().mean()) <= 0.01       # the check is not hollow


@pytest.mark.parametrize("xname", XDTYPES)
@pytest.mark.parametrize("dname", list(HALVES))
def test_nan_and_infinities_in_x(dname, xname, dev):
    from halo_amd import dwconv
    dt = HALVES[dname]
    shape = K.PLAIN["vec_d3_two_blocks"][0]
    case = list(R.exact_case(7, *shape))
    x = case[0]
    x[0, 0, 5, 9], x[0, 1, 20, 100], x[1, 2, 49, 175], x[1, 0, 0, 0], x[1, 1, 30, 3] = float("nan"), float("inf"), float("-inf"), float("inf"), float("nan")
    conv, bn = R.modules(case[1], case[3], case[4], shape[4], dev)
    x, g16, xd, gd = _operands(case, dt, xname == "x16", dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        y16 = dwconv.depthwise_bn_relu_autocast(xd, conv, bn).cpu()
    f = R.forward(x, case[1], case[3], case[4], shape[4], dt)
    assert bool(R.same(y16, f.y16).all())
    assert int(torch.isnan(y16).sum()) > 0 and int(torch.isinf(y16).sum()) > 0


@pytest.mark.parametrize("xname", XDTYPES)
def test_a_float16_sum_past_65504_is_an_infinity_on_both_sides(xname, dev):
    from halo_amd import dwconv
    dt = torch.float16
    B, C, H, W, d = 1, 3, 9, 12, 2
    x = torch.full((B, C, H, W), 8000.0)                                             # a float16 value; nine of them are 72 000, four 32 000
    w = torch.ones(C, 1, 3, 3)
    scale, shift = torch.tensor([1.0, 0.5, -1.0]), torch.zeros(C)
    conv, bn = R.modules(w, scale, shift, d, dev)
    xd = (x.to(dt) if xname == "x16" else x).to(dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        y16 = dwconv.depthwise_bn_relu_autocast(xd, conv, bn).cpu()
        stock = dwconv.autocast_statement(xd, conv, bn).cpu()
    f = R.forward(xd.cpu(), w, scale, shift, d, dt)
    assert torch.equal(y16, f.y16) and torch.equal(y16, stock)
    assert bool(torch.isinf(y16[:, :2, 4, 6]).all()) and bool((y16[:, 2] == 0).all()) and bool(torch.isfinite(y16[:, 0, 0, 0]).all())


def test_launches_follow_needs_input_grad(dev):
    from halo_amd import dwconv
    dt = torch.bfloat16
    shape = K.PLAIN["d6_two_segments"][0]
    case = R.exact_case(3, *shape)
    conv, bn = R.modules(case[1], case[3], case[4], shape[4], dev)
    x, g16, xd, gd = _operands(case, dt, False, dev)
    ref = _device_run(dwconv.depthwise_bn_relu_autocast, xd, gd, conv, bn, dt)
    for want, add in (((True, False), (1, 1, 0)), ((False, True), (1, 0, 1)), ((True, True), (1, 1, 1))):
        before = dict(dwconv.autocast_launches)
        y16, gx, gw = _device_run(dwconv.depthwise_bn_relu_autocast, xd, gd, conv, bn, dt, want)
        assert [dwconv.autocast_launches[k] - before[k] for k in ("fwd", "bwd_data", "bwd_weight")] == list(add)
        assert torch.equal(y16, ref[0]) and (gx is None or torch.equal(gx, ref[1])) and (gw is None or torch.equal(gw, ref[2]))
    before = dict(dwconv.autocast_launches)
    conv.weight.requires_grad_(False)
    with torch.autocast("cuda", dtype=dt):
        y = dwconv.depthwise_bn_relu_autocast(xd, conv, bn)
    assert not y.requires_grad and torch.equal(y, ref[0])
    assert [dwconv.autocast_launches[k] - before[k] for k in ("fwd", "bwd_data", "bwd_weight")] == [1, 0, 0]


@pytest.mark.parametrize("dname", list(HALVES))
def test_repeated_and_side_stream_calls_return_equal_bits(dname, dev):
    from halo_amd import dwconv
    dt = HALVES[dname]
    shape = K.PLAIN["vec_d1_five_lane_block"][0]
    case = R.random_case(9, *shape)
    conv, bn = R.modules(case[1], case[3], case[4], shape[4], dev)
    x, g16, xd, gd = _operands(case, dt, False, dev)
    first = _device_run(dwconv.depthwise_bn_relu_autocast, xd, gd, conv, bn, dt)
    again = _device_run(dwconv.depthwise_bn_relu_autocast, xd, gd, conv, bn, dt)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = _device_run(dwconv.depthwise_bn_relu_autocast, xd, gd, conv, bn, dt)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("dname", list(HALVES))
def test_outside_the_envelope_the_stock_statements_run(dname, dev, deterministic_convolutions):
    from halo_amd import dwconv
    dt = HALVES[dname]
    shape = (2, 3, 17, 20, 2)
    case = R.exact_case(5, *shape)
    conv, bn = R.modules(case[1], case[3], case[4], 2, dev)
    x, g16, xd, gd = _operands(case, dt, False, dev)
    before = dict(dwconv.autocast_launches)
    strided = torch.empty(2, 3, 17, 40, device=dev)[..., ::2].copy_(xd)                     # not contiguous
    stock_bn = nn.BatchNorm2d(3).to(dev).eval().requires_grad_(False)                       # the library's batch norm on a half input
    with torch.autocast("cuda", dtype=dt):
        for xin, norm, word in ((strided, bn, "contiguous"), (xd, stock_bn, "FrozenBatchNorm2d"), (xd.double(), bn, "neither float32")):
            assert word in dwconv.autocast_fallback_reason(xin, conv, norm)
            if xin.dtype == torch.float64:
                continue
            got = dwconv.depthwise_bn_relu_autocast(xin, conv, norm)
            want = dwconv.autocast_statement(xin, conv, norm)
            assert got.dtype == want.dtype == dt and torch.equal(got, want)
    got = dwconv.depthwise_bn_relu_autocast(xd, conv, bn)                                   # autocast off: the float32 statements
    assert got.dtype == torch.float32 and torch.equal(got, dwconv.torch_statement(xd, conv, bn))
    assert dwconv.autocast_launches == before


# ---------------------------------------------------------------- the hooks on a stand-in v3+ head
class _Head(EuclidHead):
    """a stand-in v3+ head at channels 16 / 8 / 8 with the reference's three dilated branches and two decoder blocks"""

    def __init__(self, block):
        super().__init__(block=block, old=True, top=16, mid=8, low=8, short=6)
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(16, 8, 1, bias=False), frozen(8, 1), nn.ReLU(inplace=True))] + [
            block(16, 8, d) for d in (6, 12, 18)])
        self.bottleneck = nn.Sequential(nn.Conv2d(5 * 8, 8, 3, padding=1, bias=False), frozen(8, 3), nn.ReLU(inplace=True))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data = torch.randn(m.weight.shape) * (2.0 / m.weight[0].numel() ** 0.5)


def _heads(dev, *block_classes):
    from halo_amd.core.models.classifier import v3plus_forward
    Head = type("Head", (_Head,), {"forward": v3plus_forward})
    torch.manual_seed(21)
    with torch.no_grad():
        heads = [Head(b) for b in block_classes]
    for h in heads[1:]:
        h.load_state_dict(heads[0].state_dict())
    gen = torch.Generator().manual_seed(22)
    feats = {"low": torch.randn(2, 8, 12, 16, generator=gen).to(dev), "out": torch.randn(2, 16, 6, 8, generator=gen).to(dev)}
    return [h.to(dev).eval() for h in heads], feats


@pytest.mark.parametrize("dname", list(HALVES))
def test_a_marked_head_under_autocast(dname, dev, deterministic_convolutions):
    """five forward launches; the unmarked head's dtypes; and outputs no further from the unmarked head's under autocast than
    those are from that head's own float32 run"""
    from halo_amd import dwconv
    from halo_amd.hooks import use_autocast_depthwise, use_fused_depthwise
    dt = HALVES[dname]
    Plain = use_fused_depthwise(type("Plain", (Block,), {}))
    Marked = use_autocast_depthwise(use_fused_depthwise(type("Marked", (Block,), {})))
    (plain, marked), feats = _heads(dev, Plain, Marked)
    with torch.no_grad():
        full = plain(feats)
        before = dict(dwconv.autocast_launches)
        with torch.autocast("cuda", dtype=dt):
            stock = plain(feats)
            assert dwconv.autocast_launches == before
            got = marked(feats)
        assert dwconv.autocast_launches["fwd"] == before["fwd"] + 5 and dwconv.autocast_launches["bwd_data"] == before["bwd_data"]
        off = marked(feats)                                                              # autocast off: what it did before
        assert dwconv.autocast_launches["fwd"] == before["fwd"] + 5
    for name, g, s, f, o in zip(("out", "decoder_out"), got, stock, full, off):
        assert g.dtype == s.dtype and g.shape == s.shape and torch.equal(o, f), name
        ours, theirs = float((g.float() - s.float()).abs().max()), float((s.float() - f.float()).abs().max())
        print("%s %s: marked against unmarked under autocast %.4g, unmarked autocast against float32 %.4g" % (dname, name, ours, theirs))
        assert bool(torch.isfinite(g).all()) and float(g.float().std()) > 0 and ours <= theirs, name
    # forward + backward: five data and five weight launches, finite gradients of the unmarked head's dtypes
    top = feats["out"].clone().requires_grad_(True)
    before = dict(dwconv.autocast_launches)
    with torch.autocast("cuda", dtype=dt):
        out, _ = marked({"low": feats["low"], "out": top})
    params = [p for p in marked.parameters() if p.requires_grad]
    grads = torch.autograd.grad(out.float().square().mean(), [top] + params)
    assert [dwconv.autocast_launches[k] - before[k] for k in ("fwd", "bwd_data", "bwd_weight")] == [5, 5, 5]
    assert all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads) and float(grads[0].abs().sum()) > 0


@pytest.mark.parametrize("dname", list(HALVES))
def test_a_head_with_only_the_pointwise_norm_marked_equals_the_unmarked_one(dname, dev, deterministic_convolutions, monkeypatch):
    from halo_amd import dwconv, norm
    from halo_amd.hooks import use_fused_pointwise_norm
    dt = HALVES[dname]
    Tail = use_fused_pointwise_norm(type("Tail", (Block,), {}))
    (plain, tail), feats = _heads(dev, Block, Tail)
    before, dw_before = dict(norm.launches), dict(dwconv.autocast_launches)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        want, got = plain(feats), tail(feats)
    assert norm.launches["ac_fwd"] == before["ac_fwd"] + 5 and dwconv.autocast_launches == dw_before
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
    monkeypatch.setattr(norm, "AUTOCAST_AUTOGRAD_MIN_ELEMENTS", {})                      # a speed rule only: serve the small maps with a gradient too
    top = feats["out"].clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dt):
        want, got = plain({"low": feats["low"], "out": top}), tail({"low": feats["low"], "out": top})
    assert norm.launches["ac_fwd"] == before["ac_fwd"] + 10
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
