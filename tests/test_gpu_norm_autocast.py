"""halo_amd.norm.norm_relu_autocast (halo_norm_autocast.hip) and the hooks under torch.autocast("cuda", dtype) against the stock torch
chain and autograd on the same device, for float16 and bfloat16.  The kernels run the chain's own operations with the chain's
roundings and autocast's cast, so every comparison is norm_ref.same_bits (NaN positions equal, everything else torch.equal).  Whole
models are held to the difference between two runs of the unhooked model, gradient by gradient; with the library's deterministic
convolution algorithms, which those tests ask for, that difference is zero and the comparison is torch.equal too.

The shapes, with the constants of halo_norm_autocast.hip (256 lanes; the wide route takes groups of 8 elements, 2 per lane, a chunk
of 512 groups = 4096 elements; the one-element route 4 per lane, a chunk of 1024 elements):"""
import pytest
import torch
import torch.nn as nn

import norm_ref as N
from test_gpu_norm_relu import _norm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = {
    "short_plane": (2, 3, 5, 7),                 # HW = 35: the one-element route, a plane shorter than a wave
    "wide_partial_block": (1, 2, 8, 12),         # HW = 96: the wide route, 12 groups of eight in one partial workgroup
    "multiple_of_four_only": (1, 2, 37, 52),     # HW = 1924 = 4 * 481, no multiple of 8: the one-element route, a whole chunk and 900 more
    "single_whole_chunk": (2, 3, 13, 79),        # HW = 1027: a whole chunk of single elements and three more
    "wide_several_chunks": (2, 5, 80, 160),      # HW = 12800: the wide route, three full chunks of 512 groups and a ragged one of 64
    "unaligned_view": (1, 2, 8, 12),             # a storage offset of one element: half operands 2 bytes off, float32 operands 4 bytes
    "unaligned_chunks": (1, 2, 33, 128),         # the same offset over HW = 4224: four whole chunks of single elements, a ragged fifth
    "single_random_scales": (2, 6, 41, 61),      # HW = 2501: the one-element route over channels whose scales are no powers of two, so
}                                                # that products round in float32 before they round to half (the C = 5 shape: the wide route)
HALVES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
RESIDUALS = ("none", "plain", "affine")                    # no residual; a float32 identity; a half residual with a residual_bn
VARIANTS = [("none", "float"), ("none", "half"), ("plain", "float"), ("plain", "both"), ("affine", "float"), ("affine", "both")]
MODES = {"float": ("g32",), "half": ("g16",), "both": ("g32", "g16", "g32+g16")}       # where gradients arrive


@pytest.fixture(autouse=True)
def every_size_served(monkeypatch):
    """halo_amd.norm leaves small tensors that need a gradient to the stock statements because they are faster there (a speed
    rule: the bits are the same); these tests are about the kernels and the hooks, so they switch the rule off"""
    from halo_amd import norm
    monkeypatch.setattr(norm, "AUTOCAST_AUTOGRAD_MIN_ELEMENTS", {})


def _ac_norm(C, seed, dt):
    """tests/test_gpu_norm_relu.py's norm (channel 0: scale -2, shift +1, x = 0.5 gives pre == 0) with the last channel scale
    2^-20, shift 0: x = 2^-10 gives y32 = 2^-30 > 0, a float16 zero.  bfloat16 has float32's exponent range: scale 2^-100 and
    x = 2^-40 give a float32 subnormal, held to whatever the chain makes of it on the device"""
    bn = _norm(C, seed)
    with torch.no_grad():
        bn.weight[C - 1], bn.running_var[C - 1], bn.bias[C - 1], bn.running_mean[C - 1] = 2.0 ** (-20 if dt == torch.float16 else -100), 1.0, 0.0, 0.0
    return bn


def _tiny(dt):
    return 2.0 ** (-10 if dt == torch.float16 else -40)


def _place(flat, shape, dtype, unaligned):
    """`flat` as a contiguous tensor of `dtype` on the device, its storage one element off where `unaligned`"""
    n = flat.numel()
    if unaligned:
        base = torch.empty(n + 1, device=DEV, dtype=dtype)
        base[1:].copy_(flat)
        out = base[1:].view(shape)
        assert out.is_contiguous() and out.data_ptr() % 16 == base.element_size()
        return out
    return flat.view(shape).to(device=DEV, dtype=dtype)


def _values(shape, gen, special):
    n = 1
    for s in shape:
        n *= s
    flat = torch.randn(n, generator=gen)
    if special:
        k = min(n, 28)
        flat[torch.randperm(n, generator=gen)[:k]] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 0.5, 0.5] * 4)[:k]
    return flat


@pytest.fixture(scope="module")
def cases():
    """per (shape name, dtype name, residual): operands, the stock chain's y32 and y16 under autocast, and autograd's gradients for
    a gradient arriving at y32, at y16 and at both; computed once and left unchanged"""
    out = {}
    for si, (name, shape) in enumerate(SHAPES.items()):
        for di, (dname, dt) in enumerate(HALVES.items()):
            for vi, res in enumerate(RESIDUALS):
                gen = torch.Generator().manual_seed(1000 * si + 10 * vi + di)
                un = name.startswith("unaligned")
                C = shape[1]
                bn = _ac_norm(C, 7 + si, dt)
                rbn = _ac_norm(C, 70 + si, dt) if res == "affine" else None
                xv = _values(shape, gen, True).view(shape)
                rv = _values(shape, gen, True).view(shape)
                # channel 0, first row: s == 0 exactly (x = 0.5 gives pre == 0; the identity there is 0, or 0.5 under channel 0's norm)
                xv[0, 0, 0, :3], rv[0, 0, 0, :3] = 0.5, (0.5 if res == "affine" else 0.0)
                xv[0, 0, 1, 0], xv[0, 0, 1, 1] = -0.0, float("nan")
                xv[0, 0, 2, :2], rv[0, 0, 2, :2] = -40000.0, 0.0                                 # pre = 80001 > 65504: a float16 inf
                xv[0, C - 1, 0, :3], rv[0, C - 1, 0, :3] = _tiny(dt), 0.0                        # the last channel: a tiny positive y32
                x = _place(xv.reshape(-1), shape, dt, un)
                r = None if res == "none" else _place(rv.reshape(-1), shape, torch.float32 if res == "plain" else dt, un)
                g32 = _values(shape, gen, False).view(shape)
                g16 = _values(shape, gen, False).view(shape)
                g32[torch.rand(shape, generator=gen) < 0.2] = 0.0
                g16[torch.rand(shape, generator=gen) < 0.2] = 0.0
                g32[0, C - 1, 0, :3], g16[0, C - 1, 0, :3] = 1.0, 1.0
                g32, g16 = _place(g32.reshape(-1), shape, torch.float32, un), _place(g16.reshape(-1), shape, dt, un)
                xs = x.clone().requires_grad_(True)
                rs = r.clone().requires_grad_(True) if r is not None else None
                ins = [xs] if r is None else [xs, rs]
                grads = {}
                with torch.autocast("cuda", dtype=dt):
                    y32 = N.stock_chain(xs, bn, rs, rbn)
                    y16 = y32.to(dt)                                   # autocast's cast in front of the next convolution
                    grads["g32"] = torch.autograd.grad([y32], ins, [g32], retain_graph=True)
                    grads["g16"] = torch.autograd.grad([y16], ins, [g16], retain_graph=True)
                    grads["g32+g16"] = torch.autograd.grad([y32, y16], ins, [g32, g16])
                y32, y16 = y32.detach(), y16.detach()
                assert y32.dtype == torch.float32 and y16.dtype == dt and grads["g16"][0].dtype == dt
                assert r is None or grads["g32"][1].dtype == r.dtype
                # the stock result really holds the cases the comparison is about
                assert float(y32[0, 0, 0, :3].abs().max()) == 0 and bool(y32.isnan().any()) and bool(y32.isinf().any())
                assert bool((y32[0, 0, 2, :2] > 65504).all())
                if dt == torch.float16:
                    assert bool(y16[0, 0, 2, :2].isinf().all())
                    assert bool((y32[0, C - 1, 0, :3] > 0).all()) and bool((y16[0, C - 1, 0, :3] == 0).all())     # a half zero ...
                    assert bool((grads["g16"][0][0, C - 1, 0, :3] != 0).all())                                      # ... that lets g through
                else:
                    print("%s %s: bfloat16 y32 at scale 2^-100, x = 2^-40: %r" % (name, res, y32[0, C - 1, 0, :3].tolist()))
                assert bool((y32 == 0).any()) and bool((y32 > 0).any())
                out[(name, dname, res)] = dict(bn=bn, rbn=rbn, x=x, r=r, g32=g32, g16=g16, y32=y32, y16=y16, grads=grads)
    return out


def _why(got, want):
    """what differs, for an assertion's message"""
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    idx = bad.nonzero()[:4]
    return "%d of %d elements differ; first at %s: got %s, want %s" % (int(bad.sum()), got.numel(), idx.tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _leaves(c):
    x = c["x"].detach().requires_grad_(True)                 # the same storage and offset; the shared case stays as it is
    r = c["r"].detach().requires_grad_(True) if c["r"] is not None else None
    return x, r


def _outs(result, outputs):
    """(y32, y16) of a norm_relu_autocast result; None for the one not returned"""
    return result if outputs == "both" else (result, None) if outputs == "float" else (None, result)


def _backward(y32, y16, ins, c, mode):
    pairs = [(y, c[k]) for y, k in ((y32, "g32"), (y16, "g16")) if k in mode.split("+")]
    return torch.autograd.grad([p[0] for p in pairs], ins, [p[1] for p in pairs])


@pytest.mark.parametrize("variant", VARIANTS, ids=["%s-%s" % v for v in VARIANTS])
@pytest.mark.parametrize("dname", list(HALVES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_operator_equals_the_stock_chain(cases, name, dname, variant):
    from halo_amd import norm
    res, outputs = variant
    dt, c = HALVES[dname], cases[(name, dname, res)]
    x0 = c["x"].clone()
    with torch.autocast("cuda", dtype=dt):
        assert norm.autocast_fallback_reason(c["x"], c["bn"], c["r"], c["rbn"], outputs) is None
        for mode in MODES[outputs]:
            x, r = _leaves(c)
            ins = [x] if r is None else [x, r]
            before = dict(norm.launches)
            y32, y16 = _outs(norm.norm_relu_autocast(x, c["bn"], r, c["rbn"], outputs), outputs)
            grads = _backward(y32, y16, ins, c, mode)
            assert norm.launches == dict(before, ac_fwd=before["ac_fwd"] + 1, ac_bwd=before["ac_bwd"] + 1), mode     # one pass each way
            if y32 is not None:
                assert y32.dtype == torch.float32 and N.same_bits(y32.detach(), c["y32"]), "y32"
            if y16 is not None:
                assert y16.dtype == dt and N.same_bits(y16.detach(), c["y16"]), "y16"
            want = c["grads"][mode]
            assert grads[0].dtype == dt and N.same_bits(grads[0], want[0]), "g_x, %s: %s" % (mode, _why(grads[0], want[0]))
            if r is not None:
                assert grads[1].dtype == r.dtype and N.same_bits(grads[1], want[1]), "g_r, %s: %s" % (mode, _why(grads[1], want[1]))
        stock = _outs(norm.autocast_statement(c["x"], c["bn"], c["r"], c["rbn"], outputs), outputs)       # the fallback is the oracle
        for got, key in zip(stock, ("y32", "y16")):
            assert got is None or N.same_bits(got, c[key])
    assert N.same_bits(c["x"], x0)                                                                      # out of place


@pytest.mark.parametrize("dname", list(HALVES))
def test_the_half_output_allocates_no_float32_activation(cases, dname):
    from halo_amd import norm
    dt, c = HALVES[dname], cases[("wide_several_chunks", dname, "none")]
    n = c["x"].numel()
    with torch.autocast("cuda", dtype=dt):
        for grad in (False, True):
            x = c["x"].detach().requires_grad_(grad)
            norm.norm_relu_autocast(x, c["bn"], outputs="half")                      # scale and shift are cached from here on
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(DEV)
            base = torch.cuda.memory_allocated(DEV)
            y16 = norm.norm_relu_autocast(x, c["bn"], outputs="half")
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(DEV) - base
            assert 2 * n <= peak < 4 * n, "%d bytes allocated for %d half elements" % (peak, n)       # y16 alone: no float32 tensor of n elements
            assert N.same_bits(y16.detach(), c["y16"])
            # "float" allocates the float32 result, for comparison
            torch.cuda.reset_peak_memory_stats(DEV)
            base = torch.cuda.memory_allocated(DEV)
            y32 = norm.norm_relu_autocast(x, c["bn"], outputs="float")
            torch.cuda.synchronize()
            assert torch.cuda.max_memory_allocated(DEV) - base >= 4 * n and y32.dtype == torch.float32


@pytest.mark.parametrize("res", ["plain", "affine"])
@pytest.mark.parametrize("dname", list(HALVES))
def test_only_the_gradients_asked_for_are_launched(cases, dname, res):
    from halo_amd import norm
    dt, c = HALVES[dname], cases[("multiple_of_four_only", dname, res)]
    want = c["grads"]["g32+g16"]
    with torch.autocast("cuda", dtype=dt):
        x, r = c["x"].clone(), c["r"].clone()
        before = dict(norm.launches)
        y32, y16 = norm.norm_relu_autocast(x.requires_grad_(True), c["bn"], r, c["rbn"], "both")           # only x
        (gx,) = torch.autograd.grad([y32, y16], [x], [c["g32"], c["g16"]])
        assert N.same_bits(gx, want[0]) and norm.launches["ac_bwd"] == before["ac_bwd"] + 1
        x = x.detach()
        y32, y16 = norm.norm_relu_autocast(x, c["bn"], r.requires_grad_(True), c["rbn"], "both")           # only the residual
        (gr,) = torch.autograd.grad([y32, y16], [r], [c["g32"], c["g16"]])
        assert N.same_bits(gr, want[1]) and norm.launches["ac_bwd"] == before["ac_bwd"] + 2
        y32, y16 = norm.norm_relu_autocast(x, c["bn"], r.detach(), c["rbn"], "both")                       # neither: no node
        assert y32.grad_fn is None and y16.grad_fn is None and N.same_bits(y32, c["y32"]) and N.same_bits(y16, c["y16"])
        w = torch.ones((), device=DEV, requires_grad=True)
        (y32 * w).sum().backward()                                                                         # a backward that reaches y32 launches nothing here
        with torch.no_grad():
            y = norm.norm_relu_autocast(x.requires_grad_(True), c["bn"], r, c["rbn"], "float")
        assert y.grad_fn is None and N.same_bits(y, c["y32"])
    assert norm.launches == dict(before, ac_fwd=before["ac_fwd"] + 4, ac_bwd=before["ac_bwd"] + 2)


@pytest.mark.parametrize("dname", list(HALVES))
def test_repeated_and_side_stream_calls_return_equal_bits(cases, dname):
    from halo_amd.norm import norm_relu_autocast
    dt, c = HALVES[dname], cases[("wide_several_chunks", dname, "affine")]
    want = c["grads"]["g32+g16"]
    x, r = c["x"].clone().requires_grad_(True), c["r"].clone().requires_grad_(True)

    def run():
        with torch.autocast("cuda", dtype=dt):
            y32, y16 = norm_relu_autocast(x, c["bn"], r, c["rbn"], "both")
            return (y32.detach(), y16.detach()) + torch.autograd.grad([y32, y16], [x, r], [c["g32"], c["g16"]])
    runs = [run() for _ in range(3)]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        runs.append(run())
    side.synchronize()
    for got in runs:
        assert N.same_bits(got[0], c["y32"]) and N.same_bits(got[1], c["y16"]) and N.same_bits(got[2], want[0]) and N.same_bits(got[3], want[1])


@pytest.mark.parametrize("dname", list(HALVES))
def test_outside_the_envelope_the_stock_statements_run(cases, dname):
    from halo_amd import norm
    dt, c = HALVES[dname], cases[("wide_partial_block", dname, "none")]
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    before = dict(norm.launches)

    def check(x, bn, word):
        for outputs in norm.OUTPUTS:
            assert word in norm.autocast_fallback_reason(x, bn, outputs=outputs)
            got = _outs(norm.norm_relu_autocast(x, bn, outputs=outputs), outputs)
            want = _outs(norm.autocast_statement(x, bn, outputs=outputs), outputs)
            for g, w in zip(got, want):
                assert (g is None and w is None) or (g.dtype == w.dtype and N.same_bits(g, w))
    with torch.autocast("cuda", dtype=other):
        check(c["x"], c["bn"], "autocast dtype")                                     # an autocast dtype that is not x's
    with torch.autocast("cuda", dtype=dt):
        check(c["x"].transpose(2, 3), c["bn"], "contiguous")                         # a non-contiguous x
        bn = nn.BatchNorm2d(c["x"].shape[1]).to(DEV).eval()                          # eval-mode nn.BatchNorm2d: one ATen kernel, another order
        with torch.no_grad():
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
        check(c["x"], bn, "FrozenBatchNorm2d")
    check(c["x"], c["bn"], "not enabled")                                            # autocast off
    assert norm.launches == before


# ---------------------------------------------------------------- the hooks under autocast

@pytest.fixture
def deterministic_convolutions(monkeypatch):
    """tests/test_gpu_norm_relu.py's: with the library's deterministic algorithms two runs of the unhooked model agree, the bound is
    zero and the hooked model must be torch.equal"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


def _hooked(model):
    """use_fused_frozen_norm + fuse_norm_relu_pairs (norm_ref.hooked_copy) + fuse_residual_chains on a deep copy"""
    from halo_amd.hooks import fuse_residual_chains
    twin, pairs = N.hooked_copy(model)
    return twin, pairs, fuse_residual_chains(twin)


def _g_of(outs):
    return [torch.randn(o.shape, generator=torch.Generator().manual_seed(31 + i)).to(device=DEV, dtype=o.dtype) for i, o in enumerate(outs)]


def _held_to_the_unhooked_spread(plain, hooked, x, dt, label):
    """under autocast: outputs torch.equal and of the stock model's dtypes; each gradient of the hooked model differs from the
    unhooked model's by at most the largest difference between two runs of the unhooked model (zero, i.e. torch.equal, when those
    agree)"""
    with torch.autocast("cuda", dtype=dt):
        o1, g1 = N.run_with_grads(plain, x, _g_of)
        o2, g2 = N.run_with_grads(plain, x, _g_of)
        oh, gh = N.run_with_grads(hooked, x, _g_of)
    spread = max(float((a - b).abs().max()) for a, b in zip(g1, g2))
    diff = max(float((a - b).abs().max()) for a, b in zip(g1, gh))
    print("%s %s: largest gradient difference unhooked/unhooked %.3g, hooked/unhooked %.3g over %d tensors" % (label, dt, spread, diff, len(g1)))
    assert len(o1) == len(oh) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(o1, oh)), "forward"
    for k, (a, b, h) in enumerate(zip(g1, g2, gh)):
        bound = float((a - b).abs().max())
        assert a.dtype == h.dtype, "gradient %d is %s, the stock model's is %s" % (k, h.dtype, a.dtype)
        assert torch.equal(a, h) if bound == 0 else float((a - h).abs().max()) <= bound, "gradient %d: bound %.3g" % (k, bound)
    return o1


@pytest.mark.parametrize("dname", list(HALVES))
def test_hooked_model_equals_the_unhooked_one_under_autocast(deterministic_convolutions, dname):
    from halo_amd import norm
    dt = HALVES[dname]
    torch.manual_seed(41)
    plain = N.randomize_norms(N.Net(), 42).to(DEV)
    hooked, pairs, chains = _hooked(plain)
    assert pairs == 5 and chains == 1                                                  # the stem and the head's four; layer1
    x = torch.randn(2, 3, 33, 47).to(DEV)
    before = dict(norm.launches)
    outs = _held_to_the_unhooked_spread(plain, hooked, x, dt, "backbone + head")
    assert all(o.dtype == torch.float32 for o in outs)                                 # the stock chain's float32, no half leaks out
    # the stem, 3 x 3 norms of the blocks and the head's four pairs, one pass each way; none of the float32 passes
    assert norm.launches == dict(before, ac_fwd=before["ac_fwd"] + 14, ac_bwd=before["ac_bwd"] + 14)
    before = dict(norm.launches)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        want, got = plain(x), hooked(x)
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(want, got))
    assert norm.launches == dict(before, ac_fwd=before["ac_fwd"] + 14)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):                           # the backbone's dict of float32 maps
        want, got = plain.feature_extractor(x), hooked.feature_extractor(x)
    assert list(want) == list(got) and all(got[k].dtype == torch.float32 and torch.equal(want[k], got[k]) for k in want)


def test_with_autocast_off_the_hooked_model_runs_the_float32_passes(deterministic_convolutions, monkeypatch):
    from halo_amd import norm
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0})
    monkeypatch.setattr(norm, "FORK_AUTOGRAD_MIN_ELEMENTS", 0)
    torch.manual_seed(43)
    plain = N.randomize_norms(N.Net(), 44).to(DEV)
    hooked, _, _ = _hooked(plain)
    x = torch.randn(2, 3, 33, 47).to(DEV)
    before = dict(norm.launches)
    o1, g1 = N.run_with_grads(plain, x, _g_of)
    oh, gh = N.run_with_grads(hooked, x, _g_of)
    assert all(torch.equal(a, b) for a, b in zip(o1, oh)) and all(torch.equal(a, b) for a, b in zip(g1, gh))
    assert norm.launches["ac_fwd"] == before["ac_fwd"] and norm.launches["ac_bwd"] == before["ac_bwd"]
    assert norm.launches["fwd"] == before["fwd"] + 14 and norm.launches["bwd"] + norm.launches["fork_bwd"] == before["bwd"] + before["fork_bwd"] + 14


@pytest.mark.parametrize("dname", list(HALVES))
def test_a_chain_hands_its_blocks_half_and_float_from_one_node(deterministic_convolutions, dname):
    """a layer of three bottlenecks, the first with a downsample: blocks 0 and 1 end in outputs="both" -- the successor's conv1
    reads y16, its tail adds y32 --, so both gradients come back to the one node; the last block returns the layer's float32"""
    from halo_amd import norm
    dt = HALVES[dname]
    torch.manual_seed(45)
    plain = N.randomize_norms(nn.Sequential(N.Bottleneck(8, 4, 16, downsample=N.down(8, 16)), N.Bottleneck(16, 4, 16), N.Bottleneck(16, 4, 16, dilation=2)),
                              46).to(DEV)
    hooked, pairs, chains = _hooked(plain)
    assert pairs == 0 and chains == 1
    x = torch.randn(2, 8, 19, 23).to(DEV)
    asked = []
    stock = norm.norm_relu_autocast

    def recorded(x, bn, residual=None, residual_bn=None, outputs="float"):
        asked.append(outputs)
        return stock(x, bn, residual, residual_bn, outputs)
    norm.norm_relu_autocast = recorded
    try:
        before = dict(norm.launches)
        outs = _held_to_the_unhooked_spread(plain, hooked, x, dt, "chain")
    finally:
        norm.norm_relu_autocast = stock
    assert outs[0].dtype == torch.float32
    assert asked == ["half", "half", "both", "half", "half", "both", "half", "half", "float"]
    assert norm.launches == dict(before, ac_fwd=before["ac_fwd"] + 9, ac_bwd=before["ac_bwd"] + 9)
    # without fuse_residual_chains every tail is "float" and autocast casts as before
    from halo_amd.hooks import unfuse_residual_chains
    assert unfuse_residual_chains(hooked) == 1
    del asked[:]
    norm.norm_relu_autocast = recorded
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=dt):
            assert torch.equal(hooked(x), plain(x))
    finally:
        norm.norm_relu_autocast = stock
    assert asked == ["half", "half", "float"] * 3
