"""halo_amd.norm.norm_relu (halo_norm.hip) and the two hooks against the stock torch chain on the same device.  The kernel runs the
chain's own operations with the chain's roundings, so every comparison is torch.equal (NaN positions equal where the inputs carry
NaN).  Whole models are held to the difference between two runs of the unhooked model, gradient by gradient; with the library's
deterministic convolution algorithms, which those tests ask for, that difference is zero and the comparison is torch.equal too."""
import pytest
import torch

import norm_ref as N
from dwconv_ref import FrozenBatchNorm2d

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = {
    "scalar_short_plane": (2, 3, 5, 7),          # HW = 35: one element per lane, a plane shorter than a wave
    "vector_partial_block": (1, 2, 8, 12),       # HW = 96: 24 groups of four in one partial workgroup
    "several_blocks": (2, 5, 80, 160),           # HW = 12800: three full chunks of 1024 groups and a partial one
    "several_blocks_large": (1, 3, 160, 320),    # HW = 51200: twelve full chunks and a partial one
    "odd_multiple_of_four": (1, 2, 37, 52),      # HW = 1924 = 4 * 481: no multiple of a wave, a block or a chunk
    "unaligned_view": (1, 2, 8, 12),             # storage offset of one element: operands off 16 bytes
    "scalar_whole_chunk": (2, 3, 13, 79),        # HW = 1027: one element per lane, a whole chunk of 1024 and three elements more
    "unaligned_chunks": (1, 2, 33, 128),         # the same offset over HW = 4224: four whole chunks of single elements, a ragged fifth
}
VARIANTS = ("none", "plain", "affine")


@pytest.fixture(autouse=True)
def every_size_served(monkeypatch):
    """halo_amd.norm leaves small tensors that need a gradient to the stock statements because they are faster there (a speed
    rule: the bits are the same); these tests are about the kernels, so they switch the rule off"""
    from halo_amd import norm
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0})


def _norm(C, seed):
    """channel 0: scale = -2, shift = +1; channel 1: scale = +2, shift = -1 (x = 0.5 gives pre == 0 in both); the rest random with
    both signs"""
    bn = N.randomize_norms(FrozenBatchNorm2d(C), seed)
    with torch.no_grad():
        bn.weight[0], bn.running_var[0], bn.bias[0], bn.running_mean[0] = -2.0, 1.0, 1.0, 0.0
        bn.weight[1], bn.running_var[1], bn.bias[1], bn.running_mean[1] = 2.0, 1.0, -1.0, 0.0
    return bn.to(DEV)


def _tensor(shape, gen, unaligned, special):
    n = 1
    for s in shape:
        n *= s
    flat = torch.randn(n, generator=gen)
    if special:
        k = min(n, 28)
        flat[torch.randperm(n, generator=gen)[:k]] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 0.5, 0.5] * 4)[:k]
        t = flat.view(shape)
        t[0, 0, 0, :3] = 0.5                       # pre == 0 exactly in channels 0 and 1
        t[0, 1, -1, -3:] = 0.5
        t[0, 0, 1, 0], t[0, 1, 1, 1] = -0.0, float("nan")
    if unaligned:
        base = torch.empty(n + 1, device=DEV)
        base[1:].copy_(flat)
        out = base[1:].view(shape)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4
        return out
    return flat.view(shape).to(DEV)


@pytest.fixture(scope="module")
def cases():
    """per (shape name, variant): operands, the stock chain's y and gradients, computed once and left unchanged"""
    out = {}
    for si, (name, shape) in enumerate(SHAPES.items()):
        for vi, variant in enumerate(VARIANTS):
            gen = torch.Generator().manual_seed(100 * si + vi)
            un = name.startswith("unaligned")
            bn = _norm(shape[1], 7 + si)
            rbn = _norm(shape[1], 70 + si) if variant == "affine" else None
            x = _tensor(shape, gen, un, True)
            r = _tensor(shape, gen, un, True) if variant != "none" else None
            g = _tensor(shape, gen, un, False)
            g[torch.rand(shape, generator=gen).to(DEV) < 0.2] = 0.0
            xs = x.clone().requires_grad_(True)
            rs = r.clone().requires_grad_(True) if r is not None else None
            ys = N.stock_chain(xs, bn, rs, rbn)
            grads = torch.autograd.grad(ys, [xs] if r is None else [xs, rs], g)
            pre = bn(x)
            assert int((pre == 0).sum()) >= 2 and bool(pre.isnan().any()) and bool(pre.isinf().any())
            s = bn.weight * bn.running_var.rsqrt()
            assert bool((s < 0).any()) and bool((s > 0).any())
            sh = bn.bias - bn.running_mean * s
            assert bool((sh < 0).any()) and bool((sh > 0).any())
            out[(name, variant)] = dict(bn=bn, rbn=rbn, x=x, r=r, g=g, y=ys.detach(), gx=grads[0], gr=grads[1] if r is not None else None)
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_operator_equals_the_stock_chain(cases, name, variant):
    from halo_amd import norm
    c = cases[(name, variant)]
    assert norm.fallback_reason(c["x"], c["bn"], c["r"], c["rbn"]) is None
    x0 = c["x"].clone()
    x = c["x"].detach().requires_grad_(True)                 # the same storage and offset; the shared case stays as it is
    r = c["r"].detach().requires_grad_(True) if c["r"] is not None else None
    before = dict(norm.launches)
    y = norm.norm_relu(x, c["bn"], r, c["rbn"])
    grads = torch.autograd.grad(y, [x] if r is None else [x, r], c["g"])
    assert norm.launches["fwd"] == before["fwd"] + 1 and norm.launches["bwd"] == before["bwd"] + 1     # one pass each way
    assert N.same_bits(y.detach(), c["y"]), "y"
    assert N.same_bits(grads[0], c["gx"]), "g_x"
    if r is not None:
        assert N.same_bits(grads[1], c["gr"]), "g_r"
    assert N.same_bits(c["x"], x0)                                                                     # out of place


@pytest.mark.parametrize("variant", ["plain", "affine"])
def test_only_the_gradients_asked_for_are_launched(cases, variant):
    from halo_amd import norm
    c = cases[("odd_multiple_of_four", variant)]
    x, r = c["x"].clone(), c["r"].clone()
    before = dict(norm.launches)
    y = norm.norm_relu(x.requires_grad_(True), c["bn"], r, c["rbn"])                       # only x
    (gx,) = torch.autograd.grad(y, [x], c["g"])
    assert N.same_bits(gx, c["gx"]) and norm.launches["bwd"] == before["bwd"] + 1
    x = x.detach()
    y = norm.norm_relu(x, c["bn"], r.requires_grad_(True), c["rbn"])                       # only the residual
    (gr,) = torch.autograd.grad(y, [r], c["g"])
    assert N.same_bits(gr, c["gr"]) and norm.launches["bwd"] == before["bwd"] + 2
    y = norm.norm_relu(x, c["bn"], r.detach(), c["rbn"])                                   # neither: the stem, whose input is the image
    assert y.grad_fn is None and not y.requires_grad and N.same_bits(y, c["y"])
    w = torch.ones((), device=DEV, requires_grad=True)
    (y * w).sum().backward()                                                               # a backward pass that reaches y launches nothing here
    assert norm.launches["bwd"] == before["bwd"] + 2 and norm.launches["fwd"] == before["fwd"] + 3


def test_repeated_and_side_stream_calls_return_equal_bits(cases):
    from halo_amd.norm import norm_relu
    c = cases[("several_blocks", "affine")]
    x, r = c["x"].clone().requires_grad_(True), c["r"].clone().requires_grad_(True)
    runs = []
    for _ in range(3):
        y = norm_relu(x, c["bn"], r, c["rbn"])
        runs.append((y.detach(),) + torch.autograd.grad(y, [x, r], c["g"]))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        y = norm_relu(x, c["bn"], r, c["rbn"])
        runs.append((y.detach(),) + torch.autograd.grad(y, [x, r], c["g"]))
    side.synchronize()
    for run in runs:
        assert N.same_bits(run[0], c["y"]) and N.same_bits(run[1], c["gx"]) and N.same_bits(run[2], c["gr"])


def test_cache_cannot_serve_stale_statistics():
    from halo_amd.norm import cached_scale_shift, norm_relu
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 6, 9, 12, generator=gen).to(DEV)
    bn = N.randomize_norms(FrozenBatchNorm2d(6), 12).to(DEV)

    def check():
        assert torch.equal(norm_relu(x, bn), N.stock_chain(x, bn))
    check()
    pair = cached_scale_shift(bn)
    check()
    assert cached_scale_shift(bn)[0] is pair[0]                                            # reused
    bn.load_state_dict(N.randomize_norms(FrozenBatchNorm2d(6), 13).state_dict())
    check()
    assert cached_scale_shift(bn)[0] is not pair[0]
    with torch.no_grad():
        bn.running_var.mul_(3.0)
    check()
    bn.bias = bn.bias + 1.0                                                                # a replaced buffer
    check()
    bn.cpu()
    assert torch.equal(norm_relu(x.cpu(), bn), N.stock_chain(x.cpu(), bn))                 # off the device: the stock statements
    bn.to(DEV)
    check()


def test_offsets_past_two_to_the_31_elements():
    """1 x 2049 x 1024 x 1024: the last plane starts at element 2^31.  No full-size stock chain is run: the first and the last plane
    are compared with the stock chain run on those two slices."""
    from halo_amd.norm import norm_relu
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 24 * 2 ** 30:
        pytest.skip("%.1f GB free on the device, 24 GB needed for x and y of 8.6 GB each" % (free / 2 ** 30))
    C, H, W = 2049, 1024, 1024
    bn = N.randomize_norms(FrozenBatchNorm2d(C), 21).to(DEV)
    x = torch.empty((1, C, H, W), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(22)
    for c0 in range(0, C, 256):                                                            # in pieces: no 8.6 GB temporary
        x[:, c0:c0 + 256].normal_(generator=gen)
    with torch.no_grad():
        y = norm_relu(x, bn)
    for c in (0, C - 1):
        one = FrozenBatchNorm2d(1).to(DEV)
        with torch.no_grad():
            for n in ("weight", "bias", "running_mean", "running_var"):
                getattr(one, n).copy_(getattr(bn, n)[c:c + 1])
            want = N.stock_chain(x[:, c:c + 1].clone(), one)
        assert torch.equal(y[:, c:c + 1], want), "plane %d" % c
        assert float(want.max()) > 0 and float(want.min()) == 0
    del x, y
    torch.cuda.empty_cache()


@pytest.fixture
def deterministic_convolutions(monkeypatch):
    """Left to itself the library's backward of the stem's stride-2 convolution sums its weight gradient in an order that changes
    from run to run: over eight runs of the UNHOOKED stand-in that one tensor differed by up to 5.7e-6 from run to run while every
    other gradient and the forward were bit-equal, hooked or not.  A bound drawn from two such runs is a draw of its own (the hooked
    run's distance can land above or below it), so the model comparisons ask the library for its deterministic algorithms: the two
    unhooked runs then agree, the bound is zero and the hooked model must be torch.equal."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


def _held_to_the_unhooked_spread(plain, hooked, x, label):
    """forward torch.equal; each gradient of the hooked model differs from the unhooked model's by at most the largest difference
    between two runs of the unhooked model (zero, i.e. torch.equal, when those agree)"""
    g_of = lambda outs: [torch.randn(o.shape, generator=torch.Generator().manual_seed(31 + i)).to(DEV) for i, o in enumerate(outs)]
    o1, g1 = N.run_with_grads(plain, x, g_of)
    o2, g2 = N.run_with_grads(plain, x, g_of)
    oh, gh = N.run_with_grads(hooked, x, g_of)
    spread = max(float((a - b).abs().max()) for a, b in zip(g1, g2))
    diff = max(float((a - b).abs().max()) for a, b in zip(g1, gh))
    print("%s: largest gradient difference unhooked/unhooked %.3g, hooked/unhooked %.3g over %d tensors" % (label, spread, diff, len(g1)))
    assert len(o1) == len(oh) and all(torch.equal(a, b) for a, b in zip(o1, oh)), "forward"
    for k, (a, b, h) in enumerate(zip(g1, g2, gh)):
        bound = float((a - b).abs().max())
        assert torch.equal(a, h) if bound == 0 else float((a - h).abs().max()) <= bound, "gradient %d: bound %.3g" % (k, bound)


def test_hooked_backbone_equals_the_unhooked_one(deterministic_convolutions):
    from halo_amd import norm
    torch.manual_seed(41)
    plain = N.randomize_norms(N.backbone(), 42).to(DEV)
    hooked, pairs = N.hooked_copy(plain)
    assert pairs == 1                                                                       # the stem
    x = torch.randn(2, 3, 33, 47).to(DEV)
    before = dict(norm.launches)
    _held_to_the_unhooked_spread(plain, hooked, x, "backbone")
    assert norm.launches["fwd"] == before["fwd"] + 10 and norm.launches["bwd"] == before["bwd"] + 10   # the stem and 3 x 3 norms


def test_fused_head_pairs_equal_the_unfused_head(deterministic_convolutions):
    import copy
    from halo_amd import norm
    from halo_amd.hooks import fuse_norm_relu_pairs
    torch.manual_seed(43)
    plain = N.randomize_norms(N.Net(), 44).to(DEV)
    fused = copy.deepcopy(plain)
    assert fuse_norm_relu_pairs(fused.classifier) == 4
    x = torch.randn(2, 3, 33, 47).to(DEV)
    before = dict(norm.launches)
    _held_to_the_unhooked_spread(plain, fused, x, "head")
    assert norm.launches["fwd"] == before["fwd"] + 4 and norm.launches["bwd"] == before["bwd"] + 4
