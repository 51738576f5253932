"""The separable blocks' pointwise tail on the device: halo_masked_affine_relu_fwd / _bwd of halo_norm.hip, the operator
halo_amd.norm.norm_relu_dropout2d over them, and the hooks use_fused_pointwise_norm / use_fused_decoder_dropout.

Every comparison is torch.equal (NaNs in the same places) against the stock torch statements -- relu(x * scale + shift) * noise, or the
modules themselves -- and their autograd in the same process on the same device: the kernels run those statements with those
roundings, so no tolerance is involved.  torch.equal does not tell -0.0 from +0.0."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dwconv_ref import FrozenBatchNorm2d

pytestmark = pytest.mark.gpu

# name: (B, C, H, W, storage offset of x and g in elements)
CASES = {
    "vector_ragged": (2, 3, 4, 8, 0),               # HW = 32: the 16-byte route, one ragged chunk
    "one_element": (2, 5, 3, 7, 0),                 # HW = 21: the one-element route
    "two_blocks": (1, 2, 33, 128, 0),               # 4224 elements: two workgroups of the 16-byte route, the second ragged
    "five_blocks_offset": (1, 2, 33, 128, 1),       # behind a 4-byte storage offset: five workgroups of the one-element route
    # the same two with B = 2, C = 3, so that plane, channel and mask index all differ in whole and ragged chunks alike; named to
    # sort behind the others, whose seeds are their places in the sorted names
    "work_split_images": (2, 3, 33, 128, 0),
    "work_split_images_offset": (2, 3, 33, 128, 1),
}
MASKS = ("kept", "dropped", "mixed")
KEEP = float(torch.tensor(1.0).div(1 - 0.1))        # fl32(1 / (1 - p)) as noise.div_(1 - p) leaves it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture()
def serve_all(monkeypatch):
    from halo_amd import norm
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0, "masked": 0})


def _at_offset(t, off):
    """t's values in a contiguous tensor whose storage starts `off` elements into its buffer"""
    if off == 0:
        return t
    buf = torch.empty(t.numel() + off, device=t.device, dtype=t.dtype)
    out = buf[off:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.storage_offset() == off
    return out


def same(a, b):
    """torch.equal with NaNs in the same places"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def mask_table(kind, B, C, dev):
    """the fixed tables: "mixed" drops plane (b, c) when b + c is even, so channel 0 is dropped in image 0 and kept in image 1 (and
    the other way round for channel 1): a kernel that reads mask[c] for mask[b * C + c] is caught"""
    b, c = torch.meshgrid(torch.arange(B), torch.arange(C), indexing="ij")
    m = {"kept": torch.ones(B, C, dtype=torch.bool), "dropped": torch.zeros(B, C, dtype=torch.bool), "mixed": (b + c) % 2 == 1}[kind]
    return (m.float() * KEEP).to(dev)


def operands(name, dev, special=False):
    B, C, H, W, off = CASES[name]
    gen = torch.Generator(device=dev).manual_seed(sorted(CASES).index(name))
    rn = lambda *s: torch.randn(s, device=dev, generator=gen)
    x, g = rn(B, C, H, W), rn(B, C, H, W)
    scale, shift = 0.25 + 1.5 * torch.rand(C, device=dev, generator=gen), 0.4 * rn(C)
    scale[-1] = -0.75
    if special:                                      # plane (0, 1) is a kept plane of the "mixed" table
        shift[1] = 0.0
        flat = x[0, 1].view(-1)
        flat[0], flat[1], flat[2], flat[3], flat[5] = float("nan"), float("inf"), float("-inf"), -0.0, 0.0     # flat[5]: pre == 0
    return types.SimpleNamespace(B=B, C=C, H=H, W=W, off=off, x=x, g=g, scale=scale, shift=shift)


def device_fwd(x, scale, shift, mask):
    from halo_amd import _lib
    B, C, H, W = x.shape
    assert x.is_contiguous() and mask.is_contiguous() and mask.numel() == B * C
    y = torch.empty(x.shape, device=x.device)
    _lib.check(_lib.lib().halo_masked_affine_relu_fwd(_lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(mask), _lib.ptr(y), B, C, H * W,
                                                      _lib.stream_ptr(x.device)), "halo_masked_affine_relu_fwd")
    return y


def device_bwd(g, y, scale, mask):
    from halo_amd import _lib
    B, C, H, W = y.shape
    assert g.is_contiguous() and y.is_contiguous()
    gx = torch.empty(y.shape, device=y.device)
    _lib.check(_lib.lib().halo_masked_affine_relu_bwd(_lib.ptr(g), _lib.ptr(y), _lib.ptr(scale), _lib.ptr(mask), _lib.ptr(gx), B, C, H * W,
                                                      _lib.stream_ptr(y.device)), "halo_masked_affine_relu_bwd")
    return gx


def stock(x, g, scale, shift, mask):
    """the stock statements over a fixed noise tensor, and autograd's gradient"""
    B, C = x.shape[:2]
    xt = x.clone().requires_grad_(True)
    y = F.relu(xt * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)) * mask.view(B, C, 1, 1)
    gx, = torch.autograd.grad(y, xt, g)
    return y.detach(), gx


@pytest.mark.parametrize("special", [False, True], ids=["finite", "special"])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_points_are_the_stock_statements(name, kind, special, dev):
    o = operands(name, dev, special)
    mask = mask_table(kind, o.B, o.C, dev)
    x, g = _at_offset(o.x, o.off), _at_offset(o.g, o.off)
    assert (x.data_ptr() % 16 == 0) == (o.off == 0)
    y = device_fwd(x, o.scale, o.shift, mask)
    gx = device_bwd(g, y, o.scale, mask)
    want_y, want_gx = stock(o.x, o.g, o.scale, o.shift, mask)
    assert same(y, want_y), "y"
    assert same(gx, want_gx), "g_x"
    dropped = (mask == 0).view(o.B, o.C, 1, 1).expand_as(y)
    assert bool((gx[dropped] == 0).all())
    if kind != "dropped":
        assert bool((y > 0).any()) and bool((gx != 0).any())
    if special and kind != "dropped":               # plane (0, 1) is kept: NaN stays NaN, inf stays inf, -0.0 and pre == 0 give 0
        flat, gflat = y[0, 1].view(-1), gx[0, 1].view(-1)
        assert bool(torch.isnan(flat[0])) and bool(torch.isinf(flat[1:3]).any()) and float(flat[3]) == 0.0 and float(flat[5]) == 0.0
        assert float(gflat[3]) == 0.0 and float(gflat[5]) == 0.0 and float(gflat[0]) != 0.0      # a NaN y lets g through


@pytest.mark.parametrize("name", ["vector_ragged", "five_blocks_offset"])
def test_an_inf_in_a_dropped_plane_is_a_nan_on_both_sides(name, dev):
    """the forward reads x in dropped planes too: inf * 0"""
    o = operands(name, dev)
    mask = mask_table("mixed", o.B, o.C, dev)
    assert float(mask[0, 0]) == 0.0
    sign = 1.0 if float(o.scale[0]) > 0 else -1.0
    o.x[0, 0].view(-1)[2] = sign * float("inf")                       # pre = +inf in the dropped plane (0, 0)
    o.x[0, 0].view(-1)[3] = -sign * float("inf")                      # pre = -inf: the ReLU's 0, times 0
    y = device_fwd(_at_offset(o.x, o.off), o.scale, o.shift, mask)
    want_y, _ = stock(o.x, o.g, o.scale, o.shift, mask)
    assert same(y, want_y)
    flat = y[0, 0].view(-1)
    assert bool(torch.isnan(flat[2])) and bool(torch.isnan(want_y[0, 0].view(-1)[2])) and float(flat[3]) == 0.0
    assert int(torch.isnan(y).sum()) == 1


def test_repeated_calls_and_a_side_stream_give_the_same_bits(dev):
    o = operands("five_blocks_offset", dev)
    mask = mask_table("mixed", o.B, o.C, dev)
    x, g = _at_offset(o.x, o.off), _at_offset(o.g, o.off)

    def run():
        y = device_fwd(x, o.scale, o.shift, mask)
        return y, device_bwd(g, y, o.scale, mask)
    first, second = run(), run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for t1, t2, t3 in zip(first, second, third):
        assert torch.equal(t1, t2) and torch.equal(t1, t3)


def _frozen(n, seed, dev=None):
    gen = torch.Generator().manual_seed(seed)
    bn = FrozenBatchNorm2d(n)
    bn.weight.copy_(0.25 + 1.5 * torch.rand(n, generator=gen)), bn.bias.copy_(0.4 * torch.randn(n, generator=gen))
    bn.running_mean.copy_(0.5 * torch.randn(n, generator=gen)), bn.running_var.copy_(0.3 + 1.5 * torch.rand(n, generator=gen))
    bn.weight[1] = -0.75
    return bn if dev is None else bn.to(dev)


def _pair(dev, B=2, C=16, H=4, W=8, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn((B, C, H, W), device=dev, generator=gen), torch.randn((B, C, H, W), device=dev, generator=gen)


def _both_sides(x0, g, bn, drop, seed, fn):
    x = x0.clone().requires_grad_(True)
    torch.manual_seed(seed)
    y = fn(x, bn, drop)
    state = torch.cuda.get_rng_state(x0.device)
    gx, = torch.autograd.grad(y, x, g, retain_graph=True)
    assert torch.equal(x.detach(), x0)
    return y, gx, state


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_generator_parity_with_dropout2d(seed, dev, serve_all):
    """a seeded run has nn.Dropout2d's bits and leaves the device generator where nn.Dropout2d leaves it"""
    from halo_amd import norm
    x0, g = _pair(dev, seed=seed)
    bn, drop = _frozen(16, seed, dev), nn.Dropout2d(0.5)
    assert norm.dropout_fallback_reason(x0.clone().requires_grad_(True), bn, drop) is None
    before = dict(norm.launches)
    y, gx, state = _both_sides(x0, g, bn, drop, seed, norm.norm_relu_dropout2d)
    assert norm.launches["masked_fwd"] == before["masked_fwd"] + 1 and norm.launches["masked_bwd"] == before["masked_bwd"] + 1
    want_y, want_gx, want_state = _both_sides(x0, g, bn, drop, seed, norm.dropout_statement)
    assert torch.equal(y, want_y) and torch.equal(gx, want_gx) and torch.equal(state, want_state)
    noise = y.grad_fn.saved_tensors[2]
    assert tuple(noise.shape) == (2, 16, 1, 1) and bool((noise == 0).any()) and bool((noise != 0).any())    # 32 planes: 2^-31 otherwise
    assert set(noise.unique().tolist()) == {0.0, 2.0}
    torch.manual_seed(seed + 100)                                      # another seed, another mask: the generator is really read
    other = norm.norm_relu_dropout2d(x0, bn, drop)
    assert not torch.equal(other, y.detach())


def test_eval_mode_and_p_zero_draw_nothing(dev, serve_all):
    from halo_amd import norm
    x0, g = _pair(dev, seed=3)
    bn = _frozen(16, 3, dev)
    for drop in (nn.Dropout2d(0.5).eval(), nn.Dropout2d(0.0)):
        torch.manual_seed(4)
        state = torch.cuda.get_rng_state(dev)
        before = dict(norm.launches)
        y, gx, after = _both_sides(x0, g, bn, drop, 4, norm.norm_relu_dropout2d)
        assert torch.equal(after, state)
        assert norm.launches["fwd"] == before["fwd"] + 1 and norm.launches["bwd"] == before["bwd"] + 1
        assert norm.launches["masked_fwd"] == before["masked_fwd"] and norm.launches["masked_bwd"] == before["masked_bwd"]
        x = x0.clone().requires_grad_(True)
        want = norm.norm_relu(x, bn)
        assert torch.equal(y, want) and torch.equal(gx, torch.autograd.grad(want, x, g)[0])
        want_y, want_gx, _ = _both_sides(x0, g, bn, drop, 4, norm.dropout_statement)
        assert torch.equal(y, want_y) and torch.equal(gx, want_gx)


def test_saved_tensors_and_launches_per_needs_input_grad(dev, serve_all):
    """the backward keeps y, scale and the noise tensor and nothing else; one launch each way when x needs a gradient, the forward
    alone when it does not, nothing at all from a backward that is asked for nothing"""
    from halo_amd import norm
    x0, g = _pair(dev, seed=5)
    bn, drop = _frozen(16, 5, dev), nn.Dropout2d(0.5)
    scale, _ = norm.cached_scale_shift(bn)
    kept = []
    x = x0.clone().requires_grad_(True)
    before = dict(norm.launches)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (kept.append(t), t)[1], lambda t: t):
        torch.manual_seed(6)
        y = norm.norm_relu_dropout2d(x, bn, drop)
    assert sorted(tuple(t.shape) for t in kept) == sorted([(2, 16, 4, 8), (16,), (2, 16, 1, 1)])
    assert any(t.data_ptr() == y.data_ptr() for t in kept) and any(t.data_ptr() == scale.data_ptr() for t in kept)
    assert not any(t.data_ptr() == x.data_ptr() for t in kept)                          # x is not kept
    y.backward(g)
    assert norm.launches["masked_fwd"] == before["masked_fwd"] + 1 and norm.launches["masked_bwd"] == before["masked_bwd"] + 1
    assert norm.launches["fwd"] == before["fwd"] and norm.launches["bwd"] == before["bwd"]      # the existing keys keep their meaning
    for ctx_mgr in (torch.no_grad(), torch.enable_grad()):                              # no gradient wanted: the forward alone
        before = dict(norm.launches)
        with ctx_mgr:
            torch.manual_seed(6)
            y1 = norm.norm_relu_dropout2d(x0, bn, drop)
        assert not y1.requires_grad and torch.equal(y1, y.detach())
        assert norm.launches["masked_fwd"] == before["masked_fwd"] + 1 and norm.launches["masked_bwd"] == before["masked_bwd"]
    before = dict(norm.launches)
    noise = next(t for t in kept if tuple(t.shape) == (2, 16, 1, 1))
    ctx = types.SimpleNamespace(saved_tensors=(y.detach(), scale, noise), needs_input_grad=(False, False, False, False))
    assert norm._NormReluDropFn.backward(ctx, g) == (None,) * 4 and norm.launches == before


def test_fallbacks_run_the_stock_statements(dev, serve_all):
    from halo_amd import norm
    x0, g = _pair(dev, seed=7)
    frozen = _frozen(16, 7, dev)
    live = nn.BatchNorm2d(16).to(dev).eval()
    with torch.no_grad():
        live.running_mean.copy_(frozen.running_mean), live.running_var.copy_(frozen.running_var)
    strided = torch.randn(2, 4, 8, 16, device=dev).permute(0, 3, 1, 2)                 # channels-last values behind an NCHW view
    assert tuple(strided.shape) == (2, 16, 4, 8) and not strided.is_contiguous()
    cases = (("p = 1", x0, frozen, nn.Dropout2d(1.0), True), ("in place", x0, frozen, nn.Dropout2d(0.5, inplace=True), False),
             ("FrozenBatchNorm2d", x0, live, nn.Dropout2d(0.5), True), ("contiguous", strided, frozen, nn.Dropout2d(0.5), True))
    for word, x_in, bn, drop, with_grad in cases:
        assert word in norm.dropout_fallback_reason(x_in, bn, drop), word
        before = dict(norm.launches)
        if with_grad:
            y, gx, state = _both_sides(x_in, g, bn, drop, 8, norm.norm_relu_dropout2d)
            want = _both_sides(x_in, g, bn, drop, 8, norm.dropout_statement)
            assert torch.equal(y, want[0]) and torch.equal(gx, want[1]) and torch.equal(state, want[2]), word
        else:                                       # torch's own backward refuses relu_ followed by an in-place product
            with torch.no_grad():
                torch.manual_seed(8)
                y = norm.norm_relu_dropout2d(x_in.clone(), bn, drop)
                torch.manual_seed(8)
                assert torch.equal(y, norm.dropout_statement(x_in.clone(), bn, drop)), word
        assert norm.launches == before, word


# ---------------------------------------------------------------- the hooks on a stand-in v3+ head

class Block(nn.Module):
    """DepthwiseSeparableConv2d's attribute names and layout"""

    def __init__(self, cin, cout, d):
        super().__init__()
        self.depthwise_conv = nn.Conv2d(cin, cin, 3, 1, d, d, groups=cin, bias=False)
        self.depthwise_bn = _frozen(cin, cin + d)
        self.depthwise_activate = nn.ReLU(inplace=True)
        self.pointwise_conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.pointwise_bn = _frozen(cout, cout + d + 1)
        self.pointwise_activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.depthwise_activate(self.depthwise_bn(self.depthwise_conv(x)))
        return self.pointwise_activate(self.pointwise_bn(self.pointwise_conv(x)))


class _Head(nn.Module):
    """a stand-in v3+ hyperbolic head: channels 16 / 8 / 8, the reference's attribute names, dilations and block layout, with the
    nn.Dropout2d behind decoder[1]"""

    def __init__(self, block, C=16, K=5, top=16, mid=8, low=8):
        super().__init__()
        from halo_amd.core.utils.hyperbolic import HyperMapper, HyperMLR
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(top, mid, 1, bias=False), _frozen(mid, 1), nn.ReLU(inplace=True))] + [
            block(top, mid, d) for d in (6, 12, 18)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(top, mid, 1, bias=False), _frozen(mid, 2), nn.ReLU(inplace=True))
        self.bottleneck = nn.Sequential(nn.Conv2d(5 * mid, mid, 3, padding=1, bias=False), _frozen(mid, 3), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(low, 6, 1, bias=False), _frozen(6, 4), nn.ReLU(inplace=True))
        self.decoder = nn.Sequential(block(mid + 6, mid, 1), block(mid, mid, 1), nn.Dropout2d(0.5))
        self.conv_reduce = nn.Conv2d(mid, C, 1)
        self.mapper = HyperMapper(c=1.0)
        self.conv_seg = HyperMLR(C, K, c=1.0)
        for m in self.modules():                                     # pre-activations a few times the norms' shifts: every ReLU of the
            if isinstance(m, nn.Conv2d):                             # head has active and inactive elements in most planes
                m.weight.data = torch.randn(m.weight.shape) * (2.0 / m.weight[0].numel() ** 0.5)


def _run(head, feats, g_out, g_embed, seed):
    top, low = feats["out"].clone().requires_grad_(True), feats["low"].clone().requires_grad_(True)
    torch.manual_seed(seed)
    out, embed = head({"out": top, "low": low})
    state = torch.cuda.get_rng_state(top.device)
    named = [(n, p) for n, p in head.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad([out, embed], [top, low] + [p for _, p in named], [g_out, g_embed])
    return (out.detach(), embed.detach(), state) + grads, ["out", "embed", "generator", "g_top", "g_low"] + [n for n, _ in named]


@pytest.mark.parametrize("front", [False, True], ids=["plain_front", "fused_front"])
@pytest.mark.parametrize("order", ["depthwise_first", "pointwise_first"])
def test_marked_head_returns_the_unmarked_heads_bits(order, front, dev, serve_all):
    """head A under use_fused_depthwise alone against head B with use_fused_pointwise_norm and use_fused_decoder_dropout added, in
    either binding order, in train() mode under the same seed: both outputs, every parameter gradient, the input gradients and the
    generator state"""
    from halo_amd import norm
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import (fused_dwsep_forward, use_fused_decoder_dropout, use_fused_decoder_front, use_fused_depthwise,
                                use_fused_pointwise_norm)
    BlockA = use_fused_depthwise(type("BlockA", (Block,), {}))
    BlockB = type("BlockB", (Block,), {})
    if order == "depthwise_first":
        use_fused_depthwise(BlockB), use_fused_pointwise_norm(BlockB)
    else:
        use_fused_pointwise_norm(BlockB), use_fused_depthwise(BlockB)
    assert BlockB.forward is fused_dwsep_forward and BlockB._halo_fused_pointwise_norm and not hasattr(BlockA, "_halo_fused_pointwise_norm")
    HeadA = type("HeadA", (_Head,), {"forward": v3plus_hyper_forward})
    HeadB = use_fused_decoder_dropout(type("HeadB", (_Head,), {"forward": v3plus_hyper_forward}))
    if front:
        use_fused_decoder_front(HeadA), use_fused_decoder_front(HeadB)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(11)
        with torch.no_grad():
            a, b = HeadA(BlockA), HeadB(BlockB)
        b.load_state_dict(a.state_dict())
        keys = list(a.state_dict())
        a, b = a.to(dev).train(), b.to(dev).train()
        gen = torch.Generator().manual_seed(12)
        feats = {"low": torch.randn(2, 8, 12, 16, generator=gen).to(dev), "out": torch.randn(2, 16, 6, 8, generator=gen).to(dev)}
        with torch.no_grad():
            shape_out, shape_embed = (t.shape for t in a(feats))
        g_out = torch.randn(shape_out, generator=gen).to(dev)
        g_embed = torch.randn(shape_embed, generator=gen).double().to(dev)
        before = dict(norm.launches)
        res_a, names = _run(a, feats, g_out, g_embed, 13)
        assert norm.launches == before                                 # head A runs none of this module's passes
        res_b, _ = _run(b, feats, g_out, g_embed, 13)
        # head B: the three ASPP blocks and decoder[0] through norm_relu, decoder[1] with its dropout through the masked pass
        assert norm.launches["masked_fwd"] == before["masked_fwd"] + 1 and norm.launches["masked_bwd"] == before["masked_bwd"] + 1
        assert norm.launches["fwd"] == before["fwd"] + 4 and norm.launches["bwd"] == before["bwd"] + 4
        for name, t_a, t_b in zip(names, res_a, res_b):
            assert t_a.shape == t_b.shape and torch.equal(t_a, t_b), name
        assert bool(torch.isfinite(res_a[0]).all()) and float(res_a[0].std()) > 0 and all(float(t.abs().sum()) > 0 for t in res_a[3:])
        assert list(b.state_dict()) == keys
        # eval mode: the dropout draws nothing, the pair runs norm_relu's pass
        a.eval(), b.eval()
        with torch.no_grad():
            before = dict(norm.launches)
            torch.manual_seed(14)
            state = torch.cuda.get_rng_state(dev)
            out_a, out_b = a(feats), b(feats)
            assert torch.equal(out_a[0], out_b[0]) and torch.equal(out_a[1], out_b[1]) and torch.equal(torch.cuda.get_rng_state(dev), state)
            assert norm.launches["fwd"] == before["fwd"] + 5 and norm.launches["masked_fwd"] == before["masked_fwd"]
    finally:
        torch.backends.cudnn.deterministic = was
