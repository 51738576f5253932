"""The folded image-pooling branch on the device (halo_pool_fold_* of halo_norm.hip through halo_amd.aspp and
halo_amd.hooks.use_folded_image_pooling).  u = 2^-24, u64 = 2^-53.

Operator level.  The table T is held to float64 numpy; given z and the device's T, the epilogue and its backward are the torch
composition relu(((z + tmap) * scale) + shift) and its autograd, value for value; the class sums g_T are held to float64 sums of
the device's own g_z.

Head level (the stand-in head at the bottom).  Every weight, norm scale, input and output gradient of that head is positive, so
every sum of its backward adds terms of one sign: the absolute-value evaluation of a gradient is the gradient, and a bound "terms
times u times the absolute-value evaluation" is a relative one.  The norms have running_var = 1 and running_mean = 0, so scale =
weight and shift = bias are exact on both sides; the biases have both signs, so every ReLU has inactive elements.  Term counts
(float32 roundings along the longest path, first order; map 6 x 8 = 48 pixels, B = 2, Co = 8 output channels, 16 input channels):

  forward, per layer: N_out = N_in + terms + 2 (the norm's product and sum); magnitude m_out = scale conv(|w|, m_in) + |shift| >= out
      parallel_branches[0] 16 + 2 = 18;  separable block: depthwise 9 + 2 = 11, pointwise 11 + 16 + 2 = 29      -> N_p = 29
      global_branch: mean 48 + 1, conv 16, norm 2                                                               -> N_v = 67
  g_z = fl(gp scale): 1;  g_p (conv backward over Co x 9 taps): 1 + 72 = 73
  g_v: g_z 1, the float64 class sums and contractions 1, the final rounding 1 = 3
  g_top: the longest path is a separable block: 73 + 1 (norm) + 8 (pointwise, Co) + 1 (norm) + 9 (depthwise) = 92, then 5 paths added = 97
      (pooled path: 3 + 1 + 8 + 1 (the mean's division) = 13;  parallel_branches[0]: 73 + 1 + 8 = 82)
  g_Wm[o,c,k] = sum over B x 48 pixels of g_z p: (96 + 1 + 1) u sum g_z p  +  N_p u sum g_z m_p      (p carries its forward error)
  g_Wg[o,c,k] = sum_b g_S v:                     3 u sum g_S v             +  N_v u sum g_S m_v
  g_Wglobal[o,c] = sum_b (g_v mask scale) mean:  (3 + 1 + 49 + 2) = 55, relative (the mean's magnitude is the mean)

The precondition that makes the ReLU masks of both sides equal -- no float64 pre-activation within N u m of zero, at any ReLU of
the stage, and within the forward bound at the bottleneck -- is asserted on the float64 evaluation; the seed is one for which it
holds.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dwconv_ref as R

pytestmark = pytest.mark.gpu
U, U64 = 2.0 ** -24, 2.0 ** -53
CX = 3

# name: (B, Co, H, W, Cg, storage offset of z and g in elements)
CASES = {
    "vector_interior": (2, 5, 5, 8, 3, 0),          # 16-byte route, interior rows
    "no_interior": (2, 3, 2, 2, 2, 0),              # every pixel a corner
    "one_element": (1, 2, 5, 7, 4, 0),              # W % 4 != 0
    "offset": (2, 5, 5, 8, 3, 1),                   # W % 4 == 0 behind a 4-byte storage offset: the one-element route
    "two_blocks": (1, 2, 33, 128, 5, 0),            # 4224 elements: two workgroups of the 16-byte route, the second ragged
    "five_blocks_offset": (1, 2, 33, 128, 5, 3),    # five workgroups of the one-element route, the last ragged
    "wide_pool": (2, 2, 3, 4, 300, 0),              # Cg above and no multiple of the fold pass's 256 lanes
    # two_blocks and five_blocks_offset with B = 2, Co = 3, so that plane and channel differ in whole and ragged chunks alike; named
    # to sort behind the others, whose seeds are their places in the sorted names
    "work_split_images": (2, 3, 33, 128, 5, 0),
    "work_split_images_offset": (2, 3, 33, 128, 5, 1),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _at_offset(t, off):
    """t's values in a contiguous tensor whose storage starts `off` elements into its buffer"""
    if off == 0:
        return t
    buf = torch.empty(t.numel() + off, device=t.device, dtype=t.dtype)
    out = buf[off:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.storage_offset() == off
    return out


def operands(name, dev, special=False):
    B, Co, H, W, Cg, off = CASES[name]
    gen = torch.Generator(device=dev).manual_seed(sorted(CASES).index(name))
    rn = lambda *s: torch.randn(s, device=dev, generator=gen)
    w, v, z, g = rn(Co, CX + Cg, 3, 3), rn(B, Cg, 1, 1), rn(B, Co, H, W), rn(B, Co, H, W)
    scale, shift = 0.25 + 1.5 * torch.rand(Co, device=dev, generator=gen), 0.4 * rn(Co)
    scale[-1] = -0.75
    if special:
        shift[0] = 0.0
        flat = z.view(-1)
        flat[0], flat[1], flat[2], flat[3] = float("nan"), float("inf"), float("-inf"), -0.0
        g.view(-1)[5] = float("inf")
    return types.SimpleNamespace(B=B, Co=Co, H=H, W=W, Cg=Cg, off=off, w=w, v=v, z=z, g=g, scale=scale, shift=shift)


def classes(H, W, dev):
    rc = torch.ones(H, dtype=torch.long, device=dev)
    rc[0], rc[-1] = 0, 2
    cc = torch.ones(W, dtype=torch.long, device=dev)
    cc[0], cc[-1] = 0, 2
    return rc, cc


def table_map(T, H, W):
    rc, cc = classes(H, W, T.device)
    return T[:, :, rc][:, :, :, cc]


def same(a, b):
    """torch.equal with NaNs in the same places"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_against_float64(name, dev):
    from halo_amd import aspp
    o = operands(name, dev)
    T = aspp.fold_table(o.w, o.v, CX).cpu().numpy().astype(np.float64).reshape(o.B, o.Co, 9)
    Wg = o.w[:, CX:].cpu().numpy().astype(np.float64).reshape(o.Co, o.Cg, 9)
    v = o.v.cpu().numpy().astype(np.float64).reshape(o.B, o.Cg)
    M = aspp.class_to_tap_matrix().numpy()
    T64 = np.einsum("ock,bc->bok", Wg, v) @ M.T
    mag = np.einsum("ock,bc->bok", np.abs(Wg), np.abs(v)) @ M.T
    bound = U * np.abs(T64) + (9 * o.Cg + 9) * U64 * mag
    ratio = float((np.abs(T - T64) / bound).max())
    print("%s: T, max |delta| / bound %.3f" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("special", [False, True], ids=["finite", "special"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_epilogue_is_the_torch_composition(name, special, dev):
    """y and g_z are the torch statement's values given z and the device's T; g_T is the float64 sum of that g_z per class"""
    from halo_amd import aspp
    o = operands(name, dev, special)
    T = aspp.fold_table(o.w, o.v, CX)
    tmap = table_map(T, o.H, o.W)
    if special:
        o.z[0, 0, 1, 1] = -tmap[0, 0, 1, 1]                              # z + T = 0 under shift[0] = 0: pre == 0
        o.z[0, 0, -1, -1] = -tmap[0, 0, -1, -1]
    z, g = _at_offset(o.z, o.off), _at_offset(o.g, o.off)
    y = aspp.fold_forward(z, T, o.scale, o.shift)
    g_z, g_T = aspp.fold_backward(g, y, o.scale)
    zt = o.z.clone().requires_grad_(True)
    want = F.relu(((zt + tmap) * o.scale.view(1, -1, 1, 1)) + o.shift.view(1, -1, 1, 1))
    want_gz, = torch.autograd.grad(want, zt, o.g)
    assert same(y, want.detach()) and same(g_z, want_gz)
    if special:
        assert float(y[0, 0, 1, 1]) == 0.0 and torch.isnan(y.view(-1)[0]) and float(g_z[0, 0, 1, 1]) == 0.0
        return
    # the class sums: n_class float64 additions of exactly converted float32 values in some order, then cpp - 1 more
    rc, cc = classes(o.H, o.W, dev)
    cls = (rc[:, None] * 3 + cc[None, :]).reshape(-1)
    gz64 = g_z.double().reshape(o.B, o.Co, -1)
    want_T = torch.zeros(o.B, o.Co, 9, dtype=torch.float64, device=dev).index_add_(2, cls, gz64)
    mag = torch.zeros(o.B, o.Co, 9, dtype=torch.float64, device=dev).index_add_(2, cls, gz64.abs())
    n_class = torch.bincount(cls, minlength=9).double()
    bound = (n_class + 8) * U64 * mag
    err = (g_T.reshape(o.B, o.Co, 9) - want_T).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert bool((g_T.reshape(o.B, o.Co, 9)[:, :, n_class == 0] == 0).all())          # a class without pixels sums to zero
    # g_z not wanted: the same sums; g_T not wanted: the same g_z
    only_T = aspp.fold_backward(g, y, o.scale, want_z=False)
    only_z = aspp.fold_backward(g, y, o.scale, want_T=False)
    assert only_T[0] is None and torch.equal(only_T[1], g_T) and only_z[1] is None and torch.equal(only_z[0], g_z)


@pytest.mark.parametrize("name", ["vector_interior", "no_interior", "one_element", "two_blocks"])
def test_all_ones_give_the_tap_counts(name, dev):
    from halo_amd import aspp
    B, Co, H, W, Cg, _ = CASES[name]
    ones = lambda *s: torch.ones(s, device=dev)
    T = aspp.fold_table(ones(Co, CX + Cg, 3, 3), ones(B, Cg, 1, 1), CX)
    counts = torch.tensor([[4., 6., 4.], [6., 9., 6.], [4., 6., 4.]], device=dev)
    assert torch.equal(T, (Cg * counts).expand(B, Co, 3, 3))
    y = aspp.fold_forward(torch.zeros(B, Co, H, W, device=dev), T, ones(Co), torch.zeros(Co, device=dev))
    want = Cg * F.conv2d(ones(1, 1, H, W), ones(1, 1, 3, 3), padding=1)               # the taps inside the map, per pixel
    assert torch.equal(y, want.expand(B, Co, H, W))
    g_z, g_T = aspp.fold_backward(ones(B, Co, H, W), y, ones(Co))
    pixels = torch.tensor([[1, W - 2, 1], [H - 2, (H - 2) * (W - 2), H - 2], [1, W - 2, 1]], device=dev, dtype=torch.float64)
    assert torch.equal(g_z, ones(B, Co, H, W)) and torch.equal(g_T, pixels.expand(B, Co, 3, 3))


def test_repeated_calls_and_a_side_stream_give_the_same_bits(dev):
    from halo_amd import aspp
    o = operands("five_blocks_offset", dev)
    z, g = _at_offset(o.z, o.off), _at_offset(o.g, o.off)

    def run():
        T = aspp.fold_table(o.w, o.v, CX)
        y = aspp.fold_forward(z, T, o.scale, o.shift)
        return (T, y) + aspp.fold_backward(g, y, o.scale)
    first, second = run(), run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for t1, t2, t3 in zip(first, second, third):
        assert torch.equal(t1, t2) and torch.equal(t1, t3)


def _stage(dev, B=2, Cx=3, Cg=4, Co=5, H=5, W=8, seed=0, layout="dense"):
    """operands of the operator, drawn on the CPU (so that the float64 side is the same on every machine) and moved to dev.
    layout: v dense, a channel slice of a wider tensor behind a storage offset ("slice"), or one image's row expanded over the
    batch ("expand": stride 0, Cg elements of storage)"""
    gen = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(Cx + Cg, Co, 3, padding=1, bias=False)
    bn = R.FrozenBatchNorm2d(Co)
    with torch.no_grad():
        conv.weight.copy_(0.3 * torch.randn(conv.weight.shape, generator=gen))
        bn.weight.copy_(0.25 + 1.5 * torch.rand(Co, generator=gen))
        bn.bias.copy_(0.4 * torch.randn(Co, generator=gen))
        bn.running_mean.copy_(0.5 * torch.randn(Co, generator=gen))
        bn.running_var.copy_(0.3 + 1.5 * torch.rand(Co, generator=gen))
    p, v, g = torch.randn(B, Cx, H, W, generator=gen), torch.randn(B, Cg, 1, 1, generator=gen), torch.randn(B, Co, H, W, generator=gen)
    v = v.to(dev)
    if layout == "slice":
        wide = torch.randn(B, Cg + 3, 1, 1, generator=gen).to(dev)
        wide[:, 1:Cg + 1] = v
        v = wide.requires_grad_(True)[:, 1:Cg + 1]                 # a view of a leaf: gradients are taken for the view itself
        assert not v.is_contiguous() and v.storage_offset() == 1
    elif layout == "expand":
        v = v[:1].clone().requires_grad_(True).expand(B, -1, -1, -1)
        assert v.stride(0) == 0 and v.untyped_storage().nbytes() == 4 * Cg
    return p.to(dev), v, g.to(dev), conv.to(dev), bn.to(dev)


def test_needs_input_grad_and_the_saved_tensors(dev):
    """which outputs the binding is asked for under every combination of needs (the weight's gradient needs g_z too: the conv's own
    weight gradient), no launch when nothing is needed, and nothing of the concatenation's or the broadcast's size is kept"""
    from halo_amd import _lib, aspp
    p, v, g, conv, bn = _stage(dev)
    B, Cx, H, W = p.shape
    Cg = v.shape[1]
    assert aspp.pool_fold_fallback_reason(p, v, conv, bn) is None
    L = _lib.lib()
    real, asked = L.halo_pool_fold_affine_relu_bwd, []

    def counted(*args):
        asked.append((args[3].value is not None, args[4].value is not None))
        return real(*args)
    L.halo_pool_fold_affine_relu_bwd = counted
    try:
        full = None
        for needs in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, True, False)):
            p.requires_grad_(needs[0]), v.requires_grad_(needs[1]), conv.weight.requires_grad_(needs[2])
            kept = []
            with torch.autograd.graph.saved_tensors_hooks(lambda t: (kept.append(tuple(t.shape)), t)[1], lambda t: t):
                y = aspp.pooled_bottleneck(p, v, conv, bn)
            for shape in kept:
                n = int(np.prod(shape))
                assert shape != (B, Cx + Cg, H, W) and n not in (B * (Cx + Cg) * H * W, B * Cg * H * W), (needs, kept)
            assert tuple(y.shape) in kept                                          # the hook sees what the operator keeps
            wanted = [t for t, n in zip((p, v, conv.weight), needs) if n]
            before = len(asked)
            grads = torch.autograd.grad(y, wanted, g)
            assert asked[before:] == [(needs[0] or needs[2], needs[1] or needs[2])], (needs, asked[before:])
            if full is None:
                full = grads
            else:                                                                  # the same values whichever are asked for
                for t, t0 in zip(grads, [f for f, n in zip(full, needs) if n]):
                    assert t.shape == t0.shape and torch.allclose(t, t0, rtol=1e-4, atol=1e-5)
        # the stock statement does keep the concatenation: the hook would have seen it
        kept = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (kept.append(tuple(t.shape)), t)[1], lambda t: t):
            aspp.torch_statement(p, v, conv, bn)
        assert (B, Cx + Cg, H, W) in kept
        # nothing needed: the function's backward launches nothing
        n, before = len(asked), dict(aspp.launches)
        scale, _ = aspp.cached_scale_shift(bn)
        ctx = types.SimpleNamespace(saved_tensors=(y.detach(), v.detach(), conv.weight.detach(), scale), Cx=Cx,
                                    needs_input_grad=(False, False, False, False, False, False))
        assert aspp._PoolFoldFn.backward(ctx, g) == (None,) * 6 and len(asked) == n and aspp.launches == before
        p.requires_grad_(False), v.requires_grad_(False), conv.weight.requires_grad_(False)
        y0 = aspp.pooled_bottleneck(p, v, conv, bn)
        with torch.no_grad():
            y1 = aspp.pooled_bottleneck(p, v, conv, bn)
            part = aspp.main_weight(conv, Cx)
            assert aspp.main_weight(conv, Cx) is part                              # the contiguous slice is kept ...
            conv.weight.mul_(2.0)
            assert aspp.main_weight(conv, Cx) is not part                          # ... until the weight's version moves
            conv.weight.mul_(0.5)
        assert not y0.requires_grad and torch.equal(y0, y1) and torch.equal(y0, y.detach()) and len(asked) == n
    finally:
        L.halo_pool_fold_affine_relu_bwd = real
        conv.weight.requires_grad_(True)


STAGE_SEED = {"dense": 1, "slice": 1, "expand": 1}


@pytest.mark.parametrize("layout", ["dense", "slice", "expand"])
def test_operator_against_float64_of_the_stock_statement(layout, dev):
    """pooled_bottleneck at mixed signs against the float64 CPU evaluation of the stock statement: the forward bound of the head test,
    and the three gradients within their term counts times u times the absolute-value evaluation, outside the ReLU's band.  A v
    that is a strided slice or a batch-expanded row is served like the dense one (the operator reads a dense copy of it), and
    torch_statement over the same operands on the device lies within twice the forward bound."""
    from halo_amd import aspp
    p, v, g, conv, bn = _stage(dev, seed=STAGE_SEED[layout], layout=layout)
    p.requires_grad_(True)
    if layout == "dense":
        v.requires_grad_(True)
    assert v.is_contiguous() == (layout == "dense") and aspp.pool_fold_fallback_reason(p, v, conv, bn) is None
    y = aspp.pooled_bottleneck(p, v, conv, bn)
    got = torch.autograd.grad(y, [p, v, conv.weight], g)
    B, Cx, H, W = p.shape
    c64 = lambda t: t.detach().cpu().double()
    p64, v64, W64 = c64(p).requires_grad_(True), c64(v).requires_grad_(True), c64(conv.weight).requires_grad_(True)
    scale, shift = (c64(t) for t in aspp.cached_scale_shift(bn))
    x64 = torch.cat([p64, v64.expand(-1, -1, H, W)], 1)
    pre = F.conv2d(x64, W64, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    mag = F.conv2d(x64.detach().abs(), W64.detach().abs(), padding=1) * scale.abs().view(1, -1, 1, 1)
    bound = (9 * x64.shape[1] + 12) * U * mag
    assert bool(((c64(y) - pre.detach().clamp_min(0)).abs() <= bound).all())
    with torch.no_grad():
        assert bool(((c64(aspp.torch_statement(p, v, conv, bn)) - c64(y)).abs() <= 2 * bound).all())
    assert bool((pre.detach().abs() > bound).all()), "a pre-activation inside the forward bound: pick another seed"
    want = torch.autograd.grad(pre.clamp_min(0), [p64, v64, W64], c64(g))
    gz = (c64(g) * (pre.detach() > 0) * scale.view(1, -1, 1, 1)).abs()
    Wa, xa = W64.detach().abs(), x64.detach().abs()
    gx_mag = F.conv_transpose2d(gz, Wa, padding=1)                                   # sum_{o,k} |W| |g_z|
    gw_mag = torch.autograd.grad(F.conv2d(xa, Wa.requires_grad_(True), padding=1), Wa, gz)[0]     # sum_{b,pixels} |g_z| |x|
    Co = W64.shape[0]
    # g_p: g_z's rounding and the 9 Co products of the conv's backward; g_v: g_z's rounding, the float64 sums, one final rounding;
    # g_W: g_z's rounding and B H W products for the pyramid's slice, as g_v for the pooled slice
    terms_W = torch.cat([torch.full((Cx,), B * H * W + 1.0), torch.full((v.shape[1],), 3.0)]).double().view(1, -1, 1, 1)
    bounds = ((9 * Co + 1) * U * gx_mag[:, :Cx], 3 * U * gx_mag[:, Cx:].sum((2, 3), keepdim=True), terms_W * U * gw_mag)
    for name, t, t64, b in zip(("g_p", "g_v", "g_W"), got, want, bounds):
        ratio = float(((c64(t) - t64).abs() / b).max())
        print("%s: max |delta| / bound %.3f" % (name, ratio))
        assert ratio <= 1.0, name


# ---------------------------------------------------------------- the hook on a stand-in v3+ head

class Block(nn.Module):
    """DepthwiseSeparableConv2d's attribute names and layout"""

    def __init__(self, cin, cout, d, norm):
        super().__init__()
        self.depthwise_conv = nn.Conv2d(cin, cin, 3, 1, d, d, groups=cin, bias=False)
        self.depthwise_bn = norm(cin)
        self.depthwise_activate = nn.ReLU(inplace=True)
        self.pointwise_conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.pointwise_bn = norm(cout)
        self.pointwise_activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.depthwise_activate(self.depthwise_bn(self.depthwise_conv(x)))
        return self.pointwise_activate(self.pointwise_bn(self.pointwise_conv(x)))


class FusedBlock(Block):
    pass


def _norm(n):
    """scale = weight in (0.5, 1.5), shift = bias of both signs, both exact: running_var = 1, running_mean = 0"""
    bn = R.FrozenBatchNorm2d(n)
    bn.weight.copy_(0.5 + torch.rand(n))
    bn.bias.copy_(0.5 * torch.randn(n))
    return bn


class _Head(nn.Module):
    """a stand-in v3+ hyperbolic head: channels 16 / 8 / 8, the reference's attribute names, dilations and block layout"""

    def __init__(self, block, C=16, K=5, top=16, mid=8, low=8):
        super().__init__()
        from halo_amd.core.utils.hyperbolic import HyperMapper, HyperMLR
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(top, mid, 1, bias=False), _norm(mid), nn.ReLU(inplace=True))] + [
            block(top, mid, d, _norm) for d in (6, 12, 18)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(top, mid, 1, bias=False), _norm(mid), nn.ReLU(inplace=True))
        self.bottleneck = nn.Sequential(nn.Conv2d(5 * mid, mid, 3, padding=1, bias=False), _norm(mid), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(low, 6, 1, bias=False), _norm(6), nn.ReLU(inplace=True))
        self.decoder = nn.Sequential(block(mid + 6, mid, 1, _norm), block(mid, mid, 1, _norm))
        self.conv_reduce = nn.Conv2d(mid, C, 1)
        self.mapper = HyperMapper(c=1.0)
        self.conv_seg = HyperMLR(C, K, c=1.0)
        for m in self.modules():                                     # positive weights: see the module docstring
            if isinstance(m, nn.Conv2d):
                m.weight.data = (torch.rand(m.weight.shape) * 2.0 + 0.01) / m.weight[0].numel()


def _layer(x, mx, nx, w, bn, terms, worst, **kw):
    """float64 conv + frozen norm + ReLU with the running bound: (out, magnitude >= out, term count); `worst` collects
    min |pre| / (N u m) over the ReLU's inputs"""
    scale, shift = bn.weight.double().view(1, -1, 1, 1), bn.bias.double().view(1, -1, 1, 1)
    pre = F.conv2d(x, w, **kw) * scale + shift
    m = F.conv2d(mx, w.detach().abs(), **kw) * scale.abs() + shift.abs()
    n = nx + terms + 2
    worst.append(float((pre.detach().abs() / (n * U * m)).min()))
    return pre.clamp_min(0), m, n


def _stock64(head, top):
    """the stock statements of the head from its input to the bottleneck's ReLU in float64 on the CPU, plain torch, with the
    magnitudes and term counts of the module docstring"""
    worst = []
    w = lambda conv: conv.weight.detach().double().requires_grad_(True)
    weights, pyramid, mags, counts = {}, [], [], []
    b0 = head.parallel_branches[0]
    weights["b0"] = w(b0[0])
    out = _layer(top, top.detach(), 0, weights["b0"], b0[1], 16, worst)
    pyramid.append(out[0]), mags.append(out[1]), counts.append(out[2])
    for i, blk in enumerate(list(head.parallel_branches)[1:]):
        d = blk.depthwise_conv.dilation[0]
        weights["dw%d" % i], weights["pw%d" % i] = w(blk.depthwise_conv), w(blk.pointwise_conv)
        h, mh, nh = _layer(top, top.detach(), 0, weights["dw%d" % i], blk.depthwise_bn, 9, worst, padding=d, dilation=d, groups=top.shape[1])
        out = _layer(h, mh, nh, weights["pw%d" % i], blk.pointwise_bn, 16, worst)
        pyramid.append(out[0]), mags.append(out[1]), counts.append(out[2])
    mean = top.mean((2, 3), keepdim=True)
    weights["global"] = w(head.global_branch[1])
    v, mv, nv = _layer(mean, mean.detach(), top.shape[2] * top.shape[3] + 1, weights["global"], head.global_branch[2], 16, worst)
    H, W = top.shape[2:]
    weights["bottleneck"] = w(head.bottleneck[0])
    x = torch.cat(pyramid + [F.interpolate(v, size=(H, W), mode="bilinear", align_corners=True)], dim=1)
    mx = torch.cat(mags + [mv.expand(-1, -1, H, W)], dim=1)
    bn = head.bottleneck[1]
    scale, shift = bn.weight.double().view(1, -1, 1, 1), bn.bias.double().view(1, -1, 1, 1)
    pre = F.conv2d(x, weights["bottleneck"], padding=1) * scale + shift
    return types.SimpleNamespace(pre=pre, y=pre.clamp_min(0), x=x, mx=mx, v=v, mv=mv, mean=mean, weights=weights, worst=worst,
                                 n_p=max(counts), n_v=nv, scale=scale)


def _capture(head, feats):
    """(the head's outputs, the pyramid / pooled map / output of each call of the folded operator, the outputs of head.bottleneck)"""
    from halo_amd import aspp
    calls, outs = [], []
    real = aspp.fused_pooled_bottleneck

    def spy(p, v, conv, bn):
        y = real(p, v, conv, bn)
        calls.append((p, v, y))
        return y
    aspp.fused_pooled_bottleneck = spy
    hook = head.bottleneck.register_forward_hook(lambda m, i, o: outs.append((i[0], o)))
    try:
        return head(feats), calls, outs
    finally:
        aspp.fused_pooled_bottleneck = real
        hook.remove()


def _forward_bound(p, v, conv, bn):
    """((9 (Cx + Cg) + 12) u |scale| sum |W| |x|, the float64 stock pre-activation) from the device's own pyramid and pooled map"""
    from halo_amd.norm import cached_scale_shift
    c64 = lambda t: t.detach().cpu().double()
    x = torch.cat([c64(p), c64(v).expand(-1, -1, p.shape[2], p.shape[3])], 1)
    W = c64(conv.weight)
    scale, shift = (c64(t).view(1, -1, 1, 1) for t in cached_scale_shift(bn))        # the float32 pair the device pass reads
    pre = F.conv2d(x, W, padding=1) * scale + shift
    return (9 * x.shape[1] + 12) * U * F.conv2d(x.abs(), W.abs(), padding=1) * scale.abs(), pre


HEAD_SEED = 5


def _heads(dev, *classes_and_blocks):
    torch.manual_seed(HEAD_SEED)
    with torch.no_grad():
        heads = [cls(block) for cls, block in classes_and_blocks]
    for h in heads[1:]:
        h.load_state_dict(heads[0].state_dict())
    feats = {"low": torch.rand(2, 8, 12, 16), "out": torch.rand(2, 16, 6, 8)}
    return heads, feats


def test_marked_head_against_float64_of_the_stock_statements(dev):
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import use_folded_image_pooling

    class Marked(_Head):
        forward = v3plus_hyper_forward

    class NoForward(_Head):
        def forward(self, x):
            return x

    with pytest.raises(TypeError):
        use_folded_image_pooling(NoForward)
    assert use_folded_image_pooling(Marked) is Marked and use_folded_image_pooling(Marked) is Marked
    assert not hasattr(_Head, "_halo_folded_image_pooling")
    (cpu_head,), feats = _heads(dev, (Marked, Block))
    keys = list(cpu_head.state_dict())

    # float64, CPU, plain torch: values, magnitudes, and the precondition on every ReLU of the stage
    top64 = feats["out"].double().requires_grad_(True)
    ref = _stock64(cpu_head, top64)
    assert min(ref.worst) > 1.0, "a pre-activation within its forward bound of zero: pick another HEAD_SEED (%s)" % ref.worst
    Cin = ref.x.shape[1]
    fwd_bound = (9 * Cin + 12) * U * F.conv2d(ref.mx, ref.weights["bottleneck"].detach(), padding=1) * ref.scale
    # at the bottleneck the inputs carry their own errors: N_p u m_x through the conv, on top of the stage's own bound
    assert bool((ref.pre.detach().abs() > fwd_bound * (1 + ref.n_v / (9 * Cin + 12))).all()), "bottleneck pre-activation inside the bound: pick another HEAD_SEED"
    g64 = torch.rand(ref.y.shape).double()                            # the float32 gradient both sides are given
    names = ("global", "bottleneck")
    want = torch.autograd.grad(ref.y, [top64] + [ref.weights[n] for n in names], g64)

    head = cpu_head.to(dev).train()
    top = feats["out"].to(dev).requires_grad_(True)
    (out, embed), calls, outs = _capture(head, {"low": feats["low"].to(dev), "out": top})
    assert len(calls) == 1 and len(outs) == 0                        # the operator ran, the bottleneck module did not
    p, v, y = calls[0]
    assert tuple(p.shape) == (2, 32, 6, 8) and tuple(v.shape) == (2, 8, 1, 1) and out.shape[1] == 5
    # forward: against the stock statement in float64 over the device's own pyramid and pooled map
    bound, pre = _forward_bound(p, v, head.bottleneck[0], head.bottleneck[1])
    ratio = float(((y.detach().cpu().double() - pre.clamp_min(0)).abs() / bound).max())
    print("forward: max |delta| / bound %.3f" % ratio)
    assert ratio <= 1.0
    got = torch.autograd.grad(y, [top, head.global_branch[1].weight, head.bottleneck[0].weight], g64.float().to(dev))
    c64 = lambda t: t.detach().cpu().double()
    # the bounds of the module docstring; every quantity below is a sum of non-negative terms
    gz = (g64 * (ref.pre.detach() > 0) * ref.scale)
    Wb = ref.weights["bottleneck"].detach()
    Cx = p.shape[1]
    Wtmp = Wb.clone().requires_grad_(True)
    gW_x, = torch.autograd.grad(F.conv2d(ref.x.detach(), Wtmp, padding=1), Wtmp, gz)               # sum g_z x
    Wtmp = Wb.clone().requires_grad_(True)
    gW_m, = torch.autograd.grad(F.conv2d(ref.mx.detach(), Wtmp, padding=1), Wtmp, gz)              # sum g_z m_x
    n_pix = top.shape[0] * top.shape[2] * top.shape[3]
    bound_W = torch.cat([(n_pix + 2) * U * gW_x[:, :Cx] + ref.n_p * U * gW_m[:, :Cx],
                         3 * U * gW_x[:, Cx:] + ref.n_v * U * gW_m[:, Cx:]], dim=1)
    assert ref.n_p == 29 and ref.n_v == 67
    checks = (("head input", got[0], want[0], 97 * U * want[0]),
              ("global_branch weight", got[1], want[1], 55 * U * want[1]),
              ("bottleneck weight, pyramid slice", got[2][:, :Cx], want[2][:, :Cx], bound_W[:, :Cx]),
              ("bottleneck weight, pooled slice", got[2][:, Cx:], want[2][:, Cx:], bound_W[:, Cx:]))
    assert torch.allclose(want[2], gW_x, rtol=1e-12, atol=0)
    worst = {}
    for name, t, t64, b in checks:
        assert bool((t64 >= 0).all()) and bool((b >= 0).all()), name
        delta = (c64(t) - t64).abs()
        assert bool((delta[b == 0] == 0).all()), name                 # a ReLU inactive in every image: an exact zero on both sides
        worst[name] = float((delta[b > 0] / b[b > 0]).max())
        print("%s: max |delta| / bound %.3f" % (name, worst[name]))
    assert all(r <= 1.0 for r in worst.values()), worst
    assert list(head.state_dict()) == keys


def test_marked_head_under_the_other_hooks(dev):
    """use_device_resize, use_fused_depthwise, use_fused_decoder_front and fuse_norm_relu_pairs on both heads, in two orders: the
    marked head's bottleneck output against the unmarked head's within twice the forward bound (each lies within one of the exact
    value), over bit-equal inputs"""
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import (fuse_norm_relu_pairs, fused_v3plus_hyper_forward, use_device_resize, use_folded_image_pooling,
                                use_fused_decoder_front, use_fused_depthwise, use_fused_feature_reweighting)
    use_fused_depthwise(FusedBlock)

    class Other(_Head):
        forward = v3plus_hyper_forward

    class Marked(_Head):
        forward = v3plus_hyper_forward

    class MarkedFirst(_Head):
        forward = v3plus_hyper_forward

    use_device_resize(Other), use_fused_decoder_front(Other)
    use_device_resize(Marked), use_fused_decoder_front(Marked), use_folded_image_pooling(Marked)
    use_folded_image_pooling(MarkedFirst), use_fused_feature_reweighting(MarkedFirst), use_fused_decoder_front(MarkedFirst), use_device_resize(MarkedFirst)
    assert MarkedFirst.forward is fused_v3plus_hyper_forward and not hasattr(Other, "_halo_folded_image_pooling")
    (other, marked, first), feats = _heads(dev, (Other, FusedBlock), (Marked, FusedBlock), (MarkedFirst, FusedBlock))
    keys = list(other.state_dict())
    feats = {k: t.to(dev) for k, t in feats.items()}
    res = {}
    for tag, head in (("other", other), ("marked", marked), ("first", first)):
        head = head.to(dev).train()
        assert fuse_norm_relu_pairs(head) >= 4
        for grad in (True, False):
            with torch.set_grad_enabled(grad):
                (o, e), calls, outs = _capture(head, feats)
            if tag == "other":
                assert len(calls) == 0 and len(outs) == 1
                res[tag, grad] = (outs[0][1].detach(), o.detach(), e.detach(), outs[0][0].detach())
            else:
                assert len(calls) == 1 and len(outs) == 0
                res[tag, grad] = (calls[0][2].detach(), o.detach(), e.detach(), calls[0][0].detach(), calls[0][1].detach())
        assert list(head.state_dict()) == keys
    for grad in (True, False):
        y0, o0, e0, x0 = res["other", grad]
        for tag in ("marked", "first"):
            y1, o1, e1, p1, v1 = res[tag, grad]
            assert torch.equal(x0[:, :p1.shape[1]], p1) and torch.equal(x0[:, p1.shape[1]:], v1.expand(-1, -1, 6, 8))
            bound, _ = _forward_bound(p1, v1, marked.bottleneck[0], marked.bottleneck[1])
            ratio = float(((y1.cpu().double() - y0.cpu().double()).abs() / (2 * bound)).max())
            print("%s, grad %s: max |marked - unmarked| / (2 x bound) %.3f" % (tag, grad, ratio))
            assert ratio <= 1.0
            assert o1.shape == o0.shape and e1.shape == e0.shape and bool(torch.isfinite(o1).all())
        assert torch.equal(res["marked", grad][0], res["first", grad][0])
    # under autograd the marked head trains: every parameter of the stage receives a gradient
    marked.zero_grad()
    out, embed = marked(feats)
    (out.square().mean() + embed.sum()).backward()
    for n, prm in marked.named_parameters():
        if n.startswith(("parallel_branches", "global_branch", "bottleneck")):
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().sum()) > 0, n
