"""The fused front of the v3+ decoder on the device (halo_upcat_* of halo_dwconv.hip through halo_amd.dwconv /
halo_amd.hooks.use_fused_decoder_front).

"Composition" below is depthwise_bn_relu(torch.cat([bilinear_resize(a, (H, W)), s], 1), conv, bn) under its own autograd: the
operator promises its bits for y, g_a, g_s and g_w (same taps and bilerp as halo_bilinear_upsample, same 9-term order, same work
split, same float64 weight sums).  Independently of that conv, y, g_s and g_w are held to the derived bounds of
tests/test_gpu_dwconv.py (u = 2^-24) against the three stock modules evaluated in float64 over x_ref = cat(bilinear_resize(a), s):

  forward  15u (|scale| sum_k |w_k| |x_k| + |bias| + |running_mean scale|), the ReLU mask equal outside the band |pre_64| <= bound
  g_x      15u |scale| sum_k |w_k| |g mask| with the device's mask;  g_w  8u sum |gp| |x| per tap
  g_a      (small cases) A^T g_x[:, :Ca] with A^T the resize backward in float64 over the float32 taps (adjoint64 of
           tests/resize_ref.py, held to the float32 adjoint in tests/test_dwconv_geometry_host.py): the bound is the propagated
           error of g_up, A^T bx, plus the resize backward's own 2 (n + 8) u A^T(|g_x| + bx) of tests/test_gpu_resize.py

The synthetic cases of tests/dwconv_cases.py are drawn on the CPU and copied: tests/test_dwconv_geometry_host.py proves what each
reaches of the work split and of DwUpSrc's source-row reuse, and that at most 1e-4 of their elements lie within 4 x the forward
bound of zero -- the cap on the band that is asserted for them here.
"""
import gc
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dwconv_cases as K
import dwconv_ref as R
import resize_ref as Z

pytestmark = pytest.mark.gpu
U = R.U

# name: (a's shape, s's shape)
CASES = {
    "vector_two_bands": ((2, 3, 9, 10), (2, 2, 37, 40)),        # 16-byte route, two 16-row bands + halo, non-integer scales, plane split at Ca
    "one_column": ((1, 2, 5, 7), (1, 1, 18, 23)),               # W % 4 != 0
    "single_cell": ((2, 2, 1, 1), (2, 1, 8, 8)),                # in_size = 1: both taps coincide
    "identity": ((1, 2, 6, 8), (1, 2, 6, 8)),                   # h = H, w = W
}
SYNTHETIC = {"syn_" + name: shapes for name, (shapes, _) in K.DECODER.items()}
ALL = dict(CASES, **SYNTHETIC)
HEAD = ((2, 512, 80, 160), (2, 48, 160, 320))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def operands(shapes, dev, seed=0):
    """quarter-step a, s and g, random conv weights, a frozen norm with a negative weight entry and a shift that leaves the last
    channel of each operand with more than one channel all-zero behind the ReLU"""
    (B, Ca, h, w), (_, Cs, H, W) = shapes
    C = Ca + Cs
    gen = torch.Generator(device=dev).manual_seed(seed)
    q = lambda shape: torch.randint(-8, 9, shape, device=dev, generator=gen).float() / 4
    a, s, g = q(shapes[0]), q(shapes[1]), q((B, C, H, W))
    conv = nn.Conv2d(C, C, 3, 1, 1, 1, groups=C, bias=False).to(dev)
    bn = R.FrozenBatchNorm2d(C).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device=dev, generator=gen))
        bn.weight.copy_(0.25 + 1.5 * torch.rand(C, device=dev, generator=gen))
        bn.weight[0] = -0.75
        bn.bias.copy_(0.4 * torch.randn(C, device=dev, generator=gen) + 0.1)
        if Ca > 1:
            bn.bias[Ca - 1] = -1e4
        if Cs > 1:
            bn.bias[C - 1] = -1e4
        bn.running_mean.copy_(0.5 * torch.randn(C, device=dev, generator=gen) + 0.2)
        bn.running_var.copy_(0.3 + 1.5 * torch.rand(C, device=dev, generator=gen))
    return a, s, g, conv, bn


def synthetic_operands(name, dev):
    """a synthetic case's operands, drawn on the CPU by tests/dwconv_cases.py and copied"""
    c = K.decoder(name)
    conv, bn = R.modules(c, dev)
    a, s, g = (torch.from_numpy(c[k]).to(dev) for k in ("a", "s", "g"))
    return a, s, g, conv, bn


def fused(a, s, g, conv, bn):
    from halo_amd.dwconv import upcat_fallback_reason, upsample_cat_depthwise_bn_relu
    assert upcat_fallback_reason(a, s, conv, bn) is None
    ar, sr = a.detach().requires_grad_(True), s.detach().requires_grad_(True)
    y = upsample_cat_depthwise_bn_relu(ar, sr, conv, bn)
    assert type(y.grad_fn).__name__.startswith("_UpCatDepthwiseBnReluFn")
    return (y.detach(),) + torch.autograd.grad(y, [ar, sr, conv.weight], g)


def composition(a, s, g, conv, bn):
    from halo_amd.dwconv import depthwise_bn_relu, fallback_reason
    from halo_amd.resize import bilinear_resize
    ar, sr = a.detach().clone().requires_grad_(True), s.detach().clone().requires_grad_(True)
    x = torch.cat([bilinear_resize(ar, tuple(s.shape[2:])), sr], 1)
    assert fallback_reason(x, conv, bn) is None
    y = depthwise_bn_relu(x, conv, bn)
    return (y.detach(),) + torch.autograd.grad(y, [ar, sr, conv.weight], g)


_small = {}


def small(name, dev):
    """(operands, the composition's y, g_a, g_s, g_w) of a small case: computed once, shared, never written"""
    if name not in _small:
        if name in SYNTHETIC:
            ops = synthetic_operands(name[4:], dev)
        else:
            ops = operands(CASES[name], dev, seed=sorted(CASES).index(name) + 1)
        _small[name] = (ops, composition(*ops))
    return _small[name]


def assert_same_bits(got, want):
    for name, t1, t2 in zip(("y", "g_a", "g_s", "g_w"), got, want):
        assert t1.shape == t2.shape and torch.equal(t1, t2), name


def offset_view(t):
    """the same values in storage that starts 4 bytes off a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 1, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("name", sorted(CASES) + list(SYNTHETIC))
def test_bits_of_the_composition(dev, name):
    ops, want = small(name, dev)
    y = want[0]
    Ca = ALL[name][0][1]
    dead = (y == 0).all(dim=3).all(dim=2).all(dim=0)
    assert bool(dead[Ca - 1]) and not bool(dead[:Ca].all()) and not bool(dead[Ca:].all())     # a dead channel, live ones from a and from s
    assert_same_bits(fused(*ops), want)


def test_unaligned_operands_take_the_one_column_route_with_the_same_bits(dev):
    """s and g as storage-offset views: the 16-byte route is not taken (W % 4 == 0 all the same).  y, g_a and g_s do not depend on
    the route at all.  g_w's float64 partial sums are split differently (one column per thread), so they may differ from the
    composition's in the last bits of a float64; the float32 rounding hides that except with probability ~2^-29 per entry, and the
    operands are seeded."""
    (a, s, g, conv, bn), want = small("vector_two_bands", dev)
    assert_same_bits(fused(a, offset_view(s), offset_view(g), conv, bn), want)
    # a non-contiguous a and s are made contiguous
    wide = torch.zeros(s.shape[:3] + (2 * s.shape[3],), device=dev)
    wide[..., ::2] = s
    assert not wide[..., ::2].is_contiguous()
    assert_same_bits(fused(a.transpose(2, 3).contiguous().transpose(2, 3), wide[..., ::2], g, conv, bn), want)


def against_float64(a, s, g, conv, bn, got, band_cap=None, g_a=False):
    """y, g_s and g_w against the stock modules in float64 over x_ref (float32, the device resize's own values); g_a against the
    float64 adjoint of the resize applied to the float64 data gradient, on the CPU"""
    from halo_amd.resize import bilinear_resize
    y, ga, gs, gw = got
    Ca, (B, C, H, W) = a.shape[1], y.shape
    v = lambda t: t.double().reshape(1, C, 1, 1)
    with torch.no_grad():
        x = torch.cat([bilinear_resize(a, (H, W)), s], 1).double()
        w64 = conv.weight.double()
        scale = bn.weight.double() / bn.running_var.double().sqrt()
        pre = F.conv2d(x, w64, None, 1, 1, 1, C) * v(scale) + v(bn.bias.double() - bn.running_mean.double() * scale)
        mag = F.conv2d(x.abs(), w64.abs(), None, 1, 1, 1, C)
        bound = 15 * U * (v(scale).abs() * mag + v(bn.bias).abs() + v(bn.running_mean.double() * scale).abs())
        del mag
        err = (y.double() - pre.clamp(min=0)).abs()
        print(tuple(y.shape), "forward: max err / bound", float((err / bound).max()))
        assert bool((err <= bound).all())
        band = pre.abs() <= bound
        print(tuple(y.shape), "band fraction", float(band.double().mean()))
        if band_cap is not None:
            assert float(band.double().mean()) <= band_cap
        mask = y > 0
        assert bool(((mask == (pre > 0)) | band).all())
        del pre, err, band, bound
        gm = g.double() * mask
        gp = gm * v(scale)
        wflip = w64.flip(2, 3)                                          # the adjoint: a correlation with the mirrored taps
        rx = F.conv2d(gp, wflip, None, 1, 1, 1, C)
        bx = 15 * U * v(scale).abs() * F.conv2d(gm.abs(), wflip.abs(), None, 1, 1, 1, C)
        ex = (gs.double() - rx[:, Ca:]).abs()
        print(tuple(y.shape), "g_s: max err / bound", float((ex / bx[:, Ca:].clamp(min=1e-300)).max()))
        assert bool((ex <= bx[:, Ca:]).all())
        if g_a:
            (h, w), u = a.shape[2:], 2.0 ** -24
            r, b = rx[:, :Ca].cpu().numpy(), bx[:, :Ca].cpu().numpy()
            want = Z.adjoint64(r, h, w)
            ba = Z.adjoint64(b, h, w) + 2 * (Z.terms_bound(h, w, H, W) + 8) * u * Z.adjoint64(np.abs(r) + b, h, w)
            ea = np.abs(ga.cpu().numpy().astype(np.float64) - want)
            print(tuple(y.shape), "g_a: max err / bound", float((ea / np.maximum(ba, 1e-300)).max()))
            assert (ea <= ba).all()
            assert (ea[ba == 0] == 0).all() and (ba[:, Ca - 1] == 0).all()     # the dead a-channel: exactly 0
        del rx, bx, ex, gm
        xp = F.pad(x, (1, 1, 1, 1))
        rw, bw = torch.zeros(C, 9, dtype=torch.float64, device=y.device), torch.zeros(C, 9, dtype=torch.float64, device=y.device)
        for k in range(9):
            xs = xp[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W]
            rw[:, k] = (gp * xs).sum(dim=(0, 2, 3))
            bw[:, k] = 8 * U * (gp.abs() * xs.abs()).sum(dim=(0, 2, 3))
        ew = (gw.double().reshape(C, 9) - rw).abs()
        print(tuple(y.shape), "g_w: max err / bound", float((ew / bw.clamp(min=1e-300)).max()))    # a dead channel has bw = 0
        assert bool((ew <= bw).all())


def test_small_case_against_float64(dev):
    ops, _ = small("vector_two_bands", dev)
    against_float64(*ops, fused(*ops), g_a=True)


@pytest.mark.parametrize("name", sorted(set(CASES) - {"vector_two_bands"}) + list(SYNTHETIC))
def test_every_other_small_case_against_float64(dev, name):
    ops, _ = small(name, dev)
    against_float64(*ops, fused(*ops), band_cap=1e-4 if name in SYNTHETIC else None, g_a=True)


def test_head_shape_bits_and_float64(dev):
    """a (2, 512, 80, 160), s (2, 48, 160, 320): the composition's bits, then the float64 bounds"""
    ops = operands(HEAD, dev, seed=11)
    got = fused(*ops)
    want = composition(*ops)
    assert_same_bits(got, want)
    del want
    against_float64(*ops, got)


def test_what_is_kept_for_the_backward(dev):
    from halo_amd.dwconv import scale_shift, upsample_cat_depthwise_bn_relu
    nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
    a, s, g, conv, bn = operands(((2, 64, 40, 80), (2, 8, 80, 160)), dev, seed=3)
    ar, sr = a.requires_grad_(True), s.requires_grad_(True)
    y = upsample_cat_depthwise_bn_relu(ar, sr, conv, bn)
    saved = y.grad_fn.saved_tensors
    scale, _ = scale_shift(bn)
    assert nbytes(*saved) <= nbytes(a, s, y, conv.weight, scale)
    assert not any(t.shape[1:] == y.shape[1:] and t.data_ptr() != y.data_ptr() for t in saved if t.dim() == 4)   # nothing of x's size but y
    x_bytes = y.numel() * 4
    del y, saved

    def peak(fn):
        fn()                                                        # warm: the library, the allocator's blocks
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    p_fused = peak(lambda: fused(a, s, g, conv, bn) and None)
    p_comp = peak(lambda: composition(a, s, g, conv, bn) and None)
    print("peak above the operands: fused %.1f MiB, composition %.1f MiB, x_ref %.1f MiB" % (p_fused / 2**20, p_comp / 2**20, x_bytes / 2**20))
    assert p_comp - p_fused >= x_bytes


def test_needs_input_grad_combinations(dev, monkeypatch):
    from halo_amd import _lib
    from halo_amd.dwconv import _UpCatDepthwiseBnReluFn, scale_shift, upsample_cat_depthwise_bn_relu
    (a, s, g, conv, bn), (_, ga0, gs0, gw0) = small("vector_two_bands", dev)
    L = _lib.lib()
    calls = {"w": 0, "x": 0, "r": 0}
    seen = []
    real_w, real_x, real_r = L.halo_upcat_dwconv3x3_affine_relu_bwd_weight, L.halo_upcat_dwconv3x3_affine_relu_bwd_data, L.halo_bilinear_upsample_bwd
    monkeypatch.setattr(L, "halo_upcat_dwconv3x3_affine_relu_bwd_weight", lambda *p: (calls.__setitem__("w", calls["w"] + 1), real_w(*p))[1])
    monkeypatch.setattr(L, "halo_upcat_dwconv3x3_affine_relu_bwd_data",
                        lambda *p: (calls.__setitem__("x", calls["x"] + 1), seen.append((p[4] is not None, p[5] is not None)), real_x(*p))[2])
    monkeypatch.setattr(L, "halo_bilinear_upsample_bwd", lambda *p: (calls.__setitem__("r", calls["r"] + 1), real_r(*p))[1])
    w = conv.weight
    try:
        w.requires_grad_(False)                                         # a frozen conv.weight launches no weight pass
        ar = a.detach().requires_grad_(True)
        y = upsample_cat_depthwise_bn_relu(ar, s.detach(), conv, bn)    # only a
        (ga,) = torch.autograd.grad(y, [ar], g)
        assert calls == {"w": 0, "x": 1, "r": 1} and seen[-1] == (True, False) and torch.equal(ga, ga0)
        sr = s.detach().requires_grad_(True)
        y = upsample_cat_depthwise_bn_relu(a.detach(), sr, conv, bn)    # only s: no g_up, no resize backward
        (gs,) = torch.autograd.grad(y, [sr], g)
        assert calls == {"w": 0, "x": 2, "r": 1} and seen[-1] == (False, True) and torch.equal(gs, gs0)
        ga, gs = torch.autograd.grad(upsample_cat_depthwise_bn_relu(ar, sr, conv, bn), [ar, sr], g, allow_unused=True)
        assert calls == {"w": 0, "x": 3, "r": 2} and torch.equal(ga, ga0) and torch.equal(gs, gs0)
        w.requires_grad_(True)                                          # only conv.weight: no data pass
        y = upsample_cat_depthwise_bn_relu(a.detach(), s.detach(), conv, bn)
        (gw,) = torch.autograd.grad(y, [w], g)
        assert calls == {"w": 1, "x": 3, "r": 2} and torch.equal(gw, gw0)
        # unrequested gradients are None: the function's backward under each combination of needs
        scale, _ = scale_shift(bn)
        for needs in ((True, False, False), (False, True, False), (False, False, True), (False, False, False), (True, True, True)):
            ctx = types.SimpleNamespace(saved_tensors=(a, s, y.detach(), w.detach(), scale), needs_input_grad=needs + (False, False))
            grads = _UpCatDepthwiseBnReluFn.backward(ctx, g)
            assert len(grads) == 5 and tuple(t is not None for t in grads) == needs + (False, False)
            for t, t0 in zip(grads, (ga0, gs0, gw0)):
                assert t is None or torch.equal(t, t0)
        assert calls == {"w": 3, "x": 6, "r": 4}
        w.requires_grad_(False)                                         # none
        y = upsample_cat_depthwise_bn_relu(a.detach(), s.detach(), conv, bn)
        assert not y.requires_grad
        with torch.no_grad():
            y2 = upsample_cat_depthwise_bn_relu(ar, sr, conv, bn)
        assert not y2.requires_grad and torch.equal(y, y2) and calls == {"w": 3, "x": 6, "r": 4}
    finally:
        w.requires_grad_(True)
        w.grad = None


def test_repeated_calls_and_a_side_stream_give_the_same_bits(dev):
    ops, want = small("vector_two_bands", dev)
    first = fused(*ops)
    second = fused(*ops)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = fused(*ops)
    side.synchronize()
    for t1, t2, t3, t0 in zip(first, second, third, want):
        assert torch.equal(t1, t2) and torch.equal(t1, t3) and torch.equal(t1, t0)


# ---------------------------------------------------------------- the hook on a stand-in v3+ head

class Block(nn.Module):
    """DepthwiseSeparableConv2d's attribute names and layout"""

    def __init__(self, cin, cout, d, norm, bias=False):
        super().__init__()
        self.depthwise_conv = nn.Conv2d(cin, cin, 3, 1, d, d, groups=cin, bias=bias)
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


def _frozen(n):
    bn = R.FrozenBatchNorm2d(n)
    bn.weight.copy_(0.5 + torch.rand(n))
    bn.bias.copy_(0.2 * torch.randn(n) + 0.1)
    bn.running_mean.copy_(0.3 * torch.randn(n))
    bn.running_var.copy_(0.5 + torch.rand(n))
    return bn


class _Head(nn.Module):
    """a stand-in v3+ hyperbolic head at reduced width: the reference's attribute names, dilations and block layout"""

    def __init__(self, block, C=64, K=5, top=32, mid=16, low=8, front_bias=False):
        super().__init__()
        from halo_amd.core.utils.hyperbolic import HyperMapper, HyperMLR
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(top, mid, 1, bias=False), _frozen(mid), nn.ReLU(inplace=True))] + [
            block(top, mid, d, _frozen) for d in (6, 12, 18)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(top, mid, 1, bias=False), _frozen(mid), nn.ReLU(inplace=True))
        self.bottleneck = nn.Sequential(nn.Conv2d(5 * mid, mid, 3, padding=1, bias=False), _frozen(mid), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(low, 6, 1, bias=False), _frozen(6), nn.ReLU(inplace=True))
        self.decoder = nn.Sequential(block(mid + 6, mid, 1, _frozen, bias=front_bias), block(mid, mid, 1, _frozen))
        self.conv_reduce = nn.Conv2d(mid, C, 1)
        self.mapper = HyperMapper(c=1.0)
        self.conv_seg = HyperMLR(C, K, c=1.0)


def _served_calls(head, feats):
    """(the head's outputs, how often the fused operator's autograd function ran)"""
    from halo_amd import dwconv
    n = []
    real = dwconv._UpCatDepthwiseBnReluFn.apply
    dwconv._UpCatDepthwiseBnReluFn.apply = lambda *args: (n.append(1), real(*args))[1]
    try:
        return head(feats), len(n)
    finally:
        dwconv._UpCatDepthwiseBnReluFn.apply = real


def test_hooked_head(dev):
    from halo_amd.core.models.classifier import _tail_modules, hyper_head_tail, v3plus_hyper_forward
    from halo_amd.hooks import use_device_resize, use_fused_decoder_front, use_fused_depthwise
    use_fused_depthwise(FusedBlock)

    class Plain(_Head):
        forward = v3plus_hyper_forward

    class Pair(_Head):                                # use_device_resize + use_fused_depthwise (through FusedBlock)
        forward = v3plus_hyper_forward

    class Front(_Head):                               # the same, and the decoder front in one pass
        forward = v3plus_hyper_forward

    class NoForward(_Head):
        def forward(self, x):
            return x

    with pytest.raises(TypeError):
        use_fused_decoder_front(NoForward)
    use_device_resize(Pair), use_device_resize(Front)
    assert use_fused_decoder_front(Front) is Front and use_fused_decoder_front(Front) is Front
    assert not hasattr(Pair, "_halo_fused_decoder_front") and not hasattr(_Head, "_halo_fused_decoder_front")

    torch.manual_seed(21)
    with torch.no_grad():
        ref, front, plain = Pair(FusedBlock), Front(FusedBlock), Plain(Block)
    keys = list(ref.state_dict())
    front.load_state_dict(ref.state_dict()), plain.load_state_dict(ref.state_dict())
    ref, front, plain = ref.to(dev).train(), front.to(dev).train(), plain.to(dev).train()
    feats = {"low": torch.randn(2, 8, 48, 80, device=dev), "out": torch.randn(2, 32, 24, 40, device=dev)}

    # marked against use_device_resize + use_fused_depthwise: the same bits, in training ...  Most parameters are convolution
    # weights whose backward is MIOpen's: it is asked for its deterministic algorithms, so that equal operands give equal bits.
    res, arriving = {}, {}
    names = [n for n, p in front.named_parameters() if p.requires_grad]
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for tag, head in (("front", front), ("ref", ref), ("ref again", ref)):
            got = arriving[tag] = []
            hooks = [m.register_forward_hook(lambda m, i, o, got=got: o.register_hook(lambda g: got.append(g.clone())) and None)
                     for m in (head.bottleneck, head.shortcut)]
            (out, embed), served = _served_calls(head, feats)
            for hk in hooks:
                hk.remove()
            assert served == (1 if tag == "front" else 0)
            loss = out.square().mean() + embed.sum()
            res[tag] = (out.detach(), embed.detach(), torch.autograd.grad(loss, [p for p in head.parameters() if p.requires_grad]))
    finally:
        torch.backends.cudnn.deterministic = was
    assert torch.equal(res["front"][0], res["ref"][0]) and torch.equal(res["front"][1], res["ref"][1])
    # the gradients arriving at the shortcut's and the bottleneck's outputs, and the front's own weight gradient
    assert len(arriving["front"]) == len(arriving["ref"]) == 2
    for g1, g2 in zip(arriving["front"], arriving["ref"]):
        assert torch.equal(g1, g2)
    k = names.index("decoder.0.depthwise_conv.weight")
    assert torch.equal(res["front"][2][k], res["ref"][2][k])
    assert len(res["front"][2]) == len(res["ref"][2]) == len(names) > 10
    for n, g1, g2, g3 in zip(names, res["front"][2], res["ref"][2], res["ref again"][2]):
        if not torch.equal(g1, g2) or not torch.equal(g2, g3):
            print("%s: max |front - ref| %.3g, max |ref - ref again| %.3g, max |ref| %.3g"
                  % (n, float((g1 - g2).abs().max()), float((g2 - g3).abs().max()), float(g2.abs().max())))
    for g1, g2 in zip(res["front"][2], res["ref"][2]):
        assert torch.equal(g1, g2)
    # ... and under no_grad
    front.eval(), ref.eval(), plain.eval()
    with torch.no_grad():
        (o1, e1), served = _served_calls(front, feats)
        o2, e2 = ref(feats)
    assert served == 1 and torch.equal(o1, o2) and torch.equal(e1, e2)
    assert list(front.state_dict()) == keys and all(torch.equal(v, ref.state_dict()[k]) for k, v in front.state_dict().items())

    # an unmarked class runs the two forwards' statements as they were before they shared a helper
    with torch.no_grad():
        low, top = feats["low"], feats["out"]
        pyramid = [branch(top) for branch in plain.parallel_branches]
        pyramid.append(F.interpolate(plain.global_branch(top), size=top.shape[2:], mode="bilinear", align_corners=True))
        fused_ = plain.bottleneck(torch.cat(pyramid, dim=1))
        fused_ = F.interpolate(fused_, size=low.shape[2:], mode="bilinear", align_corners=True)
        dec = plain.decoder(torch.cat([fused_, plain.shortcut(low)], dim=1))
        dec = plain.conv_reduce(dec)
        want_out, want_embed = hyper_head_tail(dec, *_tail_modules(plain), size=(96, 160), resize_embed=False, resize=None)
        got_out, got_embed = plain(feats, size=(96, 160))
    assert torch.equal(got_out, want_out) and torch.equal(got_embed, want_embed)

    # a decoder[0] outside the envelope (a conv bias): a marked head takes the unmarked statements
    torch.manual_seed(22)
    with torch.no_grad():
        biased, twin = Front(Block, front_bias=True), Pair(Block, front_bias=True)
    twin.load_state_dict(biased.state_dict())
    biased, twin = biased.to(dev).eval(), twin.to(dev).eval()
    with torch.no_grad():
        (o1, e1), served = _served_calls(biased, feats)
        o2, e2 = twin(feats)
    assert served == 0 and torch.equal(o1, o2) and torch.equal(e1, e2)
