"""Fused depthwise conv + frozen norm + ReLU on the device (halo_dwconv.hip through halo_amd.dwconv / halo_amd.hooks) against the
float64 evaluation of tests/golden/dwconv.npz (the reference's own modules, tests/golden/make_dwconv_fixtures.py; every channel
through tests/dwconv_ref.py, which tests/test_dwconv_host.py holds to the stored channels).  u = 2^-24; the bounds are derived:

  forward  |pre_dev - pre_64| <= 15u (|scale| sum_k |w_k| |x_k| + |bias| + |running_mean scale|): gamma_9 for the 9-term sum in any
           order, one rounding each for * scale and + shift, the roundings of scale and shift themselves; checked through y (ReLU
           is 1-Lipschitz)
  mask     [y_dev > 0] == [pre_64 > 0] outside the band |pre_64| <= bound, which may hold at most 1e-4 of the elements
  g_x      against the float64 adjoint with the device's own mask: 15u |scale| sum_k |w_k| |g mask| at the gathered positions
  g_w      against the float64 sum with the same mask: 8u sum |gp| |x| per tap
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dwconv_ref as R

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def run(c, dev, x=None):
    from halo_amd.dwconv import depthwise_bn_relu, fallback_reason
    conv, bn = R.modules(c, dev)
    x = (torch.from_numpy(c["x"]).to(dev) if x is None else x).requires_grad_(True)
    assert fallback_reason(x, conv, bn) is None
    y = depthwise_bn_relu(x, conv, bn)
    gx, gw = torch.autograd.grad(y, [x, conv.weight], torch.from_numpy(c["g"]).to(dev))
    return y.detach(), gx, gw


@pytest.mark.parametrize("name", R.case_names())
def test_fixture(dev, name):
    c = R.load(name)
    y, gx, gw = (t.cpu().numpy().astype(np.float64) for t in run(c, dev))
    pre, bound = R.forward(c)
    err = np.abs(y - np.maximum(pre, 0))
    print(name, "forward: max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (y[bound == 0] == np.maximum(pre, 0)[bound == 0]).all()
    band = np.abs(pre) <= bound
    print(name, "band fraction", float(band.mean()))
    assert band.mean() <= 1e-4
    mask = y > 0
    assert (mask == (pre > 0))[~band].all()
    rx, bx = R.grad_x(c, mask)
    ex = np.abs(gx - rx)
    print(name, "g_x: max err / bound", float((ex[bx > 0] / bx[bx > 0]).max()))
    assert (ex <= bx).all()
    rw, bw = R.grad_w(c, mask)
    ew = np.abs(gw - rw)
    print(name, "g_w: max err / bound", float((ew[bw > 0] / bw[bw > 0]).max()))
    assert (ew <= bw).all()


@pytest.mark.parametrize("shape,d", [((2, 3, 9, 12), 1), ((1, 2, 7, 8), 3), ((2, 2, 6, 7), 2), ((1, 2, 3, 4), 5)])
def test_all_ones_counts_the_taps(dev, shape, d):
    """all-ones g, w, scale and zero shift over positive x: g_x is the in-bounds tap count (1 to 9) exactly and g_w the exact sums of
    x over the shifted windows (x in multiples of 1/4: every float32 and float64 sum is exact)"""
    from halo_amd.dwconv import depthwise_bn_relu
    B, C, H, W = shape
    rng = np.random.default_rng(5)
    xn = rng.integers(1, 9, shape).astype(np.float32) / 4
    conv = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False).to(dev)
    bn = R.FrozenBatchNorm2d(C).to(dev)
    with torch.no_grad():
        conv.weight.fill_(1.0)
    x = torch.from_numpy(xn).to(dev).requires_grad_(True)
    y = depthwise_bn_relu(x, conv, bn)
    gx, gw = torch.autograd.grad(y, [x, conv.weight], torch.ones_like(y))
    ones = np.ones((H, W))
    count = sum(R.shifted(ones, dy * d, dx * d) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert count.min() >= 1 and count.max() <= 9
    assert np.array_equal(gx.cpu().numpy(), np.broadcast_to(count, shape).astype(np.float32))
    want = np.stack([R.shifted(xn.astype(np.float64), (k // 3 - 1) * d, (k % 3 - 1) * d).sum(axis=(0, 2, 3)) for k in range(9)], 1)
    assert np.array_equal(gw.cpu().numpy().reshape(C, 9), want.astype(np.float32))
    assert np.array_equal(y.detach().cpu().numpy().astype(np.float64), sum(
        R.shifted(xn.astype(np.float64), dy * d, dx * d) for dy in (-1, 0, 1) for dx in (-1, 0, 1)))


def test_repeated_calls_and_a_side_stream_give_the_same_bits(dev):
    c = R.load("d6")
    a = run(c, dev)
    b = run(c, dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s = run(c, dev)
    side.synchronize()
    for t1, t2, t3 in zip(a, b, s):
        assert torch.equal(t1, t2) and torch.equal(t1, t3)


def test_strided_x_and_the_scalar_route_agree_with_the_vector_route(dev):
    """a non-contiguous x is made contiguous; a plane whose rows start off 16 bytes runs the one-column route: the same bits"""
    c = R.load("d6")
    base = run(c, dev)
    x = torch.from_numpy(c["x"]).to(dev)
    wide = torch.zeros(x.shape[:3] + (2 * x.shape[3],), device=dev)
    wide[..., ::2] = x
    strided = wide[..., ::2]
    assert not strided.is_contiguous()
    for t1, t2 in zip(base, run(c, dev, strided)):
        assert torch.equal(t1, t2)
    # the same operands at a 4-byte offset: the library takes the one-column route
    from halo_amd import _lib
    L = _lib.lib()
    conv, bn = R.modules(c, dev)
    from halo_amd.dwconv import scale_shift
    scale, shift = scale_shift(bn)
    buf = torch.zeros(x.numel() + 1, device=dev)
    buf[1:] = x.reshape(-1)
    out = torch.zeros(x.numel() + 1, device=dev)
    B, C, H, W = x.shape
    _lib.check(L.halo_dwconv3x3_affine_relu_fwd(_lib.ptr(buf[1:]), _lib.ptr(conv.weight), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(out[1:]),
                                                B, C, H, W, c["d"], _lib.stream_ptr(dev)))
    assert torch.equal(out[1:].reshape(x.shape), base[0]) and float(out[0]) == 0.0


def test_needs_input_grad_combinations(dev, monkeypatch):
    from halo_amd import _lib
    from halo_amd.dwconv import depthwise_bn_relu
    c = R.load("w13_d2")
    _, gx0, gw0 = run(c, dev)
    L = _lib.lib()
    calls = {"w": 0, "x": 0}
    real_w, real_x = L.halo_dwconv3x3_affine_relu_bwd_weight, L.halo_dwconv3x3_affine_relu_bwd_data
    monkeypatch.setattr(L, "halo_dwconv3x3_affine_relu_bwd_weight", lambda *a: (calls.__setitem__("w", calls["w"] + 1), real_w(*a))[1])
    monkeypatch.setattr(L, "halo_dwconv3x3_affine_relu_bwd_data", lambda *a: (calls.__setitem__("x", calls["x"] + 1), real_x(*a))[1])
    g = torch.from_numpy(c["g"]).to(dev)
    conv, bn = R.modules(c, dev)
    conv.weight.requires_grad_(False)                                   # a frozen conv.weight launches no weight pass
    x = torch.from_numpy(c["x"]).to(dev).requires_grad_(True)
    (gx,) = torch.autograd.grad(depthwise_bn_relu(x, conv, bn), [x], g)
    assert calls == {"w": 0, "x": 1} and torch.equal(gx, gx0)
    conv.weight.requires_grad_(True)                                    # x needs none: no data pass
    (gw,) = torch.autograd.grad(depthwise_bn_relu(x.detach(), conv, bn), [conv.weight], g)
    assert calls == {"w": 1, "x": 1} and torch.equal(gw, gw0)
    with torch.no_grad():
        y = depthwise_bn_relu(x, conv, bn)
    assert not y.requires_grad and calls == {"w": 1, "x": 1}


@pytest.mark.parametrize("shape,d", [((2, 512, 160, 320), 1), ((2, 2048, 80, 160), 18)])
def test_head_shapes_against_float64_on_the_device(dev, shape, d):
    """the stock statements in float64 on the device at two head shapes, the same bounds (gradients with the device's mask)"""
    from halo_amd.dwconv import depthwise_bn_relu
    B, C, H, W = shape
    gen = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(shape, device=dev, generator=gen)
    g = torch.randn(shape, device=dev, generator=gen)
    conv = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False).to(dev)
    bn = R.FrozenBatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(0.25 + 1.5 * torch.rand(C, device=dev, generator=gen))
        bn.bias.copy_(0.4 * torch.randn(C, device=dev, generator=gen) + 0.1)
        bn.running_mean.copy_(0.5 * torch.randn(C, device=dev, generator=gen) + 0.2)
        bn.running_var.copy_(0.3 + 1.5 * torch.rand(C, device=dev, generator=gen))
    xr = x.clone().requires_grad_(True)
    y = depthwise_bn_relu(xr, conv, bn)
    gx, gw = torch.autograd.grad(y, [xr, conv.weight], g)
    y = y.detach()
    v = lambda t: t.double().reshape(1, C, 1, 1)
    with torch.no_grad():
        w64 = conv.weight.double()
        scale = bn.weight.double() / bn.running_var.double().sqrt()
        pre = F.conv2d(x.double(), w64, None, 1, d, d, C) * v(scale) + v(bn.bias.double() - bn.running_mean.double() * scale)
        mag = F.conv2d(x.double().abs(), w64.abs(), None, 1, d, d, C)
        bound = 15 * U * (v(scale).abs() * mag + v(bn.bias).abs() + v(bn.running_mean.double() * scale).abs())
        del mag
        err = (y.double() - pre.clamp(min=0)).abs()
        print(shape, d, "forward: max err / bound", float((err / bound).max()))
        assert bool((err <= bound).all())
        band = pre.abs() <= bound
        print(shape, d, "band fraction", float(band.double().mean()))
        assert float(band.double().mean()) <= 1e-4
        mask = y > 0
        assert bool(((mask == (pre > 0)) | band).all())
        del pre, err, band, bound
        gm = g.double() * mask
        gp = gm * v(scale)
        wflip = w64.flip(2, 3)                                          # the adjoint: a correlation with the mirrored taps
        rx = F.conv2d(gp, wflip, None, 1, d, d, C)
        bx = 15 * U * v(scale).abs() * F.conv2d(gm.abs(), wflip.abs(), None, 1, d, d, C)
        ex = (gx.double() - rx).abs()
        print(shape, d, "g_x: max err / bound", float((ex / bx.clamp(min=1e-300)).max()))
        assert bool((ex <= bx).all())
        del rx, bx, ex, gm
        xp = F.pad(x.double(), (d, d, d, d))
        rw, bw = torch.zeros(C, 9, dtype=torch.float64, device=dev), torch.zeros(C, 9, dtype=torch.float64, device=dev)
        for k in range(9):
            xs = xp[:, :, (k // 3) * d:(k // 3) * d + H, (k % 3) * d:(k % 3) * d + W]
            rw[:, k] = (gp * xs).sum(dim=(0, 2, 3))
            bw[:, k] = 8 * U * (gp.abs() * xs.abs()).sum(dim=(0, 2, 3))
        ew = (gw.double().reshape(C, 9) - rw).abs()
        print(shape, d, "g_w: max err / bound", float((ew / bw.clamp(min=1e-300)).max()))   # a channel that never fires has bw = 0
        assert bool((ew <= bw).all())


class Block(nn.Module):
    """DepthwiseSeparableConv2d's attribute names and constructor arguments (in, out, kernel 3, stride 1, padding d, dilation d, no
    bias, norm_layer)"""

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


def _frozen(n):
    bn = R.FrozenBatchNorm2d(n)
    bn.weight.copy_(0.5 + torch.rand(n))
    bn.bias.copy_(0.2 * torch.randn(n) + 0.1)
    bn.running_mean.copy_(0.3 * torch.randn(n))
    bn.running_var.copy_(0.5 + torch.rand(n))
    return bn


class _Head(nn.Module):
    """a stand-in v3+ hyperbolic head at reduced width: the reference's attribute names, dilations (1, 6, 12, 18) and block layout"""

    def __init__(self, block, C=64, K=5, top=32, mid=16, low=8):
        super().__init__()
        from halo_amd.core.utils.hyperbolic import HyperMapper, HyperMLR
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(top, mid, 1, bias=False), _frozen(mid), nn.ReLU(inplace=True))] + [
            block(top, mid, d, _frozen) for d in (6, 12, 18)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(top, mid, 1, bias=False), _frozen(mid), nn.ReLU(inplace=True))
        self.bottleneck = nn.Sequential(nn.Conv2d(5 * mid, mid, 3, padding=1, bias=False), _frozen(mid), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(low, 6, 1, bias=False), _frozen(6), nn.ReLU(inplace=True))
        self.decoder = nn.Sequential(block(mid + 6, mid, 1, _frozen), block(mid, mid, 1, _frozen))
        self.conv_reduce = nn.Conv2d(mid, C, 1)
        self.mapper = HyperMapper(c=1.0)
        self.conv_seg = HyperMLR(C, K, c=1.0)


def near(a, b, tol):
    a, b = a.double(), b.double()
    assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-30), (float((a - b).abs().max()), float(b.abs().max()))


def test_hooked_head(dev):
    """A v3+ head whose five separable blocks run the fused forward against the same head unhooked, both float32 on the device.  Each
    fused block is held to 15u-scale bounds above; behind it lie the pointwise convolutions, the decoder, conv_reduce, expmap and
    HyperMLR, the same float32 statements on both sides, so the two heads are held to the bars the package already sets for two
    float32 evaluations of this tail (tests/test_gpu_hfr.py::test_hooked_head): 2e-5 of max|.| for the logits and the embedding, 5e-4
    of max|g| for every parameter gradient.  Eval-mode no_grad inference runs through the same path."""
    from halo_amd import dwconv
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import fused_dwsep_forward, use_fused_depthwise
    assert use_fused_depthwise(FusedBlock) is FusedBlock and FusedBlock.forward is fused_dwsep_forward
    assert FusedBlock._unfused_forward is Block.__dict__["forward"] and Block.forward is not fused_dwsep_forward

    class Head(_Head):
        forward = v3plus_hyper_forward

    torch.manual_seed(21)
    with torch.no_grad():
        a = Head(Block)
        b = Head(FusedBlock)
    b.load_state_dict(a.state_dict())
    a, b = a.to(dev).train(), b.to(dev).train()
    served = []
    real = dwconv._DepthwiseBnReluFn.apply
    feats = {"low": torch.randn(2, 8, 48, 80, device=dev), "out": torch.randn(2, 32, 24, 40, device=dev)}
    outs = {}
    for tag, head in (("fused", b), ("plain", a)):
        dwconv._DepthwiseBnReluFn.apply = lambda *args: (served.append(tag), real(*args))[1]
        try:
            out, embed = head(feats)
        finally:
            dwconv._DepthwiseBnReluFn.apply = real
        loss = out.square().mean() + embed.sum()
        outs[tag] = (out.detach(), embed.detach(), torch.autograd.grad(loss, [p for p in head.parameters() if p.requires_grad]))
    assert served == ["fused"] * 5                                       # all five blocks, and only the hooked head's
    (fo, fe, fg), (po, pe, pg) = outs["fused"], outs["plain"]
    near(fo, po, 2e-5)
    near(fe, pe, 2e-5)
    assert len(fg) == len(pg) > 10
    for x1, x2 in zip(fg, pg):
        near(x1, x2, 5e-4)
    a.eval(), b.eval()
    with torch.no_grad():
        o1, _ = b(feats)
        o2, _ = a(feats)
    near(o1, o2, 2e-5)
