"""The joint depthwise backward on the device (halo_joint_* of halo_dwconv.hip through halo_amd.dwconv's joint_backward keyword and
halo_amd.hooks.use_joint_depthwise_backward) against the two entries it replaces, bit for bit.

The contract (include/halo_hip.h) is the bits of halo_dwconv3x3_affine_relu_bwd_data / _bwd_weight (the front: halo_upcat_*) on the
same operands, so every comparison is torch.equal and nothing here has a tolerance; those entries are held to float64 by
tests/test_gpu_dwconv.py, tests/test_gpu_dwconv_geometry.py and tests/test_gpu_decoder_front.py.  The operands are the cases of
tests/dwconv_cases.py, whose reach of the work split tests/test_dwconv_geometry_host.py proves.  The speed rule is switched off:
every shape runs the kernels."""
import numpy as np
import pytest
import torch

import dwconv_cases as K
import dwconv_ref as R

pytestmark = pytest.mark.gpu
GUARD = -777.0
PLAIN, UPCAT = "halo_joint_dwconv3x3_affine_relu_bwd", "halo_joint_upcat_dwconv3x3_affine_relu_bwd"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def rule_off(monkeypatch):
    from halo_amd import dwconv
    monkeypatch.setattr(dwconv, "JOINT_MIN_ELEMENTS", {k: 0 for k in dwconv.JOINT_MIN_ELEMENTS})


class Guarded:
    """an output of `shape` inside a buffer of GUARD values, `off` floats (0 or 1) behind a 16-byte boundary: one guard element in
    front and one behind (and the rest of the buffer) must come back unchanged"""

    def __init__(self, shape, dev, off=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 9,), GUARD, device=dev)
        self.lo = 4 + off
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 4 * off

    def intact(self):
        n = self.t.numel()
        return bool((self.buf[:self.lo] == GUARD).all()) and bool((self.buf[self.lo + n:] == GUARD).all())


def placed(t, off):
    """the same values in storage that starts 4 * off bytes behind a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 4, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


def workspace(need, dev):
    ws = torch.full((need // 8 + 4,), GUARD, dtype=torch.float64, device=dev)
    return ws, lambda: bool((ws[need // 8:] == GUARD).all())


def plain_operands(c, dev):
    """(g, y, x, w, scale) of a case on the device, y from the forward entry"""
    from halo_amd.dwconv import depthwise_bn_relu, fallback_reason, scale_shift
    conv, bn = R.modules(c, dev)
    x, g = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["g"]).to(dev)
    assert fallback_reason(x, conv, bn) is None
    with torch.no_grad():
        y = depthwise_bn_relu(x, conv, bn)
    return g, y, x, conv.weight.detach().contiguous(), scale_shift(bn)[0]


def parents(g, y, x, w, scale, d, dev, gx_off=0):
    """(g_x, g_w) of the two entries the joint pass replaces"""
    from halo_amd import _lib
    L = _lib.lib()
    B, C, H, W = x.shape
    st = _lib.stream_ptr(dev)
    gx = Guarded(x.shape, dev, gx_off)
    _lib.check(L.halo_dwconv3x3_affine_relu_bwd_data(_lib.ptr(g), _lib.ptr(y), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gx.t), B, C, H, W, d, st))
    need = L.halo_dwconv_workspace_bytes(B, C, H, W, d)
    ws, _ = workspace(need, dev)
    gw = torch.empty_like(w)
    _lib.check(L.halo_dwconv3x3_affine_relu_bwd_weight(_lib.ptr(g), _lib.ptr(y), _lib.ptr(x), _lib.ptr(scale), _lib.ptr(gw), B, C, H, W, d,
                                                       _lib.ptr(ws), need, st))
    return gx.t, gw


def joint(g, y, x, w, scale, d, dev, gx_off=0):
    """(g_x, g_w) of the joint entry, with the guards of both outputs and the workspace's tail checked"""
    from halo_amd import _lib
    L = _lib.lib()
    B, C, H, W = x.shape
    gx, gw = Guarded(x.shape, dev, gx_off), Guarded(w.shape, dev)
    need = L.halo_dwconv_workspace_bytes(B, C, H, W, d)
    ws, tail_intact = workspace(need, dev)
    _lib.check(getattr(L, PLAIN)(_lib.ptr(g), _lib.ptr(y), _lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gx.t), _lib.ptr(gw.t), B, C, H, W,
                                 d, _lib.ptr(ws), need, _lib.stream_ptr(dev)), PLAIN)
    assert gx.intact() and gw.intact() and tail_intact()
    return gx.t, gw.t


@pytest.mark.parametrize("name", list(K.PLAIN))
def test_entry_returns_the_bits_of_the_two_entries(dev, name):
    c = K.plain(name)
    ops = plain_operands(c, dev)
    gx0, gw0 = parents(*ops, c["d"], dev)
    gx1, gw1 = joint(*ops, c["d"], dev)
    assert torch.equal(gx1, gx0), "g_x"
    assert torch.equal(gw1, gw0), "g_w"
    assert bool((gx1[:, c["C"] - 1] == 0).all()) and bool((gw1[c["C"] - 1] == 0).all())      # the dead channel
    if gx1.numel() > 100:                                               # not equal for being all zero
        assert bool(gx1.abs().sum() > 0) and bool(gw1.abs().sum() > 0)


@pytest.mark.parametrize("name", list(K.PLAIN_OFFSET))
def test_every_operand_four_bytes_off_runs_the_one_column_route(dev, name):
    c = K.plain(name)
    g, y, x, w, scale = plain_operands(c, dev)
    aligned = parents(g, y, x, w, scale, c["d"], dev)
    g, y, x = (placed(t, 1) for t in (g, y, x))
    gx0, gw0 = parents(g, y, x, w, scale, c["d"], dev, gx_off=1)
    gx1, gw1 = joint(g, y, x, w, scale, c["d"], dev, gx_off=1)
    assert torch.equal(gx1, gx0) and torch.equal(gx1, aligned[0]), "g_x"
    assert torch.equal(gw1, gw0), "g_w"


@pytest.mark.parametrize("name", ["vec_d3_two_blocks", "vec_d1_five_lane_block"])
def test_only_g_x_misaligned(dev, name):
    """g, y and x aligned at W % 4 == 0, g_x 4 bytes off: the joint entry takes the one-column route.  g_x does not depend on the
    route; g_w is what bwd_weight returns on that route, which it takes for an x 4 bytes off."""
    c = K.plain(name)
    assert c["W"] % 4 == 0
    g, y, x, w, scale = plain_operands(c, dev)
    gx0, gw_vec = parents(g, y, x, w, scale, c["d"], dev)
    _, gw_col = parents(g, y, placed(x, 1), w, scale, c["d"], dev)
    gx1, gw1 = joint(g, y, x, w, scale, c["d"], dev, gx_off=1)
    assert torch.equal(gx1, gx0), "g_x"
    assert torch.equal(gw1, gw_col), "g_w"
    gx2, gw2 = joint(g, y, x, w, scale, c["d"], dev)                  # and aligned again: the 16-byte route's g_w
    assert torch.equal(gx2, gx0) and torch.equal(gw2, gw_vec)


# ---------------------------------------------------------------- the decoder front
def front_operands(name, dev):
    from halo_amd.dwconv import scale_shift, upcat_fallback_reason, upsample_cat_depthwise_bn_relu
    c = K.decoder(name)
    conv, bn = R.modules(c, dev)
    a, s, g = (torch.from_numpy(c[k]).to(dev) for k in ("a", "s", "g"))
    assert upcat_fallback_reason(a, s, conv, bn) is None
    with torch.no_grad():
        y = upsample_cat_depthwise_bn_relu(a, s, conv, bn)
    return (a, s, g, conv, bn), y, conv.weight.detach().contiguous(), scale_shift(bn)[0]


@pytest.mark.parametrize("name", list(K.DECODER))
def test_front_returns_the_bits_of_its_two_entries(dev, name):
    from halo_amd import _lib, dwconv
    (a, s, g, conv, bn), y, w, scale = front_operands(name, dev)
    L = _lib.lib()
    (B, Ca, h, wi), (_, Cs, H, W) = a.shape, s.shape
    st = _lib.stream_ptr(dev)
    need = L.halo_dwconv_workspace_bytes(B, Ca + Cs, H, W, 1)
    gup0, gs0, gw0 = torch.empty((B, Ca, H, W), device=dev), torch.empty_like(s), torch.empty_like(w)
    _lib.check(L.halo_upcat_dwconv3x3_affine_relu_bwd_data(_lib.ptr(g), _lib.ptr(y), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gup0), _lib.ptr(gs0),
                                                           B, Ca, Cs, H, W, st))
    ws0, _ = workspace(need, dev)
    _lib.check(L.halo_upcat_dwconv3x3_affine_relu_bwd_weight(_lib.ptr(g), _lib.ptr(y), _lib.ptr(a), _lib.ptr(s), _lib.ptr(scale), _lib.ptr(gw0),
                                                             B, Ca, Cs, h, wi, H, W, _lib.ptr(ws0), need, st))
    gup, gs, gw = Guarded((B, Ca, H, W), dev), Guarded(s.shape, dev), Guarded(w.shape, dev)
    ws, tail_intact = workspace(need, dev)
    _lib.check(getattr(L, UPCAT)(_lib.ptr(g), _lib.ptr(y), _lib.ptr(a), _lib.ptr(s), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gup.t), _lib.ptr(gs.t),
                                 _lib.ptr(gw.t), B, Ca, Cs, h, wi, H, W, _lib.ptr(ws), need, st), UPCAT)
    assert gup.intact() and gs.intact() and gw.intact() and tail_intact()
    assert torch.equal(gup.t, gup0), "g_up"
    assert torch.equal(gs.t, gs0), "g_s"
    assert torch.equal(gw.t, gw0), "g_w"
    # through the operator: every gradient, g_a behind the resize backward included, equals the operator's without the keyword
    got = {}
    for flag in (False, True):
        ar, sr = a.detach().requires_grad_(True), s.detach().requires_grad_(True)
        before = dict(dwconv.joint_launches)
        out = dwconv.upsample_cat_depthwise_bn_relu(ar, sr, conv, bn, joint_backward=flag)
        got[flag] = (out.detach(),) + torch.autograd.grad(out, [ar, sr, conv.weight], g)
        assert dwconv.joint_launches == dict(before, upcat=before["upcat"] + int(flag))
    for t0, t1, what in zip(got[False], got[True], ("y", "g_a", "g_s", "g_w")):
        assert torch.equal(t0, t1), what
    assert torch.equal(got[True][2], gs0) and torch.equal(got[True][3], gw0)


# ---------------------------------------------------------------- the operators, counted at the binding
def counted(monkeypatch, names):
    from halo_amd import _lib
    L = _lib.lib()
    calls = {n: 0 for n in names}
    for key, entry in names.items():
        real = getattr(L, entry)
        monkeypatch.setattr(L, entry, lambda *p, real=real, key=key: (calls.__setitem__(key, calls[key] + 1), real(*p))[1])
    return calls


def test_plain_operator_takes_the_joint_entry_only_for_both_gradients(dev, monkeypatch):
    from halo_amd import dwconv
    from halo_amd.dwconv import depthwise_bn_relu
    c = K.plain("vec_d2_working_second_block")
    g_, y_, x_, w_, scale = plain_operands(c, dev)
    gx0, gw0 = parents(g_, y_, x_, w_, scale, c["d"], dev)
    calls = counted(monkeypatch, {"j": PLAIN, "x": "halo_dwconv3x3_affine_relu_bwd_data", "w": "halo_dwconv3x3_affine_relu_bwd_weight"})
    conv, bn = R.modules(c, dev)
    before = dict(dwconv.joint_launches)
    x = x_.clone().requires_grad_(True)
    # what tests/test_gpu_dwconv.py::test_hooked_head leaves behind when it ran first: `apply` bound on the parent node's class
    dwconv._DepthwiseBnReluFn.apply = dwconv._DepthwiseBnReluFn.apply
    y = depthwise_bn_relu(x, conv, bn, joint_backward=True)
    assert type(y.grad_fn).__name__.startswith("_DepthwiseBnReluFn")
    gx, gw = torch.autograd.grad(y, [x, conv.weight], g_)
    assert calls == {"j": 1, "x": 0, "w": 0} and dwconv.joint_launches == dict(before, plain=before["plain"] + 1)
    assert torch.equal(gx, gx0) and torch.equal(gw, gw0)
    conv.weight.requires_grad_(False)                                   # x alone: bwd_data alone
    (gx,) = torch.autograd.grad(depthwise_bn_relu(x, conv, bn, joint_backward=True), [x], g_)
    assert calls == {"j": 1, "x": 1, "w": 0} and torch.equal(gx, gx0)
    conv.weight.requires_grad_(True)                                    # w alone: bwd_weight alone
    (gw,) = torch.autograd.grad(depthwise_bn_relu(x.detach(), conv, bn, joint_backward=True), [conv.weight], g_)
    assert calls == {"j": 1, "x": 1, "w": 1} and torch.equal(gw, gw0)
    with torch.no_grad():
        y = depthwise_bn_relu(x, conv, bn, joint_backward=True)
    assert not y.requires_grad and calls == {"j": 1, "x": 1, "w": 1}
    gx, gw = torch.autograd.grad(depthwise_bn_relu(x, conv, bn), [x, conv.weight], g_)       # the default: the two entries
    assert calls == {"j": 1, "x": 2, "w": 2} and torch.equal(gx, gx0) and torch.equal(gw, gw0)
    assert dwconv.joint_launches == dict(before, plain=before["plain"] + 1) and sorted(dwconv.launches) == ["multi_bwd", "multi_fwd"]


def test_front_operator_takes_the_joint_entry_only_for_all_three_gradients(dev, monkeypatch):
    from halo_amd import dwconv
    from halo_amd.dwconv import upsample_cat_depthwise_bn_relu as op
    (a, s, g, conv, bn), _, _, _ = front_operands("vector_two_blocks", dev)
    ar, sr = a.detach().requires_grad_(True), s.detach().requires_grad_(True)
    ga0, gs0, gw0 = torch.autograd.grad(op(ar, sr, conv, bn), [ar, sr, conv.weight], g)
    calls = counted(monkeypatch, {"j": UPCAT, "x": "halo_upcat_dwconv3x3_affine_relu_bwd_data", "w": "halo_upcat_dwconv3x3_affine_relu_bwd_weight",
                                  "r": "halo_bilinear_upsample_bwd"})
    before = dict(dwconv.joint_launches)
    dwconv._UpCatDepthwiseBnReluFn.apply = dwconv._UpCatDepthwiseBnReluFn.apply         # as tests/test_gpu_decoder_front.py leaves it
    ga, gs, gw = torch.autograd.grad(op(ar, sr, conv, bn, joint_backward=True), [ar, sr, conv.weight], g)
    assert calls == {"j": 1, "x": 0, "w": 0, "r": 1} and dwconv.joint_launches == dict(before, upcat=before["upcat"] + 1)
    assert torch.equal(ga, ga0) and torch.equal(gs, gs0) and torch.equal(gw, gw0)
    ga, gw = torch.autograd.grad(op(ar, s.detach(), conv, bn, joint_backward=True), [ar, conv.weight], g)      # a and w without s: the parents
    assert calls == {"j": 1, "x": 1, "w": 1, "r": 2} and torch.equal(ga, ga0) and torch.equal(gw, gw0)
    gs, gw = torch.autograd.grad(op(a.detach(), sr, conv, bn, joint_backward=True), [sr, conv.weight], g)      # s and w without a
    assert calls == {"j": 1, "x": 2, "w": 2, "r": 2} and torch.equal(gs, gs0) and torch.equal(gw, gw0)
    conv.weight.requires_grad_(False)
    try:
        ga, gs = torch.autograd.grad(op(ar, sr, conv, bn, joint_backward=True), [ar, sr], g)                   # a and s without w
        assert calls == {"j": 1, "x": 3, "w": 2, "r": 3} and torch.equal(ga, ga0) and torch.equal(gs, gs0)
    finally:
        conv.weight.requires_grad_(True)
    (gw,) = torch.autograd.grad(op(a.detach(), s.detach(), conv, bn, joint_backward=True), [conv.weight], g)   # w alone
    assert calls == {"j": 1, "x": 3, "w": 3, "r": 3} and torch.equal(gw, gw0)
    with torch.no_grad():
        y = op(ar, sr, conv, bn, joint_backward=True)
    assert not y.requires_grad and calls == {"j": 1, "x": 3, "w": 3, "r": 3}
    assert dwconv.joint_launches == dict(before, upcat=before["upcat"] + 1)


# ---------------------------------------------------------------- head shapes, repeats, a side stream
@pytest.mark.parametrize("shape,d", [((2, 512, 160, 320), 1), ((2, 2048, 80, 160), 18)])
def test_head_shapes(dev, shape, d):
    from halo_amd import _lib
    L = _lib.lib()
    B, C, H, W = shape
    gen = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(shape, device=dev, generator=gen)
    g = torch.randn(shape, device=dev, generator=gen)
    w = torch.randn((C, 1, 3, 3), device=dev, generator=gen)
    scale = 0.25 + 1.5 * torch.rand(C, device=dev, generator=gen)
    scale[0] = -0.75
    shift = 0.4 * torch.randn(C, device=dev, generator=gen)
    y = torch.empty_like(x)
    _lib.check(L.halo_dwconv3x3_affine_relu_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, C, H, W, d,
                                                _lib.stream_ptr(dev)))
    gx0, gw0 = parents(g, y, x, w, scale, d, dev)
    gx1, gw1 = joint(g, y, x, w, scale, d, dev)
    assert torch.equal(gx1, gx0), "g_x"
    assert torch.equal(gw1, gw0), "g_w"
    assert 0.2 < float((y > 0).float().mean()) < 0.8


def test_repeated_calls_and_a_side_stream_give_the_same_bits(dev):
    c = K.plain("scalar_d4_two_blocks")
    ops = plain_operands(c, dev)
    first = joint(*ops, c["d"], dev)
    second = joint(*ops, c["d"], dev)
    (fa, fs, fg, fconv, fbn), _, _, _ = front_operands("scalar_four_blocks", dev)

    def front():
        from halo_amd.dwconv import upsample_cat_depthwise_bn_relu as op
        ar, sr = fa.detach().requires_grad_(True), fs.detach().requires_grad_(True)
        return torch.autograd.grad(op(ar, sr, fconv, fbn, joint_backward=True), [ar, sr, fconv.weight], fg)
    f1, f2 = front(), front()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = joint(*ops, c["d"], dev)
        f3 = front()
    side.synchronize()
    for t1, t2, t3 in zip(first + f1, second + f2, third + f3):
        assert torch.equal(t1, t2) and torch.equal(t1, t3)


# ---------------------------------------------------------------- the hook
@pytest.fixture
def deterministic_convs():
    """most gradients of a block or a head are convolution backwards of MIOpen's: asked for its deterministic algorithms, equal
    operands give equal bits (as in tests/test_gpu_decoder_front.py::test_hooked_head)"""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _grads(out, leaves, g):
    return torch.autograd.grad(out, leaves, g, allow_unused=True)


def test_marked_block_returns_the_unmarked_blocks_bits(dev, deterministic_convs):
    from euclid_head_standin import Block
    from halo_amd import dwconv, hooks
    Fused = hooks.use_fused_depthwise(type("Fused", (Block,), {}))
    Joint = hooks.use_joint_depthwise_backward(hooks.use_fused_depthwise(type("Joint", (Block,), {})))
    for d, shape in ((1, (2, 6, 33, 348)), (3, (2, 6, 50, 176)), (2, (1, 6, 21, 45))):
        torch.manual_seed(d)
        with torch.no_grad():
            a, b = Fused(6, 5, d).to(dev), Joint(6, 5, d).to(dev)
        b.load_state_dict(a.state_dict())
        assert list(a.state_dict()) == list(b.state_dict())
        gen = torch.Generator(device=dev).manual_seed(d)
        x = torch.randn(shape, device=dev, generator=gen)
        g = torch.randn((shape[0], 5) + shape[2:], device=dev, generator=gen)
        res = []
        for m, add in ((a, 0), (b, 1)):
            before = dict(dwconv.joint_launches)
            xr = x.clone().requires_grad_(True)
            out = m(xr)
            res.append((out.detach(),) + _grads(out, [xr] + list(m.parameters()), g))
            assert dwconv.joint_launches == dict(before, plain=before["plain"] + add)
        assert len(res[0]) == len(res[1]) == 4
        for t0, t1 in zip(*res):
            assert torch.equal(t0, t1)


def test_marked_head_returns_the_unmarked_heads_bits(dev, deterministic_convs):
    """a stand-in Euclidean v3+ head under use_device_resize + use_fused_decoder_front with blocks under use_fused_depthwise, the
    head class and the block class marked against both unmarked: two pyramid blocks and decoder[1] take the plain joint entry,
    decoder[0]'s front the other one"""
    from euclid_head_standin import Block, EuclidHead
    from halo_amd import dwconv, hooks
    Fused = hooks.use_fused_depthwise(type("Fused", (Block,), {}))
    Joint = hooks.use_joint_depthwise_backward(hooks.use_fused_depthwise(type("Joint", (Block,), {})))

    def head_class(name):
        cls = hooks.use_v3plus_forward(type(name, (EuclidHead,), {}))
        return hooks.use_fused_decoder_front(hooks.use_device_resize(cls))
    Base, Marked = head_class("Base"), hooks.use_joint_depthwise_backward(head_class("Marked"))
    assert not hasattr(Base, "_halo_joint_depthwise_backward")
    torch.manual_seed(3)
    with torch.no_grad():
        base, marked = Base(Fused, p=0.0).to(dev).train(), Marked(Joint, p=0.0).to(dev).train()
    marked.load_state_dict(base.state_dict())
    assert list(base.state_dict()) == list(marked.state_dict())
    gen = torch.Generator(device=dev).manual_seed(4)
    out_, low_ = torch.randn(2, 24, 9, 12, device=dev, generator=gen), torch.randn(2, 12, 33, 48, device=dev, generator=gen)
    res = []
    for head, want in ((base, {"plain": 0, "upcat": 0}), (marked, {"plain": 3, "upcat": 1}), (base, {"plain": 0, "upcat": 0})):
        feats = {"out": out_.clone().requires_grad_(True), "low": low_.clone().requires_grad_(True)}
        before = dict(dwconv.joint_launches)
        out, dec = head(feats)
        loss = out.square().mean() + dec.mean()
        leaves = [feats["out"], feats["low"]] + [p for p in head.parameters() if p.requires_grad]
        res.append((out.detach(), dec.detach()) + torch.autograd.grad(loss, leaves))
        assert {k: dwconv.joint_launches[k] - before[k] for k in before} == want
    assert len(res[0]) == len(res[1]) > 12
    names = ["out", "decoder_out", "g_out", "g_low"] + [n for n, p in base.named_parameters() if p.requires_grad]
    for n, t0, t1, t2 in zip(names, *res):                               # the unmarked head twice: what a difference is measured against
        if not torch.equal(t0, t1) or not torch.equal(t0, t2):
            print("%s: max |unmarked - marked| %.3g, max |unmarked - unmarked again| %.3g, max |unmarked| %.3g"
                  % (n, float((t0 - t1).abs().max()), float((t0 - t2).abs().max()), float(t0.abs().max())))
    for n, t0, t1 in zip(names, res[0], res[1]):
        assert torch.equal(t0, t1), n
