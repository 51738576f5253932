"""The Euclidean DeepLab-v3+ head on the device: halo_amd.norm.norm_relu_dropout2d_pair over halo_dropout_pair_fwd / _bwd of
halo_norm.hip, and a stand-in head (tests/euclid_head_standin.py: the reference's attribute layout at small widths) under
halo_amd.hooks.use_v3plus_forward and the marks that accept it.

Every comparison is torch.equal: against the stock torch statements and their autograd on the same device under the same seed, or
against the package's own public operators composed by hand.  The kernels run the stock statements with their roundings, so no
tolerance is involved.  torch.equal does not tell -0.0 from +0.0.  Shapes: top 2 x 24 x 9 x 13, low 2 x 12 x 33 x 49 -- odd sizes,
ragged both ways, every operator's last chunk partial."""
import pytest
import torch
import torch.nn as nn

from euclid_head_standin import Block, EuclidHead, frozen

pytestmark = pytest.mark.gpu

# the operator's cases: (B, C, H, W).  The first three have planes that are no multiple of four elements (one element per lane:
# two chunks, one ragged chunk, five chunks); the last three take the 16-byte route (one ragged chunk; two chunks, the second ragged;
# the same with B = 2, C = 3, so that plane, channel and mask index all differ -- named to sort last: seeds are places in sorted order)
CASES = {"head": (2, 16, 33, 49), "tiny": (1, 3, 1, 5), "one_plane": (1, 1, 1, 4099), "vector_ragged": (2, 3, 4, 8),
         "vector_two_blocks": (1, 2, 33, 128), "work_split_images": (2, 3, 33, 128)}
NATIVE = ("halo_affine_relu_fwd", "halo_dwconv3x3_affine_relu_fwd", "halo_upcat_dwconv3x3_affine_relu_fwd", "halo_pool_fold_affine_relu_fwd",
          "halo_dropout_pair_fwd", "halo_dropout_pair_bwd", "halo_masked_affine_relu_fwd", "halo_bilinear_upsample", "halo_hfr_fwd_apply")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture()
def serve_all(monkeypatch):
    """the speed rules off, the convolutions' backward deterministic"""
    from halo_amd import aspp, norm
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0, "masked": 0})
    monkeypatch.setattr(norm, "PAIR_AUTOGRAD_MIN_ELEMENTS", 0)
    monkeypatch.setattr(aspp, "EXCLUDED_SHAPES", set())
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


@pytest.fixture()
def native_calls(monkeypatch):
    """counts of the calls of the native entry points in NATIVE"""
    from halo_amd import _lib
    L, calls = _lib.lib(), {}
    for name in NATIVE:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _real=real, _name=name: (calls.__setitem__(_name, calls.get(_name, 0) + 1), _real(*a))[1])
    return calls


# ---------------------------------------------------------------- 1. the operator

def _both(fn, x0, bn, drop, seed, gy, gz):
    """(y, z, generator state, g_x for both gradients / g_z alone / g_y alone) of one seeded call"""
    x = x0.clone().requires_grad_(True)
    torch.manual_seed(seed)
    y, z = fn(x, bn, drop)
    state = torch.cuda.get_rng_state(x0.device)
    both, = torch.autograd.grad([y, z], x, [gy, gz], retain_graph=True)
    only_z, = torch.autograd.grad(z, x, gz, retain_graph=True)
    only_y, = torch.autograd.grad(y, x, gy)
    assert torch.equal(x.detach(), x0)
    return (y.detach(), z.detach(), state, both, only_z, only_y), ("y", "z", "generator", "g_x (g_y, g_z)", "g_x (g_z)", "g_x (g_y)")


def _same(a, b):
    """torch.equal with NaNs in the same places"""
    if a.dtype == torch.uint8:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_is_the_stock_statements(name, p, dev, serve_all, native_calls):
    from halo_amd import norm
    B, C, H, W = CASES[name]
    gen = torch.Generator(device=dev).manual_seed(sorted(CASES).index(name))
    x0, gy, gz = (torch.randn((B, C, H, W), device=dev, generator=gen) for _ in range(3))
    bn, drop = frozen(C, 3).to(dev) if C > 1 else _frozen_one(dev), nn.Dropout2d(p)
    seed = _seed_with_both_kinds_of_plane(x0, p)
    assert norm.pair_fallback_reason(x0.clone().requires_grad_(True), bn, drop) is None
    before = dict(norm.launches)
    got, names = _both(norm.norm_relu_dropout2d_pair, x0, bn, drop, seed, gy, gz)
    assert norm.launches["pair_fwd"] == before["pair_fwd"] + 1 and norm.launches["pair_bwd"] == before["pair_bwd"] + 3
    assert native_calls == {"halo_dropout_pair_fwd": 1, "halo_dropout_pair_bwd": 3}
    assert {k: v for k, v in norm.launches.items() if not k.startswith("pair")} == {k: v for k, v in before.items() if not k.startswith("pair")}
    want, _ = _both(norm.pair_statement, x0, bn, drop, seed, gy, gz)
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape and torch.equal(a, b), n
    y, z = got[:2]
    assert bool((y > 0).any()) and bool((y == 0).any()) and bool((got[5] != 0).any())
    if B * C > 1:
        dropped = ((z == 0) & (y > 0)).flatten(2).any(2)
        assert bool(dropped.any()) and not bool(dropped.all()), "pick another seed: no plane dropped, or every plane"
        # an inf in a dropped plane: y keeps it, z = inf * 0 is the stock chain's NaN -- the forward reads x there too
        b, c = (int(i) for i in dropped.nonzero()[0])
        x1 = x0.clone()
        x1[b, c].view(-1)[0] = float("inf") if float(norm.cached_scale_shift(bn)[0][c]) > 0 else float("-inf")
        got1, _ = _both(norm.norm_relu_dropout2d_pair, x1, bn, drop, seed, gy, gz)
        want1, _ = _both(norm.pair_statement, x1, bn, drop, seed, gy, gz)
        assert bool(torch.isinf(got1[0][b, c].view(-1)[0])) and bool(torch.isnan(got1[1][b, c].view(-1)[0])) and int(torch.isnan(got1[1]).sum()) == 1
        for n, a, b_ in zip(names, got1, want1):
            assert _same(a, b_), n


def _seed_with_both_kinds_of_plane(x, p):
    """the first seed under which nn.Dropout2d(p) drops a plane of x and keeps one (0 for a single plane)"""
    B, C = x.shape[:2]
    for seed in range(256):
        torch.manual_seed(seed)
        kept = int(x.new_empty((B, C, 1, 1)).bernoulli_(1 - p).sum())
        if B * C == 1 or 0 < kept < B * C:
            return seed
    raise AssertionError("no seed below 256 drops one of %d planes and keeps another" % (B * C))


def _frozen_one(dev):
    bn = frozen(2, 3)
    one = type(bn)(1)
    for n in ("weight", "bias", "running_mean", "running_var"):
        getattr(one, n).copy_(getattr(bn, n)[:1])
    return one.to(dev)


def test_operator_in_eval_mode_and_outside_its_envelope(dev, serve_all, native_calls):
    from halo_amd import norm
    gen = torch.Generator(device=dev).manual_seed(7)
    x0, gy, gz = (torch.randn((2, 16, 5, 7), device=dev, generator=gen) for _ in range(3))
    bn = frozen(16, 4).to(dev)
    # eval mode and p = 0: nothing is drawn, norm_relu's pass, and the dropout returns its input
    for drop in (nn.Dropout2d(0.5).eval(), nn.Dropout2d(0.0)):
        native_calls.clear()
        torch.manual_seed(1)
        state = torch.cuda.get_rng_state(dev)
        x = x0.clone().requires_grad_(True)
        y, z = norm.norm_relu_dropout2d_pair(x, bn, drop)
        assert z is y and torch.equal(torch.cuda.get_rng_state(dev), state)
        assert native_calls == {"halo_affine_relu_fwd": 1}
        xs = x0.clone().requires_grad_(True)
        ys, zs = norm.pair_statement(xs, bn, drop)
        assert zs is ys and torch.equal(y, ys) and torch.equal(torch.autograd.grad(y, x, gy)[0], torch.autograd.grad(ys, xs, gy)[0])
    # outside the envelope: the two torch statements, no launch of this module
    live = nn.BatchNorm2d(16).to(dev).eval()
    with torch.no_grad():
        live.running_mean.copy_(bn.running_mean), live.running_var.copy_(bn.running_var)
    cases = (("float32", x0.double(), bn, nn.Dropout2d(0.5)), ("FrozenBatchNorm2d", x0, live, nn.Dropout2d(0.5)), ("p = 1", x0, bn, nn.Dropout2d(1.0)))
    for word, x_in, norm_mod, drop in cases:
        assert word in norm.pair_fallback_reason(x_in, norm_mod, drop), word
        native_calls.clear()
        before = dict(norm.launches)
        got, names = _both(norm.norm_relu_dropout2d_pair, x_in, norm_mod, drop, 2, gy.to(x_in.dtype), gz.to(x_in.dtype))
        want, _ = _both(norm.pair_statement, x_in, norm_mod, drop, 2, gy.to(x_in.dtype), gz.to(x_in.dtype))
        assert all(_same(a, b) for a, b in zip(got, want)), word
        assert norm.launches == before and native_calls == {}, word


def test_backward_reads_only_the_gradients_that_arrived(dev, serve_all):
    """set_materialize_grads(False): an unused output reaches the backward as None, which the entry point gets as a null pointer; a
    backward that is asked for nothing launches nothing; y, scale and the noise are what the node keeps"""
    from halo_amd import _lib, norm
    gen = torch.Generator(device=dev).manual_seed(8)
    x0, g = (torch.randn((2, 16, 5, 7), device=dev, generator=gen) for _ in range(2))
    bn, drop = frozen(16, 5).to(dev), nn.Dropout2d(0.5)
    seen = []
    L = _lib.lib()
    real = L.halo_dropout_pair_bwd
    L.halo_dropout_pair_bwd = lambda *a: (seen.append((a[0].value, a[1].value)), real(*a))[1]
    try:
        for use in ("z", "y"):
            x = x0.clone().requires_grad_(True)
            torch.manual_seed(3)
            y, z = norm.norm_relu_dropout2d_pair(x, bn, drop)
            assert y.grad_fn is z.grad_fn and sorted(tuple(t.shape) for t in y.grad_fn.saved_tensors) == sorted([(2, 16, 5, 7), (16,), (2, 16, 1, 1)])
            (z if use == "z" else y).backward(g)
            gy_ptr, gz_ptr = seen.pop()
            assert (gy_ptr is None) == (use == "z") and (gz_ptr is None) == (use == "y") and not seen
        before = dict(norm.launches)
        with torch.no_grad():
            torch.manual_seed(3)
            y1, z1 = norm.norm_relu_dropout2d_pair(x0, bn, drop)
        assert torch.equal(y1, y.detach()) and torch.equal(z1, z.detach()) and not y1.requires_grad
        assert norm.launches["pair_fwd"] == before["pair_fwd"] + 1 and norm.launches["pair_bwd"] == before["pair_bwd"] and not seen
    finally:
        L.halo_dropout_pair_bwd = real


# ---------------------------------------------------------------- the stand-in head

def _feats(dev):
    gen = torch.Generator().manual_seed(12)
    return {"out": torch.randn(2, 24, 9, 13, generator=gen).to(dev), "low": torch.randn(2, 12, 33, 49, generator=gen).to(dev)}


def _heads(dev, old, hfr, *classes_and_blocks):
    """heads of the given (class, block class) pairs with one set of weights, on the device in train() mode"""
    torch.manual_seed(11)
    with torch.no_grad():
        heads = [cls(block, old=old, hfr=hfr, p=0.5) for cls, block in classes_and_blocks]
    for h in heads[1:]:
        h.load_state_dict(heads[0].state_dict())
    return [h.to(dev).train() for h in heads]


def _step(fn, head, feats, size, seed):
    """(out, decoder_out, generator state, the gradient of every parameter and of both inputs) of one seeded call of fn(feats, size)"""
    top, low = feats["out"].clone().requires_grad_(True), feats["low"].clone().requires_grad_(True)
    named = [(n, p) for n, p in head.named_parameters() if p.requires_grad]
    torch.manual_seed(seed)
    out, dec = fn({"out": top, "low": low}, size)
    state = torch.cuda.get_rng_state(top.device)
    grads = torch.autograd.grad(out.square().sum(), [top, low] + [p for _, p in named])
    return (out.detach(), dec.detach(), state) + grads, ["out", "decoder_out", "generator", "g_top", "g_low"] + [n for n, _ in named]


@pytest.mark.parametrize("old,hfr", [(True, False), (False, True)], ids=["old_layout", "new_layout"])
def test_bound_head_under_the_bit_preserving_marks_returns_the_stand_ins_bits(old, hfr, dev, serve_all, native_calls):
    """fuse_norm_relu_pairs, use_fused_pointwise_norm and use_fused_decoder_dropout return the stock statements' bits, so the bound
    and marked head returns the unbound stand-in's: both outputs, the generator state, every parameter and input gradient"""
    from halo_amd import hooks
    Bound = hooks.use_fused_decoder_dropout(hooks.use_v3plus_forward(type("Bound", (EuclidHead,), {})))
    Tail = hooks.use_fused_pointwise_norm(type("Tail", (Block,), {}))
    plain, bound = _heads(dev, old, hfr, (EuclidHead, Block), (Bound, Tail))
    keys, modules = list(plain.state_dict()), [n for n, _ in plain.named_modules()]
    assert hooks.fuse_norm_relu_pairs(bound) == 4
    feats = _feats(dev)
    for size in (None, (40, 50)):
        want, names = _step(plain, plain, feats, size, 13)
        assert native_calls == {}                                         # the stand-in runs none of the package's passes
        again, _ = _step(plain, plain, feats, size, 13)
        assert all(torch.equal(a, b) for a, b in zip(want, again)), "the stock head does not repeat its own bits on this device"
        got, _ = _step(bound, bound, feats, size, 13)
        for name, a, b in zip(names, want, got):
            assert a.shape == b.shape and torch.equal(a, b), (size, name)
        assert bool(torch.isfinite(want[0]).all()) and float(want[0].std()) > 0 and all(float(t.abs().sum()) > 0 for t in want[3:])
        if old:
            # decoder[1] and decoder[2] ran as the two-output pass; the two ASPP blocks, decoder[0] and the four pairs as norm_relu
            assert native_calls == {"halo_dropout_pair_fwd": 1, "halo_dropout_pair_bwd": 1, "halo_affine_relu_fwd": 7}
            with torch.no_grad():
                assert not torch.equal(plain.decoder[3](want[1]), want[0])    # a plane was dropped: out is not the conv of decoder_out
        else:
            assert native_calls == {"halo_affine_relu_fwd": 8}
        native_calls.clear()
    # eval mode: nothing is drawn, and the pair is norm_relu's pass
    bound.load_state_dict(plain.state_dict())                              # wn_mlp's running statistics: plain has taken more steps
    plain.eval(), bound.eval()
    with torch.no_grad():
        torch.manual_seed(14)
        state = torch.cuda.get_rng_state(dev)
        a, b = plain(feats), bound(feats)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(torch.cuda.get_rng_state(dev), state)
        assert native_calls == {"halo_affine_relu_fwd": 8}
    assert list(bound.state_dict()) == keys and [n for n, _ in bound.named_modules()] == modules


def _by_hand(head):
    """the statements of a head under every mark and block hook, from the package's public operators"""
    from halo_amd import aspp, dwconv, hfr, norm, resize

    def block(blk, x):
        h = dwconv.depthwise_bn_relu(x, blk.depthwise_conv, blk.depthwise_bn, blk.depthwise_activate)
        return blk.pointwise_conv(h)

    def fn(feats, size):
        top, low = feats["out"], feats["low"]
        first = head.parallel_branches[0]
        pyramid = [norm.norm_relu(first[0](top), first[1])]
        pyramid += [norm.norm_relu(block(blk, top), blk.pointwise_bn) for blk in list(head.parallel_branches)[1:]]
        gb = head.global_branch
        pooled = norm.norm_relu(gb[1](gb[0](top)), gb[2])
        y = aspp.pooled_bottleneck(torch.cat(pyramid, dim=1), pooled, head.bottleneck[0], head.bottleneck[1])
        short = norm.norm_relu(head.shortcut[0](low), head.shortcut[1])
        d0, d1 = head.decoder[0], head.decoder[1]
        dec = dwconv.upsample_cat_depthwise_bn_relu(y, short, d0.depthwise_conv, d0.depthwise_bn)
        dec = norm.norm_relu(d0.pointwise_conv(dec), d0.pointwise_bn)
        if head.old_decoder:
            dec, z = norm.norm_relu_dropout2d_pair(block(d1, dec), d1.pointwise_bn, head.decoder[2])
            out = head.decoder[3](z)
        else:
            dec = head.conv_reduce(norm.norm_relu(block(d1, dec), d1.pointwise_bn))
            if head.wn_mlp is not None:
                dec = hfr.weighted_normalize(dec, head.wn_mlp)
            out = head.cls_conv(dec)
        if size is not None:
            out = resize.resize_or_interpolate(out, size)
        return out, dec
    return fn


@pytest.mark.parametrize("old,hfr", [(True, False), (False, True)], ids=["old_layout", "new_layout"])
def test_bound_head_under_every_mark_is_the_operators_composed_by_hand(old, hfr, dev, serve_all, native_calls):
    from halo_amd import aspp, dwconv, hfr as hfr_mod, hooks, norm
    Bound = hooks.use_v3plus_forward(type("Bound", (EuclidHead,), {}))
    for mark in (hooks.use_device_resize, hooks.use_fused_decoder_front, hooks.use_folded_image_pooling, hooks.use_fused_decoder_dropout,
                 hooks.use_fused_feature_reweighting):
        assert mark(Bound) is Bound
    Fused = hooks.use_fused_pointwise_norm(hooks.use_fused_depthwise(type("Fused", (Block,), {})))
    head, = _heads(dev, old, hfr, (Bound, Fused))
    assert hooks.fuse_norm_relu_pairs(head) == 4
    feats = _feats(dev)
    # every operator serves these shapes: the comparison cannot pass through fallbacks on both sides
    with torch.enable_grad():
        top = feats["out"].clone().requires_grad_(True)
        at_low = lambda c: torch.zeros(2, c, 33, 49, device=dev, requires_grad=True)
        d0, d1 = head.decoder[0], head.decoder[1]
        assert dwconv.fallback_reason(top, head.parallel_branches[1].depthwise_conv, head.parallel_branches[1].depthwise_bn) is None
        assert dwconv.fallback_reason(at_low(16), d1.depthwise_conv, d1.depthwise_bn) is None
        assert norm.fallback_reason(torch.zeros(2, 16, 9, 13, device=dev, requires_grad=True), head.bottleneck[1]) is None
        assert norm.fallback_reason(torch.zeros(2, 16, 1, 1, device=dev, requires_grad=True), head.global_branch[2]) is None
        assert norm.fallback_reason(at_low(8), head.shortcut[1]) is None and norm.fallback_reason(at_low(16), d0.pointwise_bn) is None
        assert aspp.pool_fold_fallback_reason(torch.zeros(2, 48, 9, 13, device=dev), torch.zeros(2, 16, 1, 1, device=dev), head.bottleneck[0],
                                              head.bottleneck[1], head.bottleneck[2]) is None
        assert dwconv.upcat_fallback_reason(torch.zeros(2, 16, 9, 13, device=dev), at_low(8), d0.depthwise_conv, d0.depthwise_bn) is None
        if old:
            assert norm.pair_fallback_reason(at_low(16), d1.pointwise_bn, head.decoder[2]) is None
        elif hfr:
            assert hfr_mod.fallback_reason(at_low(8), head.wn_mlp) is None
    for size in (None, (40, 50)):
        native_calls.clear()
        got, names = _step(head, head, feats, size, 15)
        ran = dict(native_calls)
        # the two ASPP blocks and decoder[1] through the depthwise pass, decoder[0]'s first half through the fused front, the folded
        # bottleneck; norm_relu for the four pairs less the bottleneck's, which the folded operator takes over, and the blocks' tails
        want_ran = {"halo_dwconv3x3_affine_relu_fwd": 3, "halo_upcat_dwconv3x3_affine_relu_fwd": 1, "halo_pool_fold_affine_relu_fwd": 1,
                    "halo_affine_relu_fwd": 6 if old else 7}
        if old:
            want_ran.update(halo_dropout_pair_fwd=1, halo_dropout_pair_bwd=1)
        assert {k: v for k, v in ran.items() if k in want_ran} == want_ran
        assert (ran.get("halo_hfr_fwd_apply", 0) >= 1) == (not old and hfr) and (ran.get("halo_bilinear_upsample", 0) >= 1) == (size is not None)
        assert "halo_masked_affine_relu_fwd" not in ran
        native_calls.clear()
        want, _ = _step(_by_hand(head), head, feats, size, 15)
        assert dict(native_calls) == ran
        for name, a, b in zip(names, want, got):
            assert a.shape == b.shape and torch.equal(a, b), (size, name)
        assert bool(torch.isfinite(got[0]).all()) and float(got[0].std()) > 0 and all(float(t.abs().sum()) > 0 for t in got[3:])


def test_two_steps_under_the_device_resize_give_the_same_gradients(dev, serve_all):
    """use_device_resize on the bound head: no resize of the step scatters atomic adds, so the gradients that arrive at the
    bottleneck's and the shortcut's outputs -- behind the resize of the logits and the one to the low-level map -- repeat bit for bit"""
    from halo_amd import hooks
    Bound = hooks.use_v3plus_forward(type("Bound", (EuclidHead,), {}))
    hooks.use_device_resize(Bound), hooks.use_fused_decoder_dropout(Bound)
    Tail = hooks.use_fused_pointwise_norm(type("Tail", (Block,), {}))
    head, = _heads(dev, True, False, (Bound, Tail))
    assert hooks.fuse_norm_relu_pairs(head) == 4
    feats = _feats(dev)
    runs = []
    for _ in range(2):
        seen = {}
        def watch(name):
            def forward_hook(mod, i, o):
                o.register_hook(lambda g: seen.__setitem__(name, g.clone()))
            return forward_hook
        handles = [m.register_forward_hook(watch(name)) for name, m in (("bottleneck", head.bottleneck), ("shortcut", head.shortcut))]
        head.zero_grad(set_to_none=True)
        torch.manual_seed(16)
        out, _ = head(feats, size=(65, 97))
        out.square().sum().backward()
        for h in handles:
            h.remove()
        assert sorted(seen) == ["bottleneck", "shortcut"] and all(float(g.abs().sum()) > 0 for g in seen.values())
        runs.append([seen["bottleneck"], seen["shortcut"]] + [p.grad.clone() for p in head.parameters()])
    assert tuple(runs[0][0].shape) == (2, 16, 9, 13) and tuple(runs[0][1].shape) == (2, 8, 33, 49)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
