"""The multi-dilation depthwise passes on the device (halo_multi_dwconv3x3_* of halo_dwconv.hip, halo_amd.dwconv.multi_depthwise_bn_relu,
halo_amd.hooks.use_fused_aspp_depthwise).

The contract is an equality against the operator that tests/test_gpu_dwconv*.py hold to float64: y_i is depthwise_bn_relu's, g_x is
((gx_0 + gx_1) + gx_2) ... of its input gradients in torch float32 adds, g_w_i is its weight gradient -- torch.equal, no tolerance.
The composition is computed once per case and shared.  Two cases are also held to float64 directly (sum_i dwconv_ref.grad_x with
the device's masks; bound: every term's own 15u bound plus (N - 1) u times the magnitudes that pass through the adds).  The head test
compares a marked stand-in head (tests/euclid_head_standin.py) with the same head under use_fused_depthwise alone: bit-equal outputs
and parameter gradients, and the gradient of the backbone's output within the distance of two float32 summation orders of its terms
t_i: 2 gamma_{n-1} sum |t_i|, gamma_k = k u / (1 - k u), u = 2^-24 (n = 4 in the stand-in: two dilated blocks, the 1 x 1 branch, the
pooled branch)."""
import numpy as np
import pytest
import torch

import dwconv_ref as R
import dwmulti_cases as K
from euclid_head_standin import Block, EuclidHead

pytestmark = pytest.mark.gpu
MULTI = ("halo_multi_dwconv3x3_affine_relu_fwd", "halo_multi_dwconv3x3_affine_relu_bwd_data")
SINGLE = ("halo_dwconv3x3_affine_relu_fwd", "halo_dwconv3x3_affine_relu_bwd_data", "halo_dwconv3x3_affine_relu_bwd_weight")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def no_speed_rule(monkeypatch):
    """the size rule is about speed alone: off, so that the small shapes run the passes"""
    from halo_amd import dwconv
    monkeypatch.setattr(dwconv, "MULTI_MIN_ELEMENTS", 0)


@pytest.fixture()
def native_calls(monkeypatch):
    """the arguments of every call of the entry points in MULTI and SINGLE"""
    from halo_amd import _lib
    L, calls = _lib.lib(), {}
    for name in MULTI + SINGLE:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _real=real, _name=name: (calls.setdefault(_name, []).append(a), _real(*a))[1])
    return calls


def offset_view(t):
    """the same values in storage that starts 4 bytes off a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 1, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def operands(cs, dev, view=lambda t: t):
    """(x, the (conv, bn) pairs, the gradients) of a case on the device"""
    x = view(torch.from_numpy(cs[0]["x"]).to(dev))
    return x, [R.modules(c, dev) for c in cs], [view(torch.from_numpy(c["g"]).to(dev)) for c in cs]


_composed = {}


def composed(key, cs, dev, view=lambda t: t):
    """the contract's right-hand side: (ys, gxs, gws) of one depthwise_bn_relu per dilation.  Computed once per case, never written."""
    if key not in _composed:
        from halo_amd.dwconv import depthwise_bn_relu, fallback_reason
        x0, blocks, gs = operands(cs, dev, view)
        ys, gxs, gws = [], [], []
        for (conv, bn), g in zip(blocks, gs):
            x = x0.detach().requires_grad_(True)
            assert fallback_reason(x, conv, bn) is None
            y = depthwise_bn_relu(x, conv, bn)
            gx, gw = torch.autograd.grad(y, [x, conv.weight], g)
            ys.append(y.detach()), gxs.append(gx), gws.append(gw)
        _composed[key] = (ys, gxs, gws)
    return _composed[key]


def added(gxs, used):
    """((gx_0 + gx_1) + gx_2) ... over the used outputs, torch float32 adds in list order"""
    total = None
    for i in used:
        total = gxs[i].clone() if total is None else total + gxs[i]
    return total


def run_multi(cs, dev, used=None, view=lambda t: t, x_grad=True):
    """(ys, g_x, g_ws) of one multi_depthwise_bn_relu call and a backward through the outputs in `used` (default: all)"""
    from halo_amd import dwconv
    x0, blocks, gs = operands(cs, dev, view)
    used = list(range(len(cs))) if used is None else used
    x = x0.detach().requires_grad_(x_grad)
    assert dwconv.multi_fallback_reason(x, blocks) is None
    ys = dwconv.multi_depthwise_bn_relu(x, blocks)
    assert isinstance(ys, tuple) and len(ys) == len(cs) and len({id(y.grad_fn) for y in ys}) == 1
    assert type(ys[0].grad_fn).__name__.startswith("_MultiDepthwiseBnReluFn")
    wanted = ([x] if x_grad else []) + [blocks[i][0].weight for i in range(len(cs))]
    grads = torch.autograd.grad([ys[i] for i in used], wanted, [gs[i] for i in used], allow_unused=True)
    gx = grads[0] if x_grad else None
    return [y.detach() for y in ys], gx, list(grads[1 if x_grad else 0:])


def assert_contract(got, want, used):
    ys, gx, gws = got
    wys, wgxs, wgws = want
    for i, (a, b) in enumerate(zip(ys, wys)):
        assert a.shape == b.shape and a.is_contiguous() and torch.equal(a, b), "y_%d" % i
    if gx is not None:
        assert torch.equal(gx, added(wgxs, used)), "g_x"
    for i, (a, b) in enumerate(zip(gws, wgws)):
        if i in used:
            assert a.shape == b.shape and torch.equal(a, b), "g_w_%d" % i
        else:
            assert a is None, "g_w_%d of an unused output" % i


@pytest.mark.parametrize("name", list(K.CASES))
def test_contract_on_every_case(dev, name, native_calls):
    from halo_amd import dwconv
    cs = K.case(name)
    want = composed(name, cs, dev)
    native_calls.clear()
    before = dict(dwconv.launches)
    got = run_multi(cs, dev)
    assert dwconv.launches == {"multi_fwd": before["multi_fwd"] + 1, "multi_bwd": before["multi_bwd"] + 1}
    assert {k: len(v) for k, v in native_calls.items()} == {MULTI[0]: 1, MULTI[1]: 1, SINGLE[2]: len(cs)}      # no single fwd, no bwd_data
    assert_contract(got, want, list(range(len(cs))))
    ys, gx, gws = got
    dead = cs[0]["C"] - 1
    assert all(bool((y[:, dead] == 0).all()) for y in ys) and bool((gx[:, dead] == 0).all())
    if ys[0].numel() > 64:
        assert all(bool((y > 0).any()) for y in ys) and bool((gx != 0).any())


@pytest.mark.parametrize("name", K.OFFSET)
def test_offset_operands_run_the_one_element_route_with_the_same_bits(dev, name, native_calls):
    """x and every g as contiguous views 4 bytes off a 16-byte boundary at a W % 4 == 0 shape: y and g_x do not depend on the route
    (the aligned composition's bits); g_w is the existing entry over the same offset operands"""
    cs = K.case(name)
    assert cs[0]["W"] % 4 == 0
    aligned = composed(name, cs, dev)
    shifted = composed(name + "/offset", cs, dev, offset_view)
    native_calls.clear()
    ys, gx, gws = run_multi(cs, dev, view=offset_view)
    assert native_calls[MULTI[0]][0][0].value % 16 == 4                                    # x
    assert all(p % 16 == 4 for p in native_calls[MULTI[1]][0][0])                          # every g_i
    n = list(range(len(cs)))
    assert_contract((ys, gx, gws), (aligned[0], aligned[1], shifted[2]), n)


@pytest.mark.parametrize("used", [[1], [0, 2]], ids=["only_1", "0_and_2"])
def test_unused_outputs_are_neither_staged_nor_added(dev, used, native_calls):
    from halo_amd import dwconv
    name = "head_dilations"
    cs = K.case(name)
    want = composed(name, cs, dev)
    native_calls.clear()
    before = dict(dwconv.launches)
    got = run_multi(cs, dev, used=used)
    assert dwconv.launches["multi_bwd"] == before["multi_bwd"] + 1
    ptrs = list(native_calls[MULTI[1]][0][0])
    assert [p is not None and p != 0 for p in ptrs] == [i in used for i in range(3)]
    assert len(native_calls[SINGLE[2]]) == len(used) and SINGLE[1] not in native_calls
    assert_contract(got, want, used)
    assert not torch.equal(got[1], added(want[1], [0, 1, 2]))


def test_x_without_a_gradient_launches_no_data_pass(dev, native_calls):
    from halo_amd import dwconv
    name = "unsorted_repeated"
    cs = K.case(name)
    want = composed(name, cs, dev)
    native_calls.clear()
    before = dict(dwconv.launches)
    got = run_multi(cs, dev, x_grad=False)
    assert dwconv.launches == {"multi_fwd": before["multi_fwd"] + 1, "multi_bwd": before["multi_bwd"]}
    assert MULTI[1] not in native_calls and SINGLE[1] not in native_calls and len(native_calls[SINGLE[2]]) == 3
    assert_contract(got, want, [0, 1, 2])
    with torch.no_grad():
        x0, blocks, _ = operands(cs, dev)
        ys = dwconv.multi_depthwise_bn_relu(x0, blocks)
    assert dwconv.launches["multi_fwd"] == before["multi_fwd"] + 2 and not ys[0].requires_grad
    assert all(torch.equal(a, b) for a, b in zip(ys, want[0]))


@pytest.mark.parametrize("name", K.FLOAT64)
def test_g_x_against_float64(dev, name):
    """independent of the composition: sum_i grad_x_64(case_i, the device's mask of y_i), and each y_i against its own float64"""
    cs = K.case(name)
    ys, gx, _ = run_multi(cs, dev)
    gx = gx.cpu().numpy().astype(np.float64)
    refs, bounds = [], []
    for c, y in zip(cs, ys):
        y = y.cpu().numpy().astype(np.float64)
        pre, fb = R.forward(c)
        band = np.abs(pre) <= fb
        assert band.mean() <= 1e-4 and ((y > 0) == (pre > 0))[~band].all()
        assert (np.abs(y - np.maximum(pre, 0)) <= fb).all()
        r, b = R.grad_x(c, y > 0)
        refs.append(r), bounds.append(b)
    bound = K.f32_sum_bound(refs, bounds)
    err = np.abs(gx - sum(refs))
    print(name, "g_x: max err / bound", float((err[bound > 0] / bound[bound > 0]).max()))
    assert (err[bound == 0] == 0).all() and (err <= bound).all()


def test_envelope_edge_is_read_from_the_library(dev, native_calls):
    from halo_amd import dwconv
    limit = dwconv.multi_max_plane()
    inside, outside = K.edge_shapes(limit)
    assert inside[2] * inside[3] == limit and outside[2] * outside[3] > limit
    cs = K.build(900, *inside, (6, 12, 18))
    want = composed("edge/inside", cs, dev)
    native_calls.clear()
    assert_contract(run_multi(cs, dev), want, [0, 1, 2])
    assert len(native_calls[MULTI[0]]) == 1 and len(native_calls[MULTI[1]]) == 1
    # one row more: a reason that names the plane, and the composition's bits through the fallback
    cs = K.build(901, *outside, (6, 12, 18))
    want = composed("edge/outside", cs, dev)
    x0, blocks, gs = operands(cs, dev)
    x = x0.requires_grad_(True)
    why = dwconv.multi_fallback_reason(x, blocks)
    assert why is not None and "plane of %d x %d" % outside[2:] in why and str(limit) in why
    native_calls.clear()
    before = dict(dwconv.launches)
    ys = dwconv.multi_depthwise_bn_relu(x, blocks)
    grads = torch.autograd.grad(ys, [x] + [b[0].weight for b in blocks], gs)
    assert dwconv.launches == before and not any(k in native_calls for k in MULTI) and len(native_calls[SINGLE[1]]) == 3
    assert_contract(([y.detach() for y in ys], grads[0], list(grads[1:])), want, [0, 1, 2])


# ---------------------------------------------------------------- the stand-in head

def _heads(dev, *classes_and_blocks):
    torch.manual_seed(21)
    with torch.no_grad():
        heads = [cls(block, old=True, hfr=False, p=0.5) for cls, block in classes_and_blocks]
    for h in heads[1:]:
        h.load_state_dict(heads[0].state_dict())
    return [h.to(dev).train() for h in heads]


def _step(head, feats, seed, split=False):
    """(out, decoder_out, g_top, g_low, every parameter gradient); split: instead of g_top, its terms -- every reader of top gets a
    leaf copy, and one torch.autograd.grad per reader gives the term that reader sends back"""
    top, low = feats["out"].clone().requires_grad_(True), feats["low"].clone().requires_grad_(True)
    named = [(n, p) for n, p in head.named_parameters() if p.requires_grad]
    leaves, handles = [], []
    if split:
        def feed(mod, inputs):
            leaves.append(inputs[0].detach().clone().requires_grad_(True))
            return (leaves[-1],)
        handles = [m.register_forward_pre_hook(feed) for m in list(head.parallel_branches) + [head.global_branch]]
    torch.manual_seed(seed)
    out, dec = head({"out": top, "low": low}, None)
    for h in handles:
        h.remove()
    loss = out.square().sum()
    if split:
        return [torch.autograd.grad(loss, leaf, retain_graph=True)[0] for leaf in leaves]
    grads = torch.autograd.grad(loss, [top, low] + [p for _, p in named])
    return (out.detach(), dec.detach()) + grads, ["out", "decoder_out", "g_top", "g_low"] + [n for n, _ in named]


def test_marked_head_returns_the_bits_of_the_head_under_use_fused_depthwise(dev, native_calls, monkeypatch):
    from halo_amd import dwconv, hooks
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    Fused = hooks.use_fused_depthwise(type("Fused", (Block,), {}))
    Base = hooks.use_v3plus_forward(type("Base", (EuclidHead,), {}))
    Marked = hooks.use_fused_aspp_depthwise(hooks.use_v3plus_forward(type("Marked", (EuclidHead,), {})))
    assert not hasattr(Base, "_halo_fused_aspp_depthwise")
    base, marked = _heads(dev, (Base, Fused), (Marked, Fused))
    keys, modules = list(base.state_dict()), [n for n, _ in base.named_modules()]
    gen = torch.Generator().manual_seed(22)
    feats = {"out": torch.randn(2, 24, 9, 13, generator=gen).to(dev), "low": torch.randn(2, 12, 33, 49, generator=gen).to(dev)}
    want, names = _step(base, feats, 23)
    assert not any(k in native_calls for k in MULTI) and len(native_calls[SINGLE[0]]) == 4            # two ASPP blocks, two decoder blocks
    again, _ = _step(base, feats, 23)
    assert all(torch.equal(a, b) for a, b in zip(want, again)), "the unmarked head does not repeat its own bits on this device"
    native_calls.clear()
    before = dict(dwconv.launches)
    got, _ = _step(marked, feats, 23)
    assert dwconv.launches == {"multi_fwd": before["multi_fwd"] + 1, "multi_bwd": before["multi_bwd"] + 1}
    assert len(native_calls[SINGLE[0]]) == 2 and len(native_calls[SINGLE[1]]) == 2                   # the decoder's two blocks alone
    terms = _step(base, feats, 23, split=True)
    assert len(terms) == 4 and all(float(t.abs().sum()) > 0 for t in terms)
    k = len(terms) - 1
    gamma = k * U / (1 - k * U)
    bound = 2 * gamma * sum(t.double().abs() for t in terms)
    for name, a, b in zip(names, want, got):
        assert a.shape == b.shape, name
        if name == "g_top":
            err = (a.double() - b.double()).abs()
            print("g_top: max err / bound", float((err / bound.clamp_min(1e-300)).max()), "equal", torch.equal(a, b))
            assert bool((err <= bound).all()), name
        else:
            assert torch.equal(a, b), name
    assert all(float(t.abs().sum()) > 0 for t in want[2:])
    with torch.no_grad():
        before = dict(dwconv.launches)
        torch.manual_seed(24)
        a = base(feats)
        torch.manual_seed(24)
        b = marked(feats)
        assert dwconv.launches == {"multi_fwd": before["multi_fwd"] + 1, "multi_bwd": before["multi_bwd"]}
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert list(marked.state_dict()) == keys and [n for n, _ in marked.named_modules()] == modules
