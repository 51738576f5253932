"""halo_amd.norm.norm_relu_fork (halo_fork_affine_relu_bwd of halo_norm.hip) and halo_amd.hooks.fuse_residual_chains on the device,
against the stock torch statements on the same device.  The engine's accumulation of two gradients is one float32 add per element
and the kernel takes that add into its pass, so every comparison is norm_ref.same_bits: NaN positions equal, everything else
torch.equal."""
import copy
import gc

import pytest
import torch
import torch.nn as nn

import norm_ref as N
from dwconv_ref import FrozenBatchNorm2d

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")
# (B, C, H, W); AN_CHUNK = 1024 groups of 4 (16-byte route) or of 1 (scalar route) per workgroup
SHAPES = {
    "vector_chunk_and_group": (2, 3, 41, 100),   # HW = 4100: 1025 groups of four, one whole chunk and one ragged group
    "scalar_chunk_and_three": (2, 3, 13, 79),    # HW = 1027: one whole chunk of single elements and three more
    "two_groups": (2, 3, 2, 4),                  # HW = 8
    "one_element": (2, 3, 1, 1),                 # HW = 1
    "offset_second_gradient": (2, 3, 41, 100),   # HW = 4100, g_b one element off 16 bytes: the scalar route
}
VARIANTS = ("none", "plain", "affine")
WANTS = {"none": ("x",), "plain": ("x", "r", "both"), "affine": ("x", "r", "both")}


@pytest.fixture(autouse=True)
def every_size_served(monkeypatch):
    """the size rules are about speed alone (both sides return the same bits); these tests are about the kernels and the plumbing"""
    from halo_amd import norm
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0, "masked": 0})
    monkeypatch.setattr(norm, "FORK_AUTOGRAD_MIN_ELEMENTS", 0)


def _norm(C, seed):
    """channel 0: scale = -2, shift = +1; channel 1: scale = +2, shift = -1 (x = 0.5 gives pre == 0 in both); the rest random"""
    bn = N.randomize_norms(FrozenBatchNorm2d(C), seed)
    with torch.no_grad():
        bn.weight[0], bn.running_var[0], bn.bias[0], bn.running_mean[0] = -2.0, 1.0, 1.0, 0.0
        bn.weight[1], bn.running_var[1], bn.bias[1], bn.running_mean[1] = 2.0, 1.0, -1.0, 0.0
    return bn.to(DEV)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _planted(shape, gen, values):
    """a random tensor with `values` at random places (as many as fit)"""
    n = _numel(shape)
    flat = torch.randn(n, generator=gen)
    k = min(n, len(values))
    where = torch.randperm(n, generator=gen)[:k]
    flat[where] = torch.tensor(values)[:k]
    return flat.view(shape), where


def _offset(t):
    """the same values in a contiguous view that starts one element past a 16-byte boundary"""
    base = torch.empty(t.numel() + 1, device=DEV)
    base[1:].copy_(t.reshape(-1))
    out = base[1:].view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


@pytest.fixture(scope="module")
def cases():
    """per (shape name, variant): operands, the two weights, and the stock statements' y and gradients with t used in both
    places; computed once and left unchanged"""
    from halo_amd import norm
    out = {}
    for si, (name, shape) in enumerate(SHAPES.items()):
        for vi, variant in enumerate(VARIANTS):
            gen = torch.Generator().manual_seed(1000 + 100 * si + vi)
            bn = _norm(shape[1], 7 + si)
            rbn = _norm(shape[1], 70 + si) if variant == "affine" else None
            x, _ = _planted(shape, gen, [float("nan"), 0.5, 0.5, -0.0, 0.0, INF, -INF, 0.5, float("nan")])       # NaN y, pre == 0
            x.view(shape[0], shape[1], -1)[0, :2, :3] = 0.5                       # pre == 0 exactly in channels 0 and 1
            r, _ = _planted(shape, gen, [0.0, -0.0, float("nan"), INF])
            pairs = [(INF, -INF), (-INF, INF), (-0.0, -0.0), (-0.0, 0.0), (0.0, -0.0), (float("nan"), 1.0), (INF, INF), (1.0, float("nan"))]
            wa, where = _planted(shape, gen, [p[0] for p in pairs] * 3)
            wb = torch.randn(_numel(shape), generator=gen)
            wb[where] = torch.tensor([p[1] for p in pairs] * 3)[:len(where)]
            wb = wb.view(shape)
            x, r, wa, wb = x.to(DEV), (r.to(DEV) if variant != "none" else None), wa.to(DEV), wb.to(DEV)
            if name == "offset_second_gradient":
                wb = _offset(wb)
            xs = x.clone().requires_grad_(True)
            rs = r.clone().requires_grad_(True) if r is not None else None
            t = norm.torch_statement(xs, bn, rs, rbn)
            inputs = [xs] if r is None else [xs, rs]
            if name == "offset_second_gradient":
                grads = torch.autograd.grad([t, t.view_as(t)], inputs, [wa, wb])
            else:
                grads = torch.autograd.grad((t * wa).sum() + (t * wb).sum(), inputs)
            if _numel(shape) > 1000:
                y = t.detach()
                assert bool(y.isnan().any()) and bool((y == 0).any()) and bool((wa + wb).isnan().any())
                assert int((bn(x) == 0).sum()) >= 2
                s = bn.weight * bn.running_var.rsqrt()
                assert bool((s < 0).any()) and bool((s > 0).any())
            out[(name, variant)] = dict(bn=bn, rbn=rbn, x=x, r=r, wa=wa, wb=wb, y=t.detach(), gx=grads[0],
                                        gr=grads[1] if r is not None else None)
    return out


def _fork_grads(c, name, want):
    """norm_relu_fork on a case with y used twice on the device; returns (y, y_id, {input name: gradient})"""
    from halo_amd import norm
    x, r = c["x"].clone(), c["r"].clone() if c["r"] is not None else None
    if want in ("x", "both"):
        x.requires_grad_(True)
    if want in ("r", "both"):
        r.requires_grad_(True)
    y, y_id = norm.norm_relu_fork(x, c["bn"], r, c["rbn"])
    names = ("x", "r") if want == "both" else (want,)
    inputs = [{"x": x, "r": r}[k] for k in names]
    if name == "offset_second_gradient":
        grads = torch.autograd.grad([y, y_id], inputs, [c["wa"], c["wb"]])
    else:
        grads = torch.autograd.grad((y * c["wa"]).sum() + (y_id * c["wb"]).sum(), inputs)
    return y, y_id, dict(zip(names, grads))


@pytest.mark.parametrize("name,variant,want", [(n, v, w) for n in SHAPES for v in VARIANTS for w in WANTS[v]])
def test_fork_equals_the_stock_statements(cases, name, variant, want):
    from halo_amd import norm
    c = cases[(name, variant)]
    assert norm.fallback_reason(c["x"], c["bn"], c["r"], c["rbn"]) is None
    before = dict(norm.launches)
    y, y_id, grads = _fork_grads(c, name, want)
    print(name, variant, want, {k: norm.launches[k] - before[k] for k in ("fwd", "bwd", "fork_bwd")})
    assert norm.launches["fwd"] == before["fwd"] + 1 and norm.launches["fork_bwd"] == before["fork_bwd"] + 1
    assert norm.launches["bwd"] == before["bwd"]                                   # one pass each way, none of the old backward
    assert y_id is not y and y_id.data_ptr() == y.data_ptr() and y_id._base is y    # a view: no copy, no extra kernel
    assert N.same_bits(y.detach(), c["y"]) and N.same_bits(y_id.detach(), c["y"])
    if "x" in grads:
        assert N.same_bits(grads["x"], c["gx"]), "g_x"
    if "r" in grads:
        assert N.same_bits(grads["r"], c["gr"]), "g_r"


@pytest.mark.parametrize("variant", ["plain", "affine"])
def test_launches_follow_the_gradients_that_arrive(cases, variant):
    from halo_amd import norm
    c = cases[("vector_chunk_and_group", variant)]
    # one output used: the single-gradient backward, whichever output it is
    xs, rs = c["x"].clone().requires_grad_(True), c["r"].clone().requires_grad_(True)
    want = torch.autograd.grad(norm.torch_statement(xs, c["bn"], rs, c["rbn"]), [xs, rs], c["wa"])
    for used in (0, 1):
        x, r = c["x"].clone().requires_grad_(True), c["r"].clone().requires_grad_(True)
        before = dict(norm.launches)
        pair = norm.norm_relu_fork(x, c["bn"], r, c["rbn"])
        got = torch.autograd.grad(pair[used], [x, r], c["wa"])
        assert norm.launches["bwd"] == before["bwd"] + 1 and norm.launches["fork_bwd"] == before["fork_bwd"]
        assert N.same_bits(got[0], want[0]) and N.same_bits(got[1], want[1])
    # no input needs a gradient: the fused forward, the same tensor twice, and nothing in a backward that reaches it
    before = dict(norm.launches)
    y, y_id = norm.norm_relu_fork(c["x"], c["bn"], c["r"], c["rbn"])
    assert y is y_id and y.grad_fn is None and not y.requires_grad and N.same_bits(y, c["y"])
    w = torch.ones((), device=DEV, requires_grad=True)
    ((y * w).sum() + (y_id * w).sum()).backward()
    with torch.no_grad():
        z, z_id = norm.norm_relu_fork(c["x"].clone().requires_grad_(True), c["bn"], c["r"], c["rbn"])
    assert z is z_id and N.same_bits(z, c["y"])
    assert norm.launches["fwd"] == before["fwd"] + 2
    assert {k: v for k, v in norm.launches.items() if k != "fwd"} == {k: v for k, v in before.items() if k != "fwd"}
    # neither output used: the node's backward launches nothing
    x = c["x"].clone().requires_grad_(True)
    before = dict(norm.launches)
    y, y_id = norm.norm_relu_fork(x, c["bn"], c["r"], c["rbn"])
    assert norm._NormReluForkFn.backward(y.grad_fn, None, None) == (None,) * 6
    assert norm.launches["bwd"] == before["bwd"] and norm.launches["fork_bwd"] == before["fork_bwd"]


def test_the_fork_follows_its_own_size_rule(cases, monkeypatch):
    from halo_amd import norm
    c = cases[("vector_chunk_and_group", "plain")]
    n = c["x"].numel()
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 2 * n, "affine": 2 * n, "masked": 2 * n})     # norm_relu: the stock statements
    for least, served in ((n, True), (n + 1, False)):
        monkeypatch.setattr(norm, "FORK_AUTOGRAD_MIN_ELEMENTS", least)
        before = dict(norm.launches)
        y, y_id, grads = _fork_grads(c, "vector_chunk_and_group", "both")
        assert (y_id is y) != served and (norm.fork_fallback_reason(c["x"].clone().requires_grad_(True), c["bn"], c["r"]) is None) == served
        assert norm.launches["fork_bwd"] == before["fork_bwd"] + served and norm.launches["fwd"] == before["fwd"] + served
        assert norm.launches["bwd"] == before["bwd"]
        assert N.same_bits(y.detach(), c["y"]) and N.same_bits(grads["x"], c["gx"]) and N.same_bits(grads["r"], c["gr"])


@pytest.mark.parametrize("what", ["autocast", "batchnorm_eval", "non_contiguous"])
def test_outside_the_envelope_autograd_does_what_it_does(cases, what):
    from halo_amd import norm
    c = cases[("scalar_chunk_and_three", "plain")]
    x0, r0, bn = c["x"], c["r"], c["bn"]
    if what == "batchnorm_eval":
        bn = nn.BatchNorm2d(x0.shape[1]).to(DEV).eval()
    if what == "non_contiguous":
        x0, r0 = x0.transpose(2, 3), r0.transpose(2, 3).contiguous()
    wa, wb = c["wa"].reshape(x0.shape), c["wb"].reshape(x0.shape)

    def run(f):
        x, r = x0.detach().clone(memory_format=torch.preserve_format).requires_grad_(True), r0.clone().requires_grad_(True)
        with torch.autocast("cuda", enabled=what == "autocast"):
            a, b = f(x, r)
            loss = (a * wa).sum() + (b * wb).sum()
        return a, b, torch.autograd.grad(loss, [x, r])

    before = dict(norm.launches)
    y, y_id, got = run(lambda x, r: norm.norm_relu_fork(x, bn, r))
    assert y is y_id and norm.launches == before
    t, _, want = run(lambda x, r: (norm.torch_statement(x, bn, r),) * 2)
    assert N.same_bits(y.detach(), t.detach()) and N.same_bits(got[0], want[0]) and N.same_bits(got[1], want[1])


# ---------------------------------------------------------------- layers

@pytest.fixture
def deterministic_convs():
    """the library's weight backward is not bit-reproducible from call to call without its deterministic algorithms"""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def bottleneck_layer():
    return nn.Sequential(N.Bottleneck(8, 4, 16, downsample=N.down(8, 16)), N.Bottleneck(16, 4, 16), N.Bottleneck(16, 4, 16, dilation=2),
                         N.Bottleneck(16, 4, 16))


def basic_layer():
    return nn.Sequential(N.BasicBlock(8, 8), N.BasicBlock(8, 8), N.BasicBlock(8, 8))


def two_layers():
    return nn.Sequential(bottleneck_layer(), nn.Sequential(N.Bottleneck(16, 4, 32, stride=2, downsample=N.down(16, 32, 2)),
                                                           N.Bottleneck(32, 4, 32)))


class LowAndOut(nn.Module):
    """IntermediateLayerGetter's "low": the chained layer's output goes to two library convs, one of them a further layer's"""

    def __init__(self):
        super().__init__()
        self.layer = bottleneck_layer()
        self.shortcut = nn.Conv2d(16, 6, 1, bias=False)
        self.further = nn.Conv2d(16, 8, 3, 1, 1, bias=False)

    def forward(self, x):
        low = self.layer(x)
        return self.shortcut(low), self.further(low), low


def bind(model):
    """a deep copy whose residual blocks are of subclasses bound by use_fused_frozen_norm (the stand-in classes stay as they are)"""
    from halo_amd.hooks import use_fused_frozen_norm
    twin, subs = copy.deepcopy(model), {}
    for m in twin.modules():
        if type(m) in (N.Bottleneck, N.BasicBlock):
            if type(m) not in subs:
                subs[type(m)] = use_fused_frozen_norm(type(type(m).__name__, (type(m),), {}))
            m.__class__ = subs[type(m)]
    return twin


def three_variants(make, seed):
    """(stock, bound by use_fused_frozen_norm, bound and chained, containers chained) on one seed"""
    from halo_amd.hooks import fuse_residual_chains
    torch.manual_seed(seed)
    stock = N.randomize_norms(make(), seed + 1).to(DEV)
    bound, chained = bind(stock), bind(stock)
    return stock, bound, chained, fuse_residual_chains(chained)


# (model, input shape, containers chained, forked blocks, tails of a bound model that run norm_relu's backward)
LAYERS = {
    "bottlenecks_scalar_route": (bottleneck_layer, (2, 8, 9, 13), 1, 3, 12),
    "bottlenecks_vector_route": (bottleneck_layer, (2, 8, 8, 16), 1, 3, 12),
    "basic_blocks": (basic_layer, (2, 8, 9, 13), 1, 2, 6),
    "two_layers_strided_downsample": (two_layers, (2, 8, 9, 13), 2, 4, 18),
    "output_read_by_two_convs": (LowAndOut, (2, 8, 8, 16), 1, 3, 12),
}


@pytest.mark.parametrize("name", list(LAYERS))
def test_chained_layer_equals_the_bound_and_the_stock_layer(deterministic_convs, name):
    from halo_amd import norm
    make, shape, boxes, forks, tails = LAYERS[name]
    stock, bound, chained, n = three_variants(make, 40 + len(name))
    assert n == boxes
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    g_of = lambda outs: [torch.randn(o.shape, generator=torch.Generator().manual_seed(6 + i)).to(DEV) for i, o in enumerate(outs)]
    want, want_g = N.run_with_grads(stock, x, g_of)
    before = dict(norm.launches)
    mid, mid_g = N.run_with_grads(bound, x, g_of)
    assert norm.launches["bwd"] == before["bwd"] + tails and norm.launches["fork_bwd"] == before["fork_bwd"]
    before = dict(norm.launches)
    got, got_g = N.run_with_grads(chained, x, g_of)
    print(name, {k: norm.launches[k] - before[k] for k in ("fwd", "bwd", "fork_bwd")})
    # every forked block's tail takes its two gradients in one launch; the containers' last blocks, the blocks in front of a
    # downsample and the norms inside the blocks stay under the old key
    assert norm.launches["fork_bwd"] == before["fork_bwd"] + forks and norm.launches["bwd"] == before["bwd"] + tails - forks
    assert norm.launches["fwd"] == before["fwd"] + tails
    assert len(want_g) == len(mid_g) == len(got_g) > 1
    for i, (a, b, c) in enumerate(zip(want, mid, got)):
        assert N.same_bits(a, b) and N.same_bits(a, c), "output %d" % i
    for i, (a, b, c) in enumerate(zip(want_g, mid_g, got_g)):
        assert N.same_bits(a, b) and N.same_bits(a, c), "gradient %d (0: the input's, then the conv weights')" % i


def test_chained_layer_keeps_no_activation_alive_without_the_collector(deterministic_convs):
    _, _, chained, n = three_variants(bottleneck_layer, 77)
    assert n == 1
    x = torch.randn(2, 8, 8, 16, device=DEV)
    g = torch.randn(2, 16, 8, 16, device=DEV)
    params = N.conv_weights(chained)

    def once():
        xin = x.clone().requires_grad_(True)
        out = chained(xin)
        grads = torch.autograd.grad(out, [xin] + params, g)
        del out, grads, xin

    once()                                                   # scale / shift caches and the library's workspaces exist from here on
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        once()
        torch.cuda.synchronize()
        left = torch.cuda.memory_allocated()
    finally:
        gc.enable()
    assert left == base, "%d bytes are still allocated after every reference was dropped" % (left - base)
