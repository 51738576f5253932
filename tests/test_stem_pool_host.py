"""CPU-side checks of the stem's fused norm + ReLU + max-pool (halo_amd.norm.norm_relu_maxpool, halo_amd.hooks.fuse_norm_relu_pool):
the restatement of its numeric contract (tests/stem_pool_ref.py) against torch's CPU autograd of the stock statements, the envelope,
the hook on a stand-in backbone (on the CPU every call falls back to the stock forwards) and the argument checks of the two ABI
entries.  No device is needed."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

import norm_ref as N
import stem_pool_ref as R
from dwconv_ref import FrozenBatchNorm2d

E_ARG, E_UNSUPPORTED = -1, -2
SHAPES = [(1, 2, 1, 1), (1, 2, 2, 3), (1, 1, 3, 2), (2, 3, 5, 7), (1, 2, 8, 9), (1, 3, 6, 130)]


class _OnDevice:
    """describes a contiguous float32 ROCm tensor without one: pool_fallback_reason reads attributes only"""
    is_cuda, requires_grad = True, False

    def __init__(self, *shape, contiguous=True, dtype=torch.float32):
        self.shape, self._c, self.dtype, self.device = torch.Size(shape), contiguous, dtype, torch.device("cpu")

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(torch.Size(self.shape).numel())

    def is_contiguous(self):
        return self._c


@pytest.fixture(autouse=True)
def described_tensors_count_as_tensors(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_torch_autograd_of_the_stock_statements(shape):
    from halo_amd.dwconv import scale_shift
    bn = R.make_norm(shape[1], 3 + shape[3])
    x, g = R.make_case(shape, 5 + shape[2])
    scale, shift = scale_shift(bn)
    assert float(scale[0]) < 0                                                     # one negative-scale channel
    ref = R.stem_pool_ref(x, scale, shift, g)
    xs = x.clone().requires_grad_(True)
    out, index = nn.MaxPool2d(3, 2, 1, return_indices=True)(torch.relu_(bn(xs)))
    (g_x,) = torch.autograd.grad(out, xs, g)
    assert N.same_bits(ref["out"], out.detach()), "out"
    assert torch.equal(ref["index"], index), "recorded tap"
    assert N.same_bits(ref["g_x"], g_x), "g_x"
    # the tap code is the recorded tap's place in its window, or BLOCKED exactly where the pooled value is not positive
    OH, OW = out.shape[2:]
    oh, ow = torch.arange(OH).view(OH, 1), torch.arange(OW).view(1, OW)
    tap = ref["tap"].long()
    named = (2 * oh - 1 + tap // 3) * shape[3] + (2 * ow - 1 + tap % 3)
    blocked = tap == R.BLOCKED
    assert torch.equal(blocked, out.detach() <= 0) and torch.equal(named[~blocked], index[~blocked])
    if R.planted(shape):
        z = torch.relu(bn(x))
        assert bool(blocked[0, 0, 0, 0]) and float(z[0, 0, :2, :2].max()) == 0    # a window without a positive tap
        assert int(tap[0, 1, 1, 1]) == 0 and float(z[0, 1, 1, 1]) == float(z[0, 1, 2, 2]) == float(out.detach()[0, 1, 1, 1]) > 0    # the first of two equal taps
        top = OH - 1
        assert int(x[-1, -1, 2 * top, :2].isnan().sum()) == 2 and int(tap[-1, -1, top, 0]) == 5      # the last NaN of two
    if x.numel() >= 30:
        assert bool(x.isnan().any()) and bool(x.isinf().any())


POOLS = {
    "kernel 2": nn.MaxPool2d(2, 2, 1), "stride 1": nn.MaxPool2d(3, 1, 1), "padding 0": nn.MaxPool2d(3, 2, 0),
    "dilation 2": nn.MaxPool2d(3, 2, 1, dilation=2), "ceil_mode": nn.MaxPool2d(3, 2, 1, ceil_mode=True),
    "return_indices": nn.MaxPool2d(3, 2, 1, return_indices=True), "average": nn.AvgPool2d(3, 2, 1),
}


@pytest.mark.parametrize("which", list(POOLS))
def test_unserved_pools_run_the_stock_statements(which):
    from halo_amd.norm import norm_relu_maxpool, pool_fallback_reason
    pool, bn = POOLS[which], R.make_norm(3, 11)
    served = nn.MaxPool2d((3, 3), stride=(2, 2), padding=[1, 1], dilation=1)       # pairs are accepted like ints
    on_device = _OnDevice(2, 3, 9, 11)
    assert isinstance(pool_fallback_reason(on_device, bn, pool), str)              # the pool alone decides: x and bn would be served
    assert pool_fallback_reason(on_device, bn, served) is None and pool_fallback_reason(on_device, bn, nn.MaxPool2d(3, 2, 1)) is None
    x, _ = R.make_case((2, 3, 9, 11), 12)
    got, want = norm_relu_maxpool(x, bn, pool), pool(torch.relu_(bn(x)))
    got, want = (got, want) if isinstance(got, torch.Tensor) else (got[0], want[0])
    assert N.same_bits(got, want)


def test_unserved_tensors_and_norms_run_the_stock_statements():
    from halo_amd.norm import norm_relu_maxpool, pool_fallback_reason
    pool, bn = nn.MaxPool2d(3, 2, 1), R.make_norm(3, 13)
    x, g = R.make_case((2, 3, 9, 11), 14)
    assert "ROCm" in pool_fallback_reason(x, bn, pool)                             # a CPU tensor
    assert "float64" in pool_fallback_reason(_OnDevice(2, 3, 9, 11, dtype=torch.float64), bn, pool)
    assert "FrozenBatchNorm2d" in pool_fallback_reason(_OnDevice(2, 3, 9, 11), nn.BatchNorm2d(3).eval(), pool)
    assert "contiguous" in pool_fallback_reason(_OnDevice(2, 3, 9, 11, contiguous=False), bn, pool)
    for xx, norm_module in ((x, bn), (x.double(), bn.double()), (x, nn.BatchNorm2d(3).eval())):
        xs = xx.clone().requires_grad_(True)
        x0 = xs.detach().clone()
        got = norm_relu_maxpool(xs, norm_module, pool)
        (g_got,) = torch.autograd.grad(got, xs, g.to(xx.dtype))
        xr = xx.clone().requires_grad_(True)
        want = pool(torch.relu_(norm_module(xr)))
        (g_want,) = torch.autograd.grad(want, xr, g.to(xx.dtype))
        assert N.same_bits(got.detach(), want.detach()) and N.same_bits(g_got, g_want) and N.same_bits(xs.detach(), x0)


def test_speed_rule_is_a_constant_of_its_own(monkeypatch):
    from halo_amd import norm
    bn, pool = R.make_norm(3, 15), nn.MaxPool2d(3, 2, 1)
    assert "pool" not in norm.AUTOGRAD_MIN_ELEMENTS and isinstance(norm.POOL_AUTOGRAD_MIN_ELEMENTS, int)
    x = _OnDevice(2, 3, 9, 11)
    x.requires_grad = True
    monkeypatch.setattr(norm, "POOL_AUTOGRAD_MIN_ELEMENTS", 2 * 3 * 9 * 11 + 1)
    assert "fewer" in norm.pool_fallback_reason(x, bn, pool)
    with torch.no_grad():
        assert norm.pool_fallback_reason(x, bn, pool) is None                      # without a gradient every size is served
    monkeypatch.setattr(norm, "POOL_AUTOGRAD_MIN_ELEMENTS", 2 * 3 * 9 * 11)
    assert norm.pool_fallback_reason(x, bn, pool) is None


def _stem(model):
    fe = model.feature_extractor if hasattr(model, "feature_extractor") else model
    return fe["bn1"], fe["relu"], fe["maxpool"]


def test_hook_counts_names_fallback_upgrade_and_undo():
    from halo_amd import hooks
    torch.manual_seed(3)
    plain = N.randomize_norms(N.backbone(), 4)
    net = copy.deepcopy(plain)
    keys, names = list(net.state_dict().keys()), [n for n, _ in net.named_modules()]
    assert hooks.fuse_norm_relu_pool(net) == 1 and hooks.fuse_norm_relu_pool(net) == 0
    bn1, relu, pool = _stem(net)
    assert isinstance(bn1.__dict__["forward"], hooks._PoolNorm) and all(isinstance(m.__dict__["forward"], hooks._PoolPass) for m in (relu, pool))
    assert sum("forward" in m.__dict__ for m in net.modules()) == 3                 # the triple and nothing else
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_modules()] == names
    assert hooks.fuse_norm_relu_pairs(net) == 0                                     # the triple is left alone by the pairs hook
    assert isinstance(bn1.__dict__["forward"], hooks._PoolNorm)
    x = torch.randn(2, 3, 33, 47)
    g_of = lambda outs: [torch.full_like(o, 0.25) for o in outs]
    o1, g1 = N.run_with_grads(plain, x, g_of)
    o2, g2 = N.run_with_grads(net, x, g_of)                                         # on the CPU: the three stock forwards
    assert len(o1) == len(o2) and all(torch.equal(a, b) for a, b in zip(o1 + g1, o2 + g2))
    twin = copy.deepcopy(net)                                                       # a copy's triple refers to the copy's modules
    f = _stem(twin)[0].forward
    assert (f.norm, f.act, f.pool) == _stem(twin)
    assert hooks.unfuse_norm_relu_pairs(net) == 0                                   # not the pairs hook's to undo
    assert hooks.unfuse_norm_relu_pool(net) == 1 and hooks.unfuse_norm_relu_pool(net) == 0
    assert all("forward" not in m.__dict__ for m in net.modules())
    o3, g3 = N.run_with_grads(net, x, g_of)
    assert all(torch.equal(a, b) for a, b in zip(o1 + g1, o3 + g3))
    # an existing pair is upgraded
    assert hooks.fuse_norm_relu_pairs(net) == 1 and isinstance(bn1.__dict__["forward"], hooks._PairNorm)
    assert hooks.fuse_norm_relu_pool(net) == 1
    assert isinstance(bn1.__dict__["forward"], hooks._PoolNorm) and isinstance(relu.__dict__["forward"], hooks._PoolPass)
    assert hooks.fuse_norm_relu_pairs(net) == 0 and hooks.unfuse_norm_relu_pairs(net) == 0
    o4, g4 = N.run_with_grads(net, x, g_of)
    assert all(torch.equal(a, b) for a, b in zip(o1 + g1, o4 + g4))
    assert hooks.unfuse_norm_relu_pool(net) == 1 and all("forward" not in m.__dict__ for m in net.modules())


def test_hook_leaves_returned_shared_foreign_and_unserved_modules_alone():
    from halo_amd.hooks import fuse_norm_relu_pool

    def getter(returned, pool=None, act=None):
        layers = {"conv1": nn.Conv2d(3, 4, 1), "bn1": FrozenBatchNorm2d(4), "relu": act or nn.ReLU(inplace=True),
                  "maxpool": pool or nn.MaxPool2d(3, 2, 1)}
        return N.IntermediateLayerGetter(layers, returned)
    assert fuse_norm_relu_pool(getter({"bn1": "pre"})) == 0                         # the norm's own output is returned
    assert fuse_norm_relu_pool(getter({"relu": "act"})) == 0                        # the ReLU's
    assert fuse_norm_relu_pool(getter({"maxpool": "stem"})) == 1                    # the pool's is the triple's
    assert fuse_norm_relu_pool(getter({}, pool=nn.MaxPool2d(2, 2))) == 0 and fuse_norm_relu_pool(getter({}, pool=nn.AvgPool2d(3, 2, 1))) == 0
    assert fuse_norm_relu_pool(getter({}, act=nn.ReLU6())) == 0
    act = nn.ReLU(inplace=True)
    shared = nn.Sequential(nn.Conv2d(3, 4, 1), FrozenBatchNorm2d(4), act, nn.MaxPool2d(3, 2, 1), nn.Conv2d(4, 4, 1), act)
    assert fuse_norm_relu_pool(shared) == 0 and "forward" not in act.__dict__       # one ReLU object in two places
    pool = nn.MaxPool2d(3, 2, 1)
    twice = nn.Sequential(nn.Conv2d(3, 4, 1), FrozenBatchNorm2d(4), nn.ReLU(), pool, nn.Conv2d(4, 4, 1), FrozenBatchNorm2d(4), nn.ReLU(), pool)
    assert fuse_norm_relu_pool(twice) == 0 and "forward" not in pool.__dict__
    for victim in ("bn1", "relu", "maxpool"):
        box = getter({})
        box[victim].forward = lambda x: x                                           # somebody else's instance-level forward
        assert fuse_norm_relu_pool(box) == 0
    plain = nn.ModuleDict({"bn1": FrozenBatchNorm2d(4), "relu": nn.ReLU(), "maxpool": nn.MaxPool2d(3, 2, 1)})     # no container that calls in order
    assert fuse_norm_relu_pool(plain) == 0
    assert fuse_norm_relu_pool(nn.Sequential(nn.BatchNorm2d(4).eval(), nn.ReLU(), nn.MaxPool2d(3, 2, 1))) == 0


def test_argument_errors_are_reported_not_crashed():
    """null pointers, empty shapes and planes past the 32-bit limit: the checks run before anything is launched, so host bytes
    stand in for device memory and no device is needed"""
    from halo_amd import _build, _lib
    assert "halo_maxpool.hip" in _build.SOURCES
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = L.halo_maxpool_affine_relu_fwd, L.halo_maxpool_affine_relu_bwd
    assert fwd(None, None, None, None, None, 0, 0, 0, 0, None) == E_ARG and b"halo_maxpool_affine_relu_fwd" in L.halo_last_error()
    assert bwd(None, None, None, None, 0, 0, 0, 0, None) == E_ARG and b"halo_maxpool_affine_relu_bwd" in L.halo_last_error()
    for missing in range(4):                                                        # x, scale, shift, out; tap alone may be NULL
        ptrs = [a, a, a, a]
        ptrs[missing] = None
        assert fwd(*ptrs, a, 1, 2, 8, 8, None) == E_ARG and b"null" in L.halo_last_error()
        assert bwd(*ptrs, 1, 2, 8, 8, None) == E_ARG and b"null" in L.halo_last_error()      # g, tap, scale, g_x
    for shape in ((0, 2, 8, 8), (1, 0, 8, 8), (1, 2, 0, 8), (1, 2, 8, 0), (1, 2, -1, 8)):
        assert fwd(a, a, a, a, None, *shape, None) == E_ARG and b"empty" in L.halo_last_error()
        assert bwd(a, a, a, a, *shape, None) == E_ARG and b"empty" in L.halo_last_error()
    for shape in ((1, 2, 1 << 16, 1 << 15), (1, 2, 1, (1 << 31) - 1024), (1, 1, 1 << 40, 1 << 40), (1 << 20, 1 << 20, 64, 64)):
        assert fwd(a, a, a, a, a, *shape, None) == E_UNSUPPORTED, shape             # a plane above 2^31 - 1025, or too many workgroups
        assert bwd(a, a, a, a, *shape, None) == E_UNSUPPORTED, shape
