"""CPU checks of the chained residual layers (halo_fork_affine_relu_bwd of halo_norm.hip, halo_amd.norm.norm_relu_fork,
halo_amd.hooks.fuse_residual_chains): the entry point is declared and bound, the hook's bookkeeping, which containers it takes,
what a hook on a block does to a call, and the walk's outputs and gradients against the unhooked layer on CPU tensors, where every
tail runs the stock statements."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import norm_ref as N

E_ARG = -1                # HALO_E_ARG of include/halo_hip.h


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


def bottleneck_layer(seed=3):
    torch.manual_seed(seed)
    layer = nn.Sequential(N.Bottleneck(8, 4, 16, downsample=N.down(8, 16)), N.Bottleneck(16, 4, 16), N.Bottleneck(16, 4, 16, dilation=2),
                          N.Bottleneck(16, 4, 16))
    return N.randomize_norms(layer, seed + 1)


def basic_layer(seed=5):
    torch.manual_seed(seed)
    return N.randomize_norms(nn.Sequential(N.BasicBlock(8, 8), N.BasicBlock(8, 8), N.BasicBlock(8, 8)), seed + 1)


def test_header_declares_the_fork_entry_and_the_binding_agrees():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    found = re.findall(r"\bint\s+halo_fork_affine_relu_bwd\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1
    params = [p.strip() for p in found[0].split(",")]
    assert len(params) == 11 and params[0].endswith("g_a") and params[1].endswith("g_b") and params[-1] == "void *stream"
    assert set(re.findall(r"\b(halo_affine_relu\w+)\s*\(", text)) == {"halo_affine_relu_fwd", "halo_affine_relu_bwd"}
    assert re.search(r"#define\s+HALO_ABI_VERSION\s+13\b", text)
    restype, argtypes = _lib.SIGNATURES["halo_fork_affine_relu_bwd"]
    assert restype is ctypes.c_int and len(argtypes) == len(params)
    for kind, p in zip(argtypes, params):
        assert (kind is ctypes.c_int64) == p.startswith("int64_t"), p
    assert hasattr(ctypes.CDLL(_build.build()), "halo_fork_affine_relu_bwd")
    assert _lib.lib().halo_version() == _lib.ABI_VERSION == 13


def test_fork_entry_refuses_bad_arguments_before_any_launch():
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    fork = L.halo_fork_affine_relu_bwd
    assert fork(None, a, a, a, None, a, None, 1, 2, 16, None) == E_ARG              # no g_a
    assert fork(a, None, a, a, None, a, None, 1, 2, 16, None) == E_ARG              # no g_b
    assert fork(a, a, None, a, None, a, None, 1, 2, 16, None) == E_ARG              # no y
    assert "halo_fork_affine_relu_bwd: null argument" in L.halo_last_error().decode()
    assert fork(a, a, a, a, None, None, None, 1, 2, 16, None) == E_ARG              # neither gradient asked for
    assert fork(a, a, a, None, None, a, None, 1, 2, 16, None) == E_ARG              # g_x without scale
    assert fork(a, a, a, a, None, a, a, 1, 0, 16, None) == E_ARG                    # empty shape
    assert fork(a, a, a, a, None, a, a, 1, 2, 1 << 31, None) == _lib.E_UNSUPPORTED
    assert "halo_fork_affine_relu_bwd" in L.halo_last_error().decode()


def test_fork_on_cpu_tensors_returns_one_tensor_twice():
    from halo_amd import norm
    torch.manual_seed(0)
    bn, rbn = N.randomize_norms(N.FrozenBatchNorm2d(3), 1), N.randomize_norms(N.FrozenBatchNorm2d(3), 2)
    x, r = torch.randn(2, 3, 4, 5), torch.randn(2, 3, 4, 5)
    before = dict(norm.launches)
    for args in ((x, bn), (x, bn, r), (x, bn, r, rbn)):
        y, y_id = norm.norm_relu_fork(*args)
        assert y is y_id and torch.equal(y, N.stock_chain(*args))
    xg = x.clone().requires_grad_(True)
    y, y_id = norm.norm_relu_fork(xg, bn, r)
    assert y is y_id and y.requires_grad
    assert norm.launches == before and "fork_bwd" in norm.launches


class _OnDevice:
    """describes a contiguous float32 ROCm tensor without one: the reasons read attributes only"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, *shape, requires_grad=True):
        self.shape, self.requires_grad = torch.Size(shape), requires_grad

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def is_contiguous(self):
        return True


def test_the_fork_has_a_size_rule_of_its_own(monkeypatch):
    from halo_amd import norm
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    assert norm.AUTOGRAD_MIN_ELEMENTS == {"plain": 2 * 1024 * 80 * 160, "affine": 2 * 512 * 80 * 160, "masked": 2 * 512 * 80 * 160}
    assert norm.FORK_AUTOGRAD_MIN_ELEMENTS == 2 * 512 * 80 * 160
    bn, rbn = N.FrozenBatchNorm2d(512), N.FrozenBatchNorm2d(512)
    x, r = _OnDevice(2, 512, 80, 160), _OnDevice(2, 512, 80, 160)
    assert norm.fork_fallback_reason(x, bn, r) is None and norm.fork_fallback_reason(x, bn, r, rbn) is None
    assert "fewer than" in norm.fallback_reason(x, bn, r)                              # norm_relu's own rule is as it was
    small = _OnDevice(2, 512, 80, 159)
    assert "fewer than" in norm.fork_fallback_reason(small, bn, small) and "fewer than" in norm.fork_fallback_reason(small, bn, small, rbn)
    off = _OnDevice(2, 512, 80, 160, requires_grad=False)
    assert norm.fork_fallback_reason(off, bn, off) == "no gradient will be asked for"
    with torch.no_grad():
        assert norm.fork_fallback_reason(x, bn, r) == "no gradient will be asked for"
    assert norm.fork_fallback_reason(x, nn.BatchNorm2d(512).eval(), r) == norm.fallback_reason(x, nn.BatchNorm2d(512).eval(), r)
    assert "channels" in norm.fork_fallback_reason(x, N.FrozenBatchNorm2d(8), r)
    monkeypatch.setattr(norm, "FORK_AUTOGRAD_MIN_ELEMENTS", 0)
    assert norm.fork_fallback_reason(small, bn, small) is None


@pytest.mark.parametrize("make", [bottleneck_layer, basic_layer], ids=["bottleneck", "basic"])
def test_chained_layer_equals_the_unhooked_layer_on_cpu(make):
    from halo_amd import hooks
    stock = make()
    chained = bind(stock)
    names, keys = [n for n, _ in chained.named_modules()], list(chained.state_dict())
    assert hooks.fuse_residual_chains(chained) == 1 and hooks.fuse_residual_chains(chained) == 0
    assert isinstance(chained.__dict__["forward"], hooks._ChainWalk)
    assert [n for n, _ in chained.named_modules()] == names and list(chained.state_dict()) == keys
    assert names == [n for n, _ in stock.named_modules()] and keys == list(stock.state_dict())
    x = torch.randn(2, 8, 9, 13, generator=torch.Generator().manual_seed(7))
    g_of = lambda outs: [torch.randn(o.shape, generator=torch.Generator().manual_seed(8)) for o in outs]
    want, want_g = N.run_with_grads(stock, x, g_of)
    got, got_g = N.run_with_grads(chained, x, g_of)
    assert len(got_g) == len(want_g) > 1
    assert all(N.same_bits(a, b) for a, b in zip(got, want)) and all(N.same_bits(a, b) for a, b in zip(got_g, want_g))
    with torch.no_grad():
        assert N.same_bits(chained(x), stock(x))
    assert hooks.unfuse_residual_chains(chained) == 1 and hooks.unfuse_residual_chains(chained) == 0
    assert "forward" not in chained.__dict__ and type(chained).forward is nn.Sequential.forward
    got, got_g = N.run_with_grads(chained, x, g_of)
    assert all(N.same_bits(a, b) for a, b in zip(got, want)) and all(N.same_bits(a, b) for a, b in zip(got_g, want_g))


def test_walk_forks_in_front_of_blocks_without_a_downsample_only(monkeypatch):
    from halo_amd import hooks, norm
    torch.manual_seed(11)
    stack = nn.Sequential(bottleneck_layer(), nn.Sequential(N.Bottleneck(16, 4, 32, stride=2, downsample=N.down(16, 32, 2)),
                                                            N.Bottleneck(32, 4, 32, act=nn.ReLU6()), N.Bottleneck(32, 4, 32)))
    N.randomize_norms(stack, 12)
    chained = bind(stack)
    assert hooks.fuse_residual_chains(chained) == 2                                  # the two layers; the stack holds no block
    assert "forward" not in chained.__dict__
    calls = []
    single = norm.norm_relu

    def fork(x, bn, residual=None, residual_bn=None):        # what norm_relu_fork does with CPU tensors
        calls.append(("fork", bn, residual is not None))
        return (single(x, bn, residual, residual_bn),) * 2

    def one(x, bn, residual=None, residual_bn=None):
        calls.append(("one", bn, residual is not None))
        return single(x, bn, residual, residual_bn)
    monkeypatch.setattr(norm, "norm_relu_fork", fork)
    monkeypatch.setattr(norm, "norm_relu", one)
    x = torch.randn(1, 8, 8, 8)
    y = chained(x)
    tails = [(kind, bn) for kind, bn, res in calls if res]
    l1, l2 = chained[0], chained[1]
    # layer 1: blocks 0, 1, 2 fork (their successors have no downsample), the last does not; layer 2: block 0 stands in front of a
    # block whose relu is not nn.ReLU, which runs its own forward and hands a plain tensor to the last block
    assert tails == [("fork", l1[0].bn3), ("fork", l1[1].bn3), ("fork", l1[2].bn3), ("one", l1[3].bn3), ("one", l2[0].bn3), ("one", l2[2].bn3)]
    assert N.same_bits(y, stack(x))


def test_containers_that_are_left_alone():
    from halo_amd import hooks
    bound = bind(bottleneck_layer())
    mixed = nn.Sequential(bound[1], nn.ReLU(), bound[2])
    assert hooks.fuse_residual_chains(mixed) == 0 and "forward" not in mixed.__dict__            # a non-residual child
    assert hooks.fuse_residual_chains(nn.Sequential(bound[3])) == 0                              # a single block
    unbound = bottleneck_layer()
    assert hooks.fuse_residual_chains(unbound) == 0 and "forward" not in unbound.__dict__        # the blocks' class is not bound
    assert hooks.fuse_residual_chains(unbound[0].downsample) == 0                                # Sequential(conv, norm)
    mine = bind(bottleneck_layer())
    mine.forward = lambda x: x
    assert hooks.fuse_residual_chains(mine) == 0 and hooks.unfuse_residual_chains(mine) == 0     # an instance-level forward of the user's
    boxed = nn.ModuleList([bound[1], bound[2]])
    assert hooks.fuse_residual_chains(boxed) == 0                                                # not an nn.Sequential
    inner = nn.Sequential(nn.Conv2d(3, 8, 1), bind(bottleneck_layer()))
    assert hooks.fuse_residual_chains(inner) == 1 and "forward" in inner[1].__dict__ and "forward" not in inner.__dict__


def test_a_hook_on_a_block_sends_the_call_through_the_blocks(monkeypatch):
    from halo_amd import hooks
    stock = bottleneck_layer()
    chained = bind(stock)
    assert hooks.fuse_residual_chains(chained) == 1
    x = torch.randn(2, 8, 6, 6)
    bodies = []
    body = hooks.residual_body
    monkeypatch.setattr(hooks, "residual_body", lambda blk, a, b, fork: bodies.append(fork) or body(blk, a, b, fork))
    want = stock(x)
    assert N.same_bits(chained(x), want) and bodies == [True, True, True, False]
    fired = []
    handle = chained[2].register_forward_hook(lambda mod, args, out: fired.append(out.shape))
    del bodies[:]
    assert N.same_bits(chained(x), want)
    assert fired == [want.shape] and bodies == [False] * 4                          # nn.Sequential.forward: every block through __call__
    handle.remove()
    pre = chained[0].register_forward_pre_hook(lambda mod, args: fired.append("pre"))
    del bodies[:]
    assert N.same_bits(chained(x), want) and fired[-1] == "pre" and bodies == [False] * 4
    pre.remove()
    del bodies[:]
    assert N.same_bits(chained(x), want) and bodies == [True, True, True, False]
