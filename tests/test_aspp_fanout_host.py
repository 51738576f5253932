"""CPU checks of the ASPP fan-out (halo_fan_dwconv3x3_affine_relu_bwd_data of halo_dwconv.hip, halo_amd.fanout,
halo_amd.hooks.use_joined_aspp_gradients): the entry is declared, bound and exported under ABI 13, every argument check refuses
before a launch, the operator on CPU tensors returns the composition with the contract's gradient order, plane_mean is
nn.AdaptiveAvgPool2d((1, 1)) with an unmaterialised gradient, the hook's class checks and routing, and the operand recipe of
tests/fanout_cases.py, which tests/test_gpu_aspp_fanout.py runs on the device, tells the contract's order from a wrong one."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT
import dwconv_ref as R
import dwmulti_cases as K
import fanout_cases as F

ENTRY = "halo_fan_dwconv3x3_affine_relu_bwd_data"
E_ARG, E_UNSUPPORTED = -1, -2

def test_header_binding_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\b(halo_fan_\w+)\s*\(", code) == [ENTRY]
    assert "#define HALO_ABI_VERSION 13" in text and _lib.ABI_VERSION == 13
    assert ENTRY in _lib.SIGNATURES and hasattr(ctypes.CDLL(_build.build()), ENTRY)
    assert _lib.lib().halo_version() == 13
    multi = _lib.SIGNATURES["halo_multi_dwconv3x3_affine_relu_bwd_data"][1]
    assert len(_lib.SIGNATURES[ENTRY][1]) == len(multi) + 3 and _lib.SIGNATURES[ENTRY][1][:len(multi) - 1] == multi[:-1]


def test_argument_checks_refuse_before_any_launch():
    """every pointer is one HOST buffer: a check that went missing would end in a launch error or worse, never in these codes"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fan = getattr(L, ENTRY)
    limit = L.halo_multi_dwconv_max_plane()
    d3, d5 = (ctypes.c_int64 * 3)(6, 12, 18), (ctypes.c_int64 * 5)(1, 2, 3, 4, 5)
    g3 = (ctypes.c_void_p * 3)(p.value, None, p.value)
    none3 = (ctypes.c_void_p * 3)(None, None, None)
    e2, f2 = (ctypes.c_void_p * 5)(p.value, None, None, None, None), (ctypes.c_int32 * 5)(0, 1, 0, 0, 0)

    def refused(rc, code, word):
        msg = L.halo_last_error().decode()
        assert rc == code and word in msg and ENTRY in msg, (rc, msg)

    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 3, d3, -1, e2, f2, None), E_ARG, "extra addends")
    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 3, d3, 5, e2, f2, None), E_ARG, "extra addends")
    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 3, d3, 2, None, f2, None), E_ARG, "null")
    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 3, d3, 2, e2, None, None), E_ARG, "null")
    refused(fan(none3, p, p, p, p, 1, 2, 4, 4, 3, d3, 2, e2, f2, None), E_ARG, "every gradient")
    refused(fan(none3, p, p, p, p, 1, 2, 4, 4, 3, d3, 0, None, None, None), E_ARG, "every gradient")
    # the existing entry's checks
    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 1, d3, 2, e2, f2, None), E_ARG, "dilations")
    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 5, d5, 2, e2, f2, None), E_ARG, "dilations")
    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 3, None, 2, e2, f2, None), E_ARG, "null")
    refused(fan(None, p, p, p, p, 1, 2, 4, 4, 3, d3, 2, e2, f2, None), E_ARG, "null")
    for missing in range(1, 5):
        args = [g3, p, p, p, p]
        args[missing] = None
        refused(fan(*args, 1, 2, 4, 4, 3, d3, 2, e2, f2, None), E_ARG, "null")
    refused(fan(g3, p, p, p, p, 1, 0, 4, 4, 3, d3, 2, e2, f2, None), E_ARG, "empty")
    refused(fan(g3, p, p, p, p, 1, 2, 4, 4, 3, (ctypes.c_int64 * 3)(6, 0, 18), 2, e2, f2, None), E_ARG, "dilation")
    refused(fan(g3, p, p, p, p, 1, 2, 1 << 25, 4, 3, d3, 2, e2, f2, None), E_UNSUPPORTED, "planes")
    refused(fan(g3, p, p, p, p, 1, 2, limit + 1, 1, 3, d3, 2, e2, f2, None), E_UNSUPPORTED, "plane of %d x 1" % (limit + 1))


def _blocks(C=5):
    torch.manual_seed(5)
    blocks = []
    for d in (1, 2, 3):
        bn = R.FrozenBatchNorm2d(C)
        bn.weight.copy_(torch.rand(C) + 0.5), bn.bias.copy_(torch.randn(C)), bn.running_mean.copy_(torch.randn(C)), bn.running_var.copy_(torch.rand(C) + 0.5)
        blocks.append((nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False), bn, nn.ReLU(inplace=True)))
    return blocks


def test_operator_on_cpu_tensors_is_the_composition_with_the_contracts_order():
    from halo_amd import dwconv, fanout
    from halo_amd.dwconv import depthwise_bn_relu
    blocks = _blocks()
    x = torch.randn(2, 5, 9, 10, requires_grad=True)
    gs = [torch.randn(2, 5, 9, 10) for _ in blocks]
    es = [torch.randn(2, 5, 9, 10), torch.randn(2, 5, 1, 1).expand(2, 5, 9, 10)]
    before = (dict(fanout.launches), dict(dwconv.launches))
    assert sorted(fanout.launches) == ["fan_bwd"]
    assert fanout.fan_fallback_reason(x, blocks, 2) == "block 0: x is not on a ROCm device"
    ys, xs = fanout.fan_depthwise_bn_relu(x, blocks, 2)
    assert isinstance(ys, tuple) and isinstance(xs, tuple) and len(ys) == 3 and len(xs) == 2
    want = [depthwise_bn_relu(x, *b) for b in blocks]
    assert all(torch.equal(a, b) for a, b in zip(ys, want))
    assert all(t.data_ptr() == x.data_ptr() and t.shape == x.shape and t.stride() == x.stride() and torch.equal(t, x) for t in xs)
    # the readers: a weighted sum (a dense gradient) and a per-plane product (a stride-0 gradient)
    got = torch.autograd.grad(list(ys) + list(xs), [x] + [b[0].weight for b in blocks], gs + es)
    parts = [torch.autograd.grad(y, [x, b[0].weight], g) for y, b, g in zip(want, blocks, gs)]
    contract = (((parts[0][0] + parts[1][0]) + parts[2][0]) + es[0]) + es[1]
    assert torch.equal(got[0], contract)
    assert not torch.equal(got[0], (((es[0] + es[1]) + parts[0][0]) + parts[1][0]) + parts[2][0])       # the inputs tell the orders apart
    assert all(torch.equal(a, p[1]) for a, p in zip(got[1:], parts))
    assert (dict(fanout.launches), dict(dwconv.launches)) == before
    # an unused alias and an unused output are left out
    ys, xs = fanout.fan_depthwise_bn_relu(x, blocks, 2)
    got = torch.autograd.grad([ys[0], ys[2], xs[1]], x, [gs[0], gs[2], es[1]])[0]
    assert torch.equal(got, (parts[0][0] + parts[2][0]) + es[1])
    # no gradient for x: x itself, `readers` times
    with torch.no_grad():
        ys, xs = fanout.fan_depthwise_bn_relu(x, blocks, 3)
    assert len(xs) == 3 and all(t is x for t in xs) and all(torch.equal(a, b) for a, b in zip(ys, want))
    x0 = x.detach()
    assert all(t is x0 for t in fanout.fan_depthwise_bn_relu(x0, blocks, 1)[1])
    for bad in (0, 5, True, 2.0):
        assert "further readers, 1 to 4" in fanout.fan_fallback_reason(x, blocks, bad)


class _OnDevice:
    """describes a float32 ROCm tensor without one: the fallback reasons read attributes only"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, *shape, requires_grad=True):
        self.shape, self.requires_grad = torch.Size(shape), requires_grad

    def dim(self):
        return len(self.shape)


def test_fallback_reason_is_the_multi_envelope_plus_readers_plus_a_wanted_gradient(monkeypatch):
    from halo_amd import dwconv
    from halo_amd.fanout import fan_fallback_reason as why
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    blocks = _blocks()
    x = _OnDevice(2, 5, 8, 10)
    assert "speed rule" in why(x, blocks, 2) and why(x, blocks, 2) == dwconv.multi_fallback_reason(x, blocks)
    monkeypatch.setattr(dwconv, "MULTI_MIN_ELEMENTS", 0)
    assert all(why(x, blocks, r) is None for r in (1, 2, 3, 4))
    assert "0 further readers" in why(x, blocks, 0) and "5 further readers" in why(x, blocks, 5)
    assert why(_OnDevice(2, 5, 8, 10, requires_grad=False), blocks, 2).startswith("no gradient will be asked for x")
    with torch.no_grad():
        assert why(x, blocks, 2).startswith("no gradient will be asked for x")
    assert why(x, blocks[:1], 2) == dwconv.multi_fallback_reason(x, blocks[:1]) != None                         # noqa: E711
    inside, outside = K.edge_shapes(dwconv.multi_max_plane())
    two = [b[:2] for b in _blocks(2)[:2]]
    assert why(_OnDevice(*inside), two, 2) is None and "plane of" in why(_OnDevice(*outside), two, 2)


@pytest.mark.parametrize("shape", [(2, 3, 13, 79), (1, 2, 80, 160), (2, 3, 1, 1)])
def test_plane_mean_is_the_adaptive_pool_with_an_unmaterialised_gradient(shape):
    from halo_amd.fanout import is_per_plane, plane_mean
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen)
    g = torch.randn(*shape[:2], 1, 1, generator=gen)
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = plane_mean(a), nn.AdaptiveAvgPool2d((1, 1))(b)
    assert ya.shape == yb.shape == shape[:2] + (1, 1) and torch.equal(ya, yb)
    ga, gb = torch.autograd.grad(ya, a, g)[0], torch.autograd.grad(yb, b, g)[0]
    assert ga.shape == gb.shape == shape and torch.equal(ga, gb)
    assert is_per_plane(ga) and ga.untyped_storage().nbytes() == 4 * shape[0] * shape[1]
    if shape[2:] != (1, 1):                                # a 1 x 1 plane is one value per plane whatever its strides say
        assert ga.stride()[2:] == (0, 0) and not is_per_plane(gb.contiguous())


def _v3plus_heads():
    from halo_amd.core.models.classifier import v3plus_forward, v3plus_hyper_forward
    from halo_amd.hooks import fused_v3plus_hyper_forward
    forwards = (v3plus_hyper_forward, fused_v3plus_hyper_forward, v3plus_forward)
    return [type("Head%d" % i, (nn.Module,), {"forward": f}) for i, f in enumerate(forwards)], forwards


def test_hook_marks_only_classes_with_a_v3plus_forward():
    import halo_amd
    from halo_amd.core.models.classifier import v2_hyper_forward
    from halo_amd.hooks import use_joined_aspp_gradients

    class Plain(nn.Module):
        def forward(self, x):
            return x

    class V2(nn.Module):
        forward = v2_hyper_forward

    heads, forwards = _v3plus_heads()
    for bad in (Plain, V2, nn.Conv2d, Plain(), "Head", None):
        with pytest.raises(TypeError, match="use_joined_aspp_gradients: "):
            use_joined_aspp_gradients(bad)
    with pytest.raises(TypeError, match="V2 does not carry one of halo_amd's v3\\+ forwards; bind one first with"):
        use_joined_aspp_gradients(V2)
    for Head, f in zip(heads, forwards):
        assert not hasattr(Head, "_halo_joined_aspp_gradients")
        assert use_joined_aspp_gradients(Head) is Head and use_joined_aspp_gradients(Head) is Head and Head._halo_joined_aspp_gradients is True
        assert Head.forward is f and not hasattr(Head, "_halo_fused_aspp_depthwise")
    Child = type("Child", (heads[0],), {})
    assert use_joined_aspp_gradients(Child) is Child
    here = os.path.dirname(halo_amd.__file__)
    init = open(os.path.join(here, "__init__.py")).read() + open(os.path.join(here, "_install.py")).read()
    assert "use_joined_aspp_gradients" not in init and "use_joined_aspp_gradients" not in inspect.getsource(halo_amd.install)
    for f in forwards:
        src = inspect.getsource(f)
        assert "pyramid, pooled = pooled_aspp_pyramid(self, top)" in src and "self.global_branch(top)" not in src


def test_unmarked_and_half_marked_heads_run_the_old_statements():
    from halo_amd import fanout, hooks
    from halo_amd.core.models.classifier import pooled_aspp_pyramid, v3plus_forward
    calls = []

    class Branch(nn.Module):
        def __init__(self, k):
            super().__init__()
            self.k = k

        def forward(self, x):
            calls.append((self.k, x))
            return x + self.k

    class Unmarked(nn.Module):
        forward = v3plus_forward

        def __init__(self):
            super().__init__()
            self.parallel_branches = nn.ModuleList([Branch(k) for k in range(4)])
            self.global_branch = Branch(9)

    x = torch.zeros(1, 2, 3, 3)
    OnlyJoined = hooks.use_joined_aspp_gradients(type("OnlyJoined", (Unmarked,), {}))
    Both = hooks.use_fused_aspp_depthwise(hooks.use_joined_aspp_gradients(type("Both", (Unmarked,), {})))      # no served run: the old statements
    before = dict(fanout.launches)
    for cls in (Unmarked, OnlyJoined, Both):
        calls.clear()
        pyramid, pooled = pooled_aspp_pyramid(cls(), x)
        assert [k for k, _ in calls] == [0, 1, 2, 3, 9] and all(t is x for _, t in calls)
        assert [float(o[0, 0, 0, 0]) for o in pyramid] == [0.0, 1.0, 2.0, 3.0] and float(pooled[0, 0, 0, 0]) == 9.0
    assert not hasattr(Unmarked, "_halo_joined_aspp_gradients") and fanout.launches == before


def test_marked_head_on_cpu_tensors_is_the_unmarked_head():
    from euclid_head_standin import Block, EuclidHead
    from halo_amd import dwconv, fanout, hooks
    Fused = hooks.use_fused_depthwise(type("Fused", (Block,), {}))
    Base = hooks.use_v3plus_forward(type("Base", (EuclidHead,), {}))
    Marked = hooks.use_joined_aspp_gradients(hooks.use_fused_aspp_depthwise(hooks.use_v3plus_forward(type("Marked", (EuclidHead,), {}))))
    torch.manual_seed(3)
    with torch.no_grad():
        base, marked = Base(Fused, p=0.5).eval(), Marked(Fused, p=0.5).eval()
    keys, modules = list(base.state_dict()), [n for n, _ in base.named_modules()]
    marked.load_state_dict(base.state_dict())
    gen = torch.Generator().manual_seed(4)
    feats = {"out": torch.randn(2, 24, 9, 13, generator=gen), "low": torch.randn(2, 12, 33, 49, generator=gen)}
    before = (dict(dwconv.launches), dict(fanout.launches))
    outs = []
    for head in (base, marked):
        top = feats["out"].clone().requires_grad_(True)
        out, dec = head({"out": top, "low": feats["low"]})
        outs.append((out.detach(), dec.detach(), torch.autograd.grad(out.square().sum(), top)[0]))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and (dict(dwconv.launches), dict(fanout.launches)) == before
    assert list(marked.state_dict()) == keys and [n for n, _ in marked.named_modules()] == modules


def test_plane_mean_stands_in_only_for_a_plain_sequential_that_starts_with_the_pool():
    from halo_amd.core.models.classifier import _plane_mean_branch as ok

    def branch(pool=None):
        return nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)) if pool is None else pool, nn.Conv2d(3, 2, 1), nn.ReLU())

    assert ok(branch()) and ok(branch(nn.AdaptiveAvgPool2d(1)))
    assert not ok(branch(nn.AdaptiveAvgPool2d(2))) and not ok(branch(nn.AdaptiveAvgPool2d((1, 2)))) and not ok(branch(nn.AdaptiveMaxPool2d(1)))
    assert not ok(nn.Sequential()) and not ok(nn.AdaptiveAvgPool2d(1)) and not ok(nn.ModuleList([nn.AdaptiveAvgPool2d(1)]))
    hooked = branch()
    handle = hooked.register_forward_hook(lambda m, i, o: None)
    assert not ok(hooked)
    handle.remove()
    assert ok(hooked)
    hooked[0].register_forward_pre_hook(lambda m, i: None)
    assert not ok(hooked)
    own = branch()
    own.forward = lambda x: x
    assert not ok(own)
    assert not ok(type("Sub", (nn.Sequential,), {"forward": lambda self, x: x})(nn.AdaptiveAvgPool2d(1)))


@pytest.mark.parametrize("name", list(K.CASES))
def test_operands_tell_the_contracts_order_from_a_wrong_one(name):
    """On the CPU, over the device test's operands: the blocks' shares (float64 reference values rounded to float32 stand in for
    the device's -- only their magnitudes matter here) and the extras added in the contract's order against the extras added first.
    Every case outside F.ORDER_BLIND must give two different results, or the device test could not see mutation (2)."""
    assert set(F.ORDER_BLIND) <= {"one_pixel", "one_row", "one_column"}
    cs = K.case(name)
    m = F.extras_count(name)
    es = F.extras_for(name)
    B, C, H, W, _ = K.CASES[name][0]
    assert len(es) == m and all(e.dtype == np.float32 for e in es) and es[0].shape == (B, C, H, W) and es[1].shape == (B, C)
    shares = []
    for c in cs:
        pre, _ = R.forward(c)
        shares.append(torch.from_numpy(R.grad_x(c, pre > 0)[0].astype(np.float32)))
    es = [torch.from_numpy(e) if e.ndim == 4 else torch.from_numpy(e)[:, :, None, None].expand(B, C, H, W) for e in es]
    contract = None
    for t in shares + es:
        contract = t.clone() if contract is None else contract + t
    wrong = None
    for t in es + shares:
        wrong = t.clone() if wrong is None else wrong + t
    if name in F.ORDER_BLIND:
        return
    assert not torch.equal(contract, wrong), name
