"""CPU checks of the separable blocks' pointwise tail (halo_masked_affine_relu_* of halo_norm.hip, halo_amd.norm.norm_relu_dropout2d,
halo_amd.hooks.use_fused_pointwise_norm / use_fused_decoder_dropout): the entry points are declared, listed and exported under ABI
13 and refuse bad arguments before any launch, every clause of the envelope, the identity the operator rests on (ATen's feature
dropout written out: mask, generator state, gradient formula), and the hooks on CPU stand-ins, where every fused pass falls back to
the stock statements."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT
from dwconv_ref import FrozenBatchNorm2d

SYMBOLS = ("halo_masked_affine_relu_fwd", "halo_masked_affine_relu_bwd")
E_ARG, E_UNSUPPORTED = -1, -2


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(halo_masked_\w+)\s*\(", code)) == set(SYMBOLS)
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
        args = re.search(r"\b%s\s*\(([^)]*)\)" % s, code).group(1).split(",")
        assert len(args) == len(_lib.SIGNATURES[s][1]) == 9, s
        # five pointers, three 64-bit extents, the stream: the header's parameter types against the binding's, one by one
        want = [ctypes.c_void_p if "*" in a else ctypes.c_int64 for a in args]
        assert "int64_t" in args[5] and "int64_t" in args[7] and "void *stream" in args[8]
        assert _lib.SIGNATURES[s][1] == want and _lib.SIGNATURES[s][0] is ctypes.c_int, s
    version = int(re.search(r"#define HALO_ABI_VERSION (\d+)", text).group(1))
    assert version == _lib.ABI_VERSION == 13 and _lib.lib().halo_version() == 13       # no exported signature changed


def test_argument_checks_refuse_before_any_launch():
    """every pointer is one HOST buffer: a check that went missing would end in a launch error or worse, never in these codes"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in SYMBOLS:
        fn = getattr(L, name)
        for k in range(5):                                                               # each of the five pointers
            args = [p] * 5
            args[k] = None
            assert fn(*args, 1, 2, 16, None) == E_ARG
            msg = L.halo_last_error().decode()
            assert "null" in msg and name in msg, msg
        for shape in ((0, 2, 16), (1, 0, 16), (1, 2, 0)):
            assert fn(p, p, p, p, p, *shape, None) == E_ARG and "empty" in L.halo_last_error().decode()
        assert fn(p, p, p, p, p, 1, 2, 1 << 31, None) == E_UNSUPPORTED                   # an_plan's limits: offsets inside a plane
        assert fn(p, p, p, p, p, 1 << 20, 1 << 20, 4096, None) == E_UNSUPPORTED          # more workgroups than a grid holds
        assert name in L.halo_last_error().decode()


class _OnDevice:
    """describes a contiguous float32 ROCm tensor without one: the envelope reads attributes only"""
    is_cuda = True

    def __init__(self, *shape, contiguous=True, dtype=torch.float32, device="cpu", requires_grad=False):
        self.shape, self._c, self.dtype, self.device = torch.Size(shape), contiguous, dtype, torch.device(device)
        self.requires_grad = requires_grad

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def is_contiguous(self):
        return self._c


def test_every_clause_of_the_envelope(monkeypatch):
    from halo_amd import norm
    why = norm.dropout_fallback_reason
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    monkeypatch.setitem(norm.AUTOGRAD_MIN_ELEMENTS, "masked", 1000)
    x, bn, drop = _OnDevice(2, 8, 5, 7), FrozenBatchNorm2d(8), nn.Dropout2d(0.1)
    assert drop.training and why(x, bn, drop) is None
    # the dropout module
    for other in (nn.Dropout(0.1), nn.Dropout3d(0.1), nn.Identity(), None):
        assert "nn.Dropout2d" in why(x, bn, other)
    assert "in place" in why(x, bn, nn.Dropout2d(0.1, inplace=True))
    assert "p = 1" in why(x, bn, nn.Dropout2d(1.0))
    # eval mode and p = 0 draw nothing and are norm_relu's business: its envelope and its size rule, whatever p is
    for quiet in (nn.Dropout2d(0.1).eval(), nn.Dropout2d(0.0), nn.Dropout2d(1.0).eval()):
        assert why(x, bn, quiet) is None
        assert why(_OnDevice(2, 8, 5, 7, contiguous=False), bn, quiet) == norm.fallback_reason(_OnDevice(2, 8, 5, 7, contiguous=False), bn)
        small = _OnDevice(2, 8, 5, 7, requires_grad=True)
        assert "autograd" in why(small, bn, quiet) and str(norm.AUTOGRAD_MIN_ELEMENTS["plain"]) in why(small, bn, quiet)
    # section 15's envelope
    assert "(B, C, H, W)" in why(_OnDevice(8, 5, 7), bn, drop) and "(B, C, H, W)" in why([1.0], bn, drop)
    assert "float32" in why(_OnDevice(2, 8, 5, 7, dtype=torch.float16), bn, drop)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert "autocast" in why(x, bn, drop)
    assert "device" in why(torch.zeros(2, 8, 5, 7), bn, drop)                              # CPU tensors: the torch statements
    assert "empty" in why(_OnDevice(0, 8, 5, 7), bn, drop)
    assert "contiguous" in why(_OnDevice(2, 8, 5, 7, contiguous=False), bn, drop)
    assert "plane" in why(_OnDevice(1, 8, 1 << 16, 1 << 15), bn, drop)
    for other in (nn.BatchNorm2d(8).eval(), nn.BatchNorm2d(8), nn.GroupNorm(2, 8), nn.Identity()):
        assert "FrozenBatchNorm2d" in why(x, other, drop)
    assert "channels" in why(x, FrozenBatchNorm2d(6), drop)
    assert "float32 on" in why(x, FrozenBatchNorm2d(8).double(), drop)
    assert "float32 on" in why(_OnDevice(2, 8, 5, 7, device="meta"), bn, drop)
    # the speed rule: its own key, under autograd only, and the other keys keep their values
    assert norm.AUTOGRAD_MIN_ELEMENTS["plain"] == 2 * 1024 * 80 * 160 and norm.AUTOGRAD_MIN_ELEMENTS["affine"] == 2 * 512 * 80 * 160
    few, enough = _OnDevice(1, 8, 5, 24, requires_grad=True), _OnDevice(1, 8, 5, 25, requires_grad=True)
    assert few.numel() == 960 and "autograd" in why(few, bn, drop) and "1000" in why(few, bn, drop)
    assert enough.numel() == 1000 and why(enough, bn, drop) is None
    assert why(_OnDevice(1, 8, 5, 24), bn, drop) is None                                   # no gradient asked for: every size
    with torch.no_grad():
        assert why(few, bn, drop) is None


@pytest.mark.parametrize("seed,p", [(0, 0.1), (1, 0.1), (2, 0.1), (3, 0.1), (11, 0.1), (5, 0.5)])
def test_the_identity_the_operator_rests_on(seed, p):
    """ATen's feature dropout written out -- x.new_empty((B, C, 1, 1)).bernoulli_(1 - p).div_(1 - p) -- is F.dropout2d's mask and
    leaves the generator where F.dropout2d leaves it, and where(pre > 0, g * m, 0) * scale is autograd's gradient of
    dropout2d(relu(x * scale + shift)), bit for bit"""
    B, C, H, W = 2, 16, 4, 8
    gen = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(B, C, H, W, generator=gen).requires_grad_(True)
    g = torch.randn(B, C, H, W, generator=gen)
    scale = (0.25 + 1.5 * torch.rand(C, generator=gen)).view(1, -1, 1, 1)
    scale[0, 1] = -0.75
    shift = (0.4 * torch.randn(C, generator=gen)).view(1, -1, 1, 1)
    torch.manual_seed(seed)
    pre = x * scale + shift
    want = F.dropout2d(F.relu(pre), p, training=True)
    state = torch.get_rng_state()
    want_gx, = torch.autograd.grad(want, x, g)
    torch.manual_seed(seed)
    noise = x.new_empty((B, C, 1, 1)).bernoulli_(1 - p).div_(1 - p)
    assert torch.equal(torch.get_rng_state(), state)
    assert set(noise.unique().tolist()) <= {0.0, float(torch.tensor(1.0).div(1 - p))}
    assert torch.equal(F.relu(pre.detach()) * noise, want.detach())
    assert torch.equal(torch.where(pre.detach() > 0, g * noise, torch.zeros(())) * scale, want_gx)
    # m >= 0: in a kept plane the saved y is positive exactly where the ReLU's output is
    kept = (noise != 0).expand_as(pre)
    assert torch.equal((want.detach() > 0)[kept], (pre.detach() > 0)[kept]) and bool((want.detach()[~kept] == 0).all())


class Block(nn.Module):
    """DepthwiseSeparableConv2d's attribute names and statements; `calls` counts what its forward runs"""

    def __init__(self, cin, cout):
        super().__init__()
        self.depthwise_conv = nn.Conv2d(cin, cin, 3, 1, 1, groups=cin, bias=False)
        self.depthwise_bn = FrozenBatchNorm2d(cin)
        self.depthwise_activate = nn.ReLU(inplace=True)
        self.pointwise_conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.pointwise_bn = FrozenBatchNorm2d(cout)
        self.pointwise_activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.depthwise_conv(x)
        x = self.depthwise_bn(x)
        x = self.depthwise_activate(x)
        x = self.pointwise_conv(x)
        x = self.pointwise_bn(x)
        x = self.pointwise_activate(x)
        return x


def _randomize(module, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, FrozenBatchNorm2d):
                n = m.weight.numel()
                m.weight.copy_(0.25 + 1.5 * torch.rand(n, generator=gen)), m.bias.copy_(0.4 * torch.randn(n, generator=gen))
                m.running_mean.copy_(0.5 * torch.randn(n, generator=gen)), m.running_var.copy_(0.3 + 1.5 * torch.rand(n, generator=gen))
            elif isinstance(m, nn.Conv2d):
                m.weight.copy_(0.5 * torch.randn(m.weight.shape, generator=gen))
    return module


class _Stage(nn.Module):
    """the modules of a hyperbolic v3+ head that v3plus_decoder reads"""

    def __init__(self, block=Block):
        super().__init__()
        self.bottleneck = nn.Sequential(nn.Conv2d(5, 4, 3, padding=1, bias=False), FrozenBatchNorm2d(4), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(3, 2, 1, bias=False), FrozenBatchNorm2d(2), nn.ReLU(inplace=True))
        self.decoder = nn.Sequential(block(6, 4), block(4, 4), nn.Dropout2d(0.5))


def test_hooks_refuse_other_classes_are_idempotent_and_keep_the_previous_forward():
    import halo_amd
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import (fused_dwsep_forward, fused_pointwise_forward, fused_v3plus_hyper_forward, use_fused_decoder_dropout,
                                use_fused_depthwise, use_fused_pointwise_norm)

    class Plain(nn.Module):
        def forward(self, x):
            return x

    for bad in (Plain, nn.Conv2d, nn.Sequential, Block(4, 4), "Block", type("NoModule", (), {})):
        with pytest.raises(TypeError):
            use_fused_pointwise_norm(bad)
    for bad in (Plain, nn.Conv2d, _Stage, Plain(), "Head"):                               # _Stage carries no package forward
        with pytest.raises(TypeError):
            use_fused_decoder_dropout(bad)
    # the block mark, on a class use_fused_depthwise has not bound: a forward of its own, the previous one kept
    Tail = type("Tail", (Block,), {})
    assert use_fused_pointwise_norm(Tail) is Tail and Tail._halo_fused_pointwise_norm is True
    assert Tail.forward is fused_pointwise_forward and Tail._unfused_forward is Block.__dict__["forward"]
    assert use_fused_pointwise_norm(Tail) is Tail and Tail._unfused_forward is Block.__dict__["forward"]       # idempotent
    assert use_fused_depthwise(Tail).forward is fused_dwsep_forward and Tail._halo_fused_pointwise_norm is True
    # the other binding order: the depthwise forward stays bound, and so does what it replaced
    Both = type("Both", (Block,), {})
    use_fused_depthwise(Both)
    assert use_fused_pointwise_norm(Both) is Both and Both.forward is fused_dwsep_forward and Both._unfused_forward is Block.__dict__["forward"]
    assert use_fused_pointwise_norm(type("Child", (Both,), {})).forward is fused_dwsep_forward               # inherited binding
    Named = type("DepthwiseSeparableConv2d", (nn.Module,), {"forward": lambda self, x: x})                   # the reference's name is enough
    assert use_fused_pointwise_norm(Named).forward is fused_pointwise_forward
    assert not hasattr(Block, "_halo_fused_pointwise_norm") and Block.forward is Block.__dict__["forward"]
    # the head mark
    Head = type("Head", (_Stage,), {"forward": v3plus_hyper_forward})
    Reweighting = type("Reweighting", (_Stage,), {"forward": fused_v3plus_hyper_forward})
    assert use_fused_decoder_dropout(Head) is Head and use_fused_decoder_dropout(Head) is Head and Head._halo_fused_decoder_dropout is True
    assert use_fused_decoder_dropout(Reweighting) is Reweighting and use_fused_decoder_dropout(type("Sub", (Head,), {}))
    assert Head.forward is v3plus_hyper_forward and Reweighting.forward is fused_v3plus_hyper_forward        # the forwards stay bound
    assert not hasattr(_Stage, "_halo_fused_decoder_dropout")
    keys = list(Head().state_dict())
    assert keys == list(_Stage().state_dict())                                                                # no parameter, no name
    here = os.path.dirname(halo_amd.__file__)
    init = open(os.path.join(here, "__init__.py")).read() + open(os.path.join(here, "_install.py")).read()
    for name in ("use_fused_pointwise_norm", "use_fused_decoder_dropout", "fused_pointwise_forward"):
        assert name not in init                                                                              # install() binds neither


def _counted(module, calls):
    """count every call of every submodule, by name"""
    hooks = []
    for name, m in module.named_modules():
        if name:
            hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: calls.__setitem__(name, calls.get(name, 0) + 1)))
    return hooks


def _decoder_operands(seed=3):
    gen = torch.Generator().manual_seed(seed)
    pyramid = [torch.randn(2, 3, 4, 6, generator=gen), torch.randn(2, 2, 4, 6, generator=gen)]
    return pyramid, torch.randn(2, 3, 8, 12, generator=gen)


def test_an_unmarked_class_runs_the_statements_it_ran_before():
    """v3plus_decoder of an unmarked head calls self.decoder -- the container, then each child once, each block's six modules once
    -- and returns the bits of the statements written out; a block class without the mark keeps its own forward"""
    from halo_amd.core.models.classifier import v3plus_decoder, v3plus_hyper_forward
    Unmarked = type("Unmarked", (_Stage,), {"forward": v3plus_hyper_forward})
    head = _randomize(Unmarked(), 1).train()
    pyramid, low = _decoder_operands()
    calls = {}
    hooks = _counted(head, calls)
    torch.manual_seed(7)
    got = v3plus_decoder(head, pyramid, low, None)
    state = torch.get_rng_state()
    for h in hooks:
        h.remove()
    names = [n for n, _ in head.named_modules() if n and not n.startswith(("bottleneck.", "shortcut."))]
    assert sorted(calls) == sorted(n for n, _ in head.named_modules() if n) and all(calls[n] == 1 for n in names), calls
    torch.manual_seed(7)
    fused = F.interpolate(head.bottleneck(torch.cat(pyramid, dim=1)), size=low.shape[2:], mode="bilinear", align_corners=True)
    want = head.decoder(torch.cat([fused, head.shortcut(low)], dim=1))
    assert torch.equal(got, want) and torch.equal(torch.get_rng_state(), state)
    assert Block.forward is Block.__dict__["forward"]


@pytest.mark.parametrize("order", ["depthwise_first", "pointwise_first", "pointwise_only"])
def test_marked_classes_fall_back_to_the_same_bits_on_cpu(order):
    """CPU tensors are outside every envelope: a marked head over marked blocks walks its decoder itself (the container and the
    dropout module's own call are not made for the fused pair) and returns the unmarked head's bits, gradients and generator state"""
    from halo_amd.core.models.classifier import v3plus_decoder, v3plus_hyper_forward
    from halo_amd.hooks import use_fused_decoder_dropout, use_fused_depthwise, use_fused_pointwise_norm
    Marked = type("MarkedBlock", (Block,), {})
    if order == "depthwise_first":
        use_fused_depthwise(Marked), use_fused_pointwise_norm(Marked)
    elif order == "pointwise_first":
        use_fused_pointwise_norm(Marked), use_fused_depthwise(Marked)
    else:
        use_fused_pointwise_norm(Marked)
    Head = use_fused_decoder_dropout(type("Head", (_Stage,), {"forward": v3plus_hyper_forward}))
    Unmarked = type("Unmarked", (_Stage,), {"forward": v3plus_hyper_forward})
    plain = _randomize(Unmarked(), 2).train()
    head = Head(Marked).train()
    head.load_state_dict(plain.state_dict())
    pyramid, low = _decoder_operands(4)
    results = []
    for h in (plain, head):
        calls = {}
        hooks = _counted(h, calls)
        leaves = [t.clone().requires_grad_(True) for t in pyramid + [low]]
        torch.manual_seed(9)
        out = v3plus_decoder(h, leaves[:2], leaves[2], None)
        state = torch.get_rng_state()
        for k in hooks:
            k.remove()
        params = [q for q in h.parameters() if q.requires_grad]
        grads = torch.autograd.grad(out, leaves + params, torch.full_like(out, 0.25))
        results.append((out.detach(), state) + grads)
        if h is head:
            # the pair (decoder.1, decoder.2) ran as one statement: neither the block's own call nor the container's was made, and
            # on the CPU that statement is the stock one -- the norm module, F.relu, the dropout module
            assert "decoder" not in calls and "decoder.1" not in calls and calls["decoder.0"] == 1 and calls["decoder.2"] == 1
            assert calls["decoder.1.pointwise_conv"] == 1 and calls["decoder.1.depthwise_conv"] == 1
            assert calls["decoder.1.pointwise_bn"] == 1 and "decoder.1.pointwise_activate" not in calls
    assert bool((results[0][0] == 0).any()) and bool((results[0][0] > 0).any())
    assert all(torch.equal(a, b) for a, b in zip(results[0], results[1]))


def test_operator_on_cpu_is_the_stock_statement():
    from halo_amd.norm import dropout_statement, norm_relu_dropout2d, torch_statement
    bn = _randomize(FrozenBatchNorm2d(6), 5)
    x0, g = torch.randn(2, 6, 5, 7), torch.randn(2, 6, 5, 7)
    inplace = nn.Dropout2d(0.5, inplace=True)          # torch's own backward refuses relu_ followed by an in-place product: forward only
    with torch.no_grad():
        torch.manual_seed(1)
        a = norm_relu_dropout2d(x0.clone(), bn, inplace)
        torch.manual_seed(1)
        assert torch.equal(a, dropout_statement(x0.clone(), bn, inplace))
    for drop in (nn.Dropout2d(0.5), nn.Dropout2d(0.5).eval(), nn.Dropout2d(0.0), nn.Dropout2d(1.0)):
        out = []
        for fn in (norm_relu_dropout2d, dropout_statement):
            x = x0.clone().requires_grad_(True)
            torch.manual_seed(1)
            y = fn(x, bn, drop)
            out.append((y.detach().clone(), torch.autograd.grad(y, x, g)[0], torch.get_rng_state()))
            assert torch.equal(x.detach(), x0)
        assert all(torch.equal(a, b) for a, b in zip(*out))
        if not drop.training or drop.p == 0:
            assert torch.equal(out[0][0], torch_statement(x0.clone(), bn))
