"""CPU checks of the Euclidean DeepLab-v3+ head on the package's forward (halo_amd.core.models.classifier.v3plus_forward,
halo_amd.hooks.use_v3plus_forward / run_decoder_pair) and of the two-output norm + ReLU + Dropout2d pass behind it
(halo_dropout_pair_* of halo_norm.hip, halo_amd.norm.norm_relu_dropout2d_pair): the bound and marked reference head against the
reference head itself where its tree is present, the hook's contract on stand-ins, the entry points' declarations and argument
checks.  On CPU tensors every operator takes its stock statements, so every comparison is torch.equal."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from euclid_head_standin import Block, EuclidHead

SYMBOLS = ("halo_dropout_pair_fwd", "halo_dropout_pair_bwd")
E_ARG, E_UNSUPPORTED = -1, -2
REF = os.environ.get("HALO_REFERENCE", "/root/reference")          # as tests/golden/make_fixtures.py
HEAD_MARKS = ("use_device_resize", "use_fused_decoder_front", "use_folded_image_pooling", "use_fused_decoder_dropout")


def _mark_everything(head_cls, block_cls):
    """use_v3plus_forward plus every head-level mark on head_cls, both block hooks on block_cls"""
    from halo_amd import hooks
    hooks.use_v3plus_forward(head_cls)
    for name in HEAD_MARKS:
        getattr(hooks, name)(head_cls)
    hooks.use_fused_feature_reweighting(head_cls)
    hooks.use_fused_depthwise(block_cls), hooks.use_fused_pointwise_norm(block_cls)
    return head_cls


def _reblock(head, old_cls, new_cls):
    """give every old_cls block of this one head the (hooked) subclass: the shared block class stays as it is"""
    for m in head.modules():
        if type(m) is old_cls:
            m.__class__ = new_cls
    return head


def _randomize_norms(module, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if type(m).__name__ == "FrozenBatchNorm2d":
                n = m.weight.numel()
                m.weight.copy_(0.25 + 1.5 * torch.rand(n, generator=gen)), m.bias.copy_(0.4 * torch.randn(n, generator=gen))
                m.running_mean.copy_(0.5 * torch.randn(n, generator=gen)), m.running_var.copy_(0.3 + 1.5 * torch.rand(n, generator=gen))
    return module


def _step(head, feats, size, seed):
    """(out, decoder_out, generator state, every parameter gradient of out.sum()) of one seeded call"""
    head.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    out, dec = head({k: v.clone() for k, v in feats.items()}, size=size)
    state = torch.get_rng_state()
    out.sum().backward()
    named = [(n, p) for n, p in head.named_parameters() if p.requires_grad]
    assert all(p.grad is not None for _, p in named)
    return [out.detach(), dec.detach(), state] + [p.grad.clone() for _, p in named], ["out", "decoder_out", "generator"] + [n for n, _ in named]


# ---------------------------------------------------------------- (a) the reference's own head

@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "core")), reason="the reference's tree is not present")
@pytest.mark.parametrize("reduced,hfr", [(512, False), (64, True), (64, False), (512, True)])
def test_bound_reference_head_equals_the_reference_head_on_cpu(reduced, hfr):
    from halo_amd import hooks
    from halo_amd.core.models.classifier import v3plus_forward
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_dwconv_fixtures import import_blocks
    RefBlock, Frozen = import_blocks()
    Ref = sys.modules["core.models.classifier"].DepthwiseSeparableASPP
    build = lambda cls: cls(32, [1, 6, 12, 18], [1, 6, 12, 18], 7, Frozen, hfr, reduced_channels=reduced)
    torch.manual_seed(3)
    plain = _randomize_norms(build(Ref), 4)
    assert plain.old_decoder == (reduced == 512 and not hfr)
    Hooked = type("HookedBlock", (RefBlock,), {})
    Bound = _mark_everything(type("Bound", (Ref,), {}), Hooked)
    assert Bound.forward is v3plus_forward and Bound._unfused_forward is Ref.__dict__["forward"]
    bound = _reblock(build(Bound), RefBlock, Hooked)
    assert type(bound.decoder[1]) is Hooked and Hooked.forward is hooks.fused_dwsep_forward and Hooked._halo_fused_pointwise_norm
    bound.load_state_dict(plain.state_dict())
    assert hooks.fuse_norm_relu_pairs(bound) == 4                       # parallel_branches[0], global_branch, bottleneck, shortcut
    assert list(bound.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in bound.named_modules()] == [n for n, _ in plain.named_modules()]
    gen = torch.Generator().manual_seed(5)
    feats = {"out": torch.randn(2, 32, 5, 7, generator=gen), "low": torch.randn(2, 256, 17, 25, generator=gen)}
    for mode in ("eval", "train"):
        getattr(plain, mode)(), getattr(bound, mode)()
        for size in (None, (33, 49)):
            want, names = _step(plain, feats, size, 6)
            got, _ = _step(bound, feats, size, 6)
            assert tuple(got[0].shape[2:]) == (size or (17, 25)) and tuple(got[1].shape[2:]) == (17, 25)
            for name, a, b in zip(names, want, got):
                assert a.shape == b.shape and torch.equal(a, b), (mode, size, name)
            assert float(want[0].std()) > 0
    assert Ref.forward is Ref.__dict__["forward"] and Ref.forward.__name__ == "forward"          # the reference classes are untouched
    assert RefBlock.forward.__name__ == "forward" and not hasattr(RefBlock, "_halo_fused_pointwise_norm")


# ---------------------------------------------------------------- (b) the hooks on stand-ins

@pytest.mark.parametrize("old,hfr", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("marked", [False, True], ids=["bound", "bound_and_marked"])
def test_bound_stand_in_equals_its_own_forward_on_cpu(old, hfr, marked):
    """the stand-in's forward is the reference's statements: v3plus_forward, unmarked and under every mark, returns their bits"""
    from halo_amd import hooks
    torch.manual_seed(1)
    plain = EuclidHead(Block, old=old, hfr=hfr, p=0.5)
    Bound = hooks.use_v3plus_forward(type("Bound", (EuclidHead,), {}))
    Hooked = type("Hooked", (Block,), {})
    if marked:
        _mark_everything(Bound, Hooked)
    bound = Bound(Hooked, old=old, hfr=hfr, p=0.5)
    bound.load_state_dict(plain.state_dict())
    if marked:
        assert hooks.fuse_norm_relu_pairs(bound) == 4
    gen = torch.Generator().manual_seed(2)
    feats = {"out": torch.randn(2, 24, 9, 13, generator=gen), "low": torch.randn(2, 12, 33, 49, generator=gen)}
    for mode in ("eval", "train"):
        getattr(plain, mode)(), getattr(bound, mode)()
        for size in (None, (40, 50)):
            want, names = _step(plain, feats, size, 7)
            got, _ = _step(bound, feats, size, 7)
            for name, a, b in zip(names, want, got):
                assert torch.equal(a, b), (mode, size, name)
    if old:                                            # the dropout really dropped planes: out is not the classifier conv of decoder_out
        with torch.no_grad():
            assert not torch.equal(plain.decoder[3](want[1]), want[0])


def test_use_v3plus_forward_refuses_other_classes_is_idempotent_and_keeps_the_previous_forward():
    import halo_amd
    from halo_amd import hooks
    from halo_amd.core.models.classifier import v3plus_forward, v3plus_hyper_forward

    class Plain(nn.Module):
        def forward(self, x):
            return x

    class NoDecoder(nn.Module):                        # five of the six attributes
        def __init__(self):
            super().__init__()
            self.parallel_branches = self.global_branch = self.bottleneck = self.shortcut = None
            self.old_decoder = True

    class HyperHead(EuclidHead):                       # the six attributes and conv_seg: a hyperbolic head
        def __init__(self):
            super().__init__()
            self.conv_seg = nn.Identity()

    named_hyper = type("DepthwiseSeparableASPP_Hyper", (nn.Module,), {"forward": v3plus_hyper_forward})
    for bad in (Plain, NoDecoder, HyperHead, named_hyper, nn.Conv2d, EuclidHead(), "EuclidHead", None, type("NoModule", (), {})):
        with pytest.raises(TypeError):
            hooks.use_v3plus_forward(bad)
    Head = type("Head", (EuclidHead,), {})
    assert hooks.use_v3plus_forward(Head) is Head and Head.forward is v3plus_forward
    assert Head._unfused_forward is EuclidHead.__dict__["forward"]
    assert hooks.use_v3plus_forward(Head) is Head and Head._unfused_forward is EuclidHead.__dict__["forward"]       # idempotent
    Sub = type("Sub", (Head,), {})
    assert hooks.use_v3plus_forward(Sub) is Sub and "forward" not in Sub.__dict__                                   # inherited binding
    Named = type("DepthwiseSeparableASPP", (nn.Module,), {"forward": lambda self, x, size=None: x})               # the reference's name is enough
    assert hooks.use_v3plus_forward(Named).forward is v3plus_forward
    assert EuclidHead.forward is EuclidHead.__dict__["forward"] and not hasattr(EuclidHead, "_unfused_forward")
    torch.manual_seed(0)
    a, b = EuclidHead(), Head()
    assert list(a.state_dict()) == list(b.state_dict())
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    here = os.path.dirname(halo_amd.__file__)
    init = open(os.path.join(here, "__init__.py")).read() + open(os.path.join(here, "_install.py")).read()
    for name in ("use_v3plus_forward", "v3plus_forward", "run_decoder_pair"):
        assert name not in init                                                                                    # install() binds none of it


def test_head_level_marks_accept_the_class_once_it_is_bound():
    from halo_amd import hooks
    from halo_amd.core.models.classifier import v3plus_forward
    attrs = {"use_device_resize": "_halo_device_resize", "use_fused_decoder_front": "_halo_fused_decoder_front",
             "use_folded_image_pooling": "_halo_folded_image_pooling", "use_fused_decoder_dropout": "_halo_fused_decoder_dropout"}
    assert v3plus_forward in hooks._package_forwards()[1:] and len(hooks._package_forwards()) == 4
    for name in HEAD_MARKS:
        Head = type("Head", (EuclidHead,), {})
        with pytest.raises(TypeError):
            getattr(hooks, name)(Head)
        assert not hasattr(Head, attrs[name])
        hooks.use_v3plus_forward(Head)
        assert getattr(hooks, name)(Head) is Head and getattr(Head, attrs[name]) is True
        assert Head.forward is v3plus_forward and not hasattr(EuclidHead, attrs[name])


def test_feature_reweighting_marks_the_bound_class_and_leaves_its_forward(monkeypatch):
    from halo_amd import hfr, hooks
    from halo_amd.core.models.classifier import v3plus_forward
    Head = hooks.use_v3plus_forward(type("Head", (EuclidHead,), {}))
    assert not getattr(Head, "_halo_fused_feature_reweighting", False)
    assert hooks.use_fused_feature_reweighting(Head) is Head
    assert Head.forward is v3plus_forward and Head._halo_fused_feature_reweighting is True
    assert Head._unfused_forward is EuclidHead.__dict__["forward"]                     # what use_v3plus_forward replaced, still
    # its behaviour on any other class is what it was: the hyperbolic forward is bound
    Other = type("Other", (EuclidHead,), {})
    assert hooks.use_fused_feature_reweighting(Other).forward is hooks.fused_v3plus_hyper_forward
    assert not hasattr(Other, "_halo_fused_feature_reweighting")
    # the mark decides which of halo_amd.hfr's two statements the forward calls
    torch.manual_seed(0)
    head, plain = Head(old=False, hfr=True).eval(), hooks.use_v3plus_forward(type("Plain", (EuclidHead,), {}))(old=False, hfr=True).eval()
    plain.load_state_dict(head.state_dict())
    feats = {"out": torch.randn(1, 24, 4, 5), "low": torch.randn(1, 12, 7, 9)}
    calls = []
    real = hfr.weighted_normalize, hfr.torch_statement
    monkeypatch.setattr(hfr, "weighted_normalize", lambda x, mlp: (calls.append("fused"), real[0](x, mlp))[1])
    monkeypatch.setattr(hfr, "torch_statement", lambda x, mlp: (calls.append("stock"), real[1](x, mlp))[1])
    with torch.no_grad():
        head(feats)
        assert calls[0] == "fused"                                                     # on the CPU it goes on to the stock statement itself
        del calls[:]
        plain(feats)
        assert calls == ["stock"]


def test_old_layout_walk_pairs_decoder_1_with_its_dropout():
    """unmarked: every decoder module is called once, in order; marked over marked blocks: decoder[1] and decoder[2] run as one
    statement (on the CPU the stock one: the norm module, F.relu, the dropout module) and decoder_out is its first result"""
    from halo_amd import hooks
    calls = []

    def counted(head):
        del calls[:]
        return [m.register_forward_hook(lambda mod, i, o, name=name: calls.append(name)) for name, m in head.named_modules()
                if name.startswith("decoder")]

    feats = {"out": torch.randn(2, 24, 4, 5), "low": torch.randn(2, 12, 7, 9)}
    Unmarked = hooks.use_v3plus_forward(type("Unmarked", (EuclidHead,), {}))
    torch.manual_seed(0)
    head = Unmarked(p=0.5).train()
    hooks_ = counted(head)
    head(feats)
    assert [c for c in calls if c.count(".") == 1] == ["decoder.0", "decoder.1", "decoder.2", "decoder.3"] and "decoder" not in calls
    Marked = hooks.use_fused_decoder_dropout(hooks.use_v3plus_forward(type("Marked", (EuclidHead,), {})))
    Hooked = hooks.use_fused_pointwise_norm(type("Hooked", (Block,), {}))
    marked = Marked(Hooked, p=0.5).train()
    marked.load_state_dict(head.state_dict())
    for h in hooks_:
        h.remove()
    counted(marked)
    torch.manual_seed(1)
    out, dec = marked(feats)
    assert "decoder.1" not in calls and calls.count("decoder.2") == 1 and calls.count("decoder.3") == 1 and calls.count("decoder.0") == 1
    assert calls.count("decoder.1.pointwise_bn") == 1 and "decoder.1.pointwise_activate" not in calls
    torch.manual_seed(1)
    want_out, want_dec = head(feats)
    assert torch.equal(out, want_out) and torch.equal(dec, want_dec)
    assert bool((dec >= 0).all()) and not torch.equal(marked.decoder[3](dec), out)     # decoder_out is the tensor in front of the dropout


# ---------------------------------------------------------------- the operator and its entry points

def test_operator_on_cpu_is_the_stock_statements():
    from halo_amd import norm
    from euclid_head_standin import frozen
    bn = frozen(6, 5)
    x0, gy, gz = torch.randn(2, 6, 5, 7), torch.randn(2, 6, 5, 7), torch.randn(2, 6, 5, 7)
    for drop in (nn.Dropout2d(0.5), nn.Dropout2d(0.5).eval(), nn.Dropout2d(0.0), nn.Dropout2d(1.0)):
        assert norm.pair_fallback_reason(x0, bn, drop) is not None             # a CPU tensor, whatever the dropout
        res = []
        for fn in (norm.norm_relu_dropout2d_pair, norm.pair_statement):
            x = x0.clone().requires_grad_(True)
            torch.manual_seed(1)
            y, z = fn(x, bn, drop)
            state = torch.get_rng_state()
            assert (z is y) == (not drop.training or drop.p == 0)
            res.append((y.detach().clone(), z.detach().clone(), state, torch.autograd.grad([y, z], x, [gy, gz], retain_graph=True)[0],
                        torch.autograd.grad(z, x, gz, retain_graph=True)[0], torch.autograd.grad(y, x, gy)[0]))
            assert torch.equal(x.detach(), x0)
        assert all(torch.equal(a, b) for a, b in zip(*res))
    assert "nn.Dropout2d" in norm.pair_fallback_reason(x0, bn, nn.Dropout(0.5))
    assert "in place" in norm.pair_fallback_reason(x0, bn, nn.Dropout2d(0.5, inplace=True))
    assert "p = 1" in norm.pair_fallback_reason(x0, bn, nn.Dropout2d(1.0))
    # the size rule is a constant of its own, not a key of the dict that other tests replace wholesale
    assert isinstance(norm.PAIR_AUTOGRAD_MIN_ELEMENTS, int) and set(norm.AUTOGRAD_MIN_ELEMENTS) == {"plain", "affine", "masked"}


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(halo_dropout_pair_\w+)\s*\(", code)) == set(SYMBOLS)
    assert not any(s.startswith(("halo_masked_", "halo_affine_relu")) for s in SYMBOLS)
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
        args = re.search(r"\b%s\s*\(([^)]*)\)" % s, code).group(1).split(",")
        assert len(args) == len(_lib.SIGNATURES[s][1]) == 10, s
        # six pointers, three 64-bit extents, the stream: the header's parameter types against the binding's, one by one
        want = [ctypes.c_void_p if "*" in a else ctypes.c_int64 for a in args]
        assert all("float *" in a for a in args[:6]) and all("int64_t" in a for a in args[6:9]) and "void *stream" in args[9]
        assert _lib.SIGNATURES[s][1] == want and _lib.SIGNATURES[s][0] is ctypes.c_int, s
    version = int(re.search(r"#define HALO_ABI_VERSION (\d+)", text).group(1))
    assert version == _lib.ABI_VERSION == 13 and _lib.lib().halo_version() == 13       # no exported signature changed


def test_argument_checks_refuse_before_any_launch():
    """every pointer is one HOST buffer: a check that went missing would end in a launch error or worse, never in these codes"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = L.halo_dropout_pair_fwd, L.halo_dropout_pair_bwd
    for k in range(6):                                                                   # each of the forward's six pointers
        args = [p] * 6
        args[k] = None
        assert fwd(*args, 1, 2, 16, None) == E_ARG
        msg = L.halo_last_error().decode()
        assert "null" in msg and "halo_dropout_pair_fwd" in msg, msg
    for k in range(2, 6):                                                                # y, scale, mask, g_x of the backward
        args = [p] * 6
        args[k] = None
        assert bwd(*args, 1, 2, 16, None) == E_ARG
        msg = L.halo_last_error().decode()
        assert "null" in msg and "halo_dropout_pair_bwd" in msg, msg
    assert bwd(None, None, p, p, p, p, 1, 2, 16, None) == E_ARG                          # one gradient may be absent, not both
    assert "neither" in L.halo_last_error().decode()
    for name, fn in (("halo_dropout_pair_fwd", fwd), ("halo_dropout_pair_bwd", bwd)):
        for shape in ((0, 2, 16), (1, 0, 16), (1, 2, 0)):
            assert fn(p, p, p, p, p, p, *shape, None) == E_ARG and "empty" in L.halo_last_error().decode()
        assert fn(p, p, p, p, p, p, 1, 2, 1 << 31, None) == E_UNSUPPORTED                # an_plan's limits: offsets inside a plane
        assert fn(p, p, p, p, p, p, 1 << 20, 1 << 20, 4096, None) == E_UNSUPPORTED       # more workgroups than a grid holds
        assert name in L.halo_last_error().decode()
    for one in ((None, p), (p, None)):                                                   # an absent gradient passes the pointer check
        assert bwd(*one, p, p, p, p, 0, 2, 16, None) == E_ARG and "empty" in L.halo_last_error().decode()
