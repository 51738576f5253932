"""CPU checks of the folded image-pooling branch (halo_pool_fold_* of halo_norm.hip, halo_amd.aspp.pooled_bottleneck,
halo_amd.hooks.use_folded_image_pooling): the entry points are declared, listed and exported under ABI 13, the argument checks
refuse before any launch, every clause of the envelope, the identity the operator rests on in float64, and the hook."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT
import dwconv_ref as R

SYMBOLS = ("halo_pool_fold_workspace_bytes", "halo_pool_fold_table", "halo_pool_fold_affine_relu_fwd", "halo_pool_fold_affine_relu_bwd")
E_ARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
U64 = 2.0 ** -53


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(halo_pool_fold_\w+)\s*\(", code)) == set(SYMBOLS)
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
    version = int(re.search(r"#define HALO_ABI_VERSION (\d+)", text).group(1))
    assert version == _lib.ABI_VERSION == 13 and _lib.lib().halo_version() == 13
    # the argument counts of the four declarations, read off the header, against the binding's
    for s in SYMBOLS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % s, code).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[s][1]), s
    assert [len(_lib.SIGNATURES[s][1]) for s in SYMBOLS] == [4, 9, 10, 12]
    assert _lib.SIGNATURES[SYMBOLS[0]][0] is ctypes.c_size_t and all(_lib.SIGNATURES[s][0] is ctypes.c_int for s in SYMBOLS[1:])


def test_argument_checks_refuse_before_any_launch():
    """every pointer is one HOST buffer: a check that went missing would end in a launch error or worse, never in these codes"""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nbytes, table, fwd, bwd = (getattr(L, s) for s in SYMBOLS)

    def refused(rc, code, word):
        msg = L.halo_last_error().decode()
        assert rc == code and word in msg and "halo_pool_fold_" in msg, (rc, msg)

    refused(table(None, p, p, 1, 2, 3, 4, 63, None), E_ARG, "null")                    # no weight
    refused(table(p, None, p, 1, 2, 3, 4, 63, None), E_ARG, "null")                    # no v
    refused(table(p, p, None, 1, 2, 3, 4, 63, None), E_ARG, "null")                    # no T
    refused(table(p, p, p, 0, 2, 3, 4, 63, None), E_ARG, "empty")
    refused(table(p, p, p, 1, 0, 3, 4, 63, None), E_ARG, "empty")
    refused(table(p, p, p, 1, 2, 0, 4, 63, None), E_ARG, "empty")                      # Cg = 0
    refused(table(p, p, p, 1, 2, 3, 4, 62, None), E_ARG, "do not fit")                 # the row is shorter than (c_off + Cg) 9
    refused(table(p, p, p, 1, 2, 3, -1, 63, None), E_ARG, "do not fit")
    for k in range(5):                                                                  # each pointer of the forward
        args = [p] * 5
        args[k] = None
        refused(fwd(*args, 1, 2, 3, 4, None), E_ARG, "null")
    refused(fwd(p, p, p, p, p, 0, 2, 3, 4, None), E_ARG, "empty")
    refused(fwd(p, p, p, p, p, 1, 0, 3, 4, None), E_ARG, "empty")
    refused(fwd(p, p, p, p, p, 1, 2, 0, 4, None), E_ARG, "empty")
    refused(fwd(p, p, p, p, p, 1, 2, 1, 4, None), E_ARG, "border")                     # H < 2
    refused(fwd(p, p, p, p, p, 1, 2, 3, 1, None), E_ARG, "border")                     # W < 2
    refused(fwd(p, p, p, p, p, 1, 2, 1 << 16, 1 << 16, None), E_UNSUPPORTED, "planes")
    n = nbytes(1, 2, 3, 4)
    assert n >= 2 * 9 * 8 and nbytes(1, 2, 1, 4) == 0 and nbytes(0, 2, 3, 4) == 0 and nbytes(1, 2, 3, 1) == 0
    assert nbytes(2, 512, 80, 160) >= 2 * 512 * 4 * 72                                 # a row per workgroup of either route
    # what a launch would refuse gives 0, and no product of unbounded factors is formed on the way
    assert nbytes(1, 2, 1 << 40, 1 << 40) == 0 and nbytes(1, 2, 1 << 62, 4) == 0 and nbytes(1, 2, 1 << 16, 1 << 16) == 0
    assert nbytes(1 << 40, 1 << 40, 3, 4) == 0 and nbytes(1 << 31, 2, 3, 4) == 0 and nbytes(1 << 20, 1 << 20, 3, 4) == 0
    assert nbytes(1 << 15, 1 << 15, 1 << 10, 1 << 10) == 0                             # 2^30 planes x 2^10 rows: more than a grid
    assert nbytes(1 << 15, 1 << 15, 3, 4) == (1 << 30) * 72
    refused(bwd(None, p, p, p, p, 1, 2, 3, 4, p, n, None), E_ARG, "null")              # no g
    refused(bwd(p, None, p, p, p, 1, 2, 3, 4, p, n, None), E_ARG, "null")              # no y
    refused(bwd(p, p, None, p, p, 1, 2, 3, 4, p, n, None), E_ARG, "null")              # no scale
    refused(bwd(p, p, p, p, p, 1, 2, 1, 4, p, n, None), E_ARG, "border")
    refused(bwd(p, p, p, p, p, 1, 2, 3, 1, p, n, None), E_ARG, "border")
    refused(bwd(p, p, p, p, p, 0, 2, 3, 4, p, n, None), E_ARG, "empty")
    refused(bwd(p, p, p, p, p, 1, 2, 3, 4, p, 2 * 9 * 8 - 1, None), E_WORKSPACE, "workspace")     # short
    refused(bwd(p, p, p, p, p, 1, 2, 3, 4, None, n, None), E_WORKSPACE, "workspace")              # none
    assert bwd(p, p, p, None, None, 1, 2, 3, 4, None, 0, None) == 0                    # no gradient wanted: nothing is launched


class _OnDevice:
    """describes a float32 ROCm tensor without one: pool_fold_fallback_reason reads attributes only"""
    is_cuda, dtype, device, contiguous = True, torch.float32, torch.device("cpu"), True

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self.contiguous


def _modules(cin=5, cout=4, **kw):
    args = dict(kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=False)
    args.update(kw)
    return nn.Conv2d(cin, cout, **args), R.FrozenBatchNorm2d(cout)


def test_envelope_decisions(monkeypatch):
    from halo_amd import aspp
    why = aspp.pool_fold_fallback_reason
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    p, v = _OnDevice(2, 3, 4, 6), _OnDevice(2, 2, 1, 1)
    conv, bn = _modules()
    assert why(p, v, conv, bn) is None and why(p, v, conv, bn, nn.ReLU()) is None and why(p, v, conv, bn, nn.ReLU(inplace=True)) is None
    assert why(_OnDevice(2, 3, 2, 2), v, conv, bn) is None                                  # the smallest map
    assert "(B, Cx, H, W)" in why(_OnDevice(3, 4, 6), v, conv, bn)
    assert "(B, Cx, H, W)" in why(None, v, conv, bn)
    double = _OnDevice(2, 3, 4, 6)
    double.dtype = torch.float64
    assert "float32" in why(double, v, conv, bn)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert "autocast" in why(p, v, conv, bn)
    strided = _OnDevice(2, 3, 4, 6)
    strided.contiguous = False
    assert "contiguous" in why(strided, v, conv, bn)
    assert "empty" in why(_OnDevice(0, 3, 4, 6), _OnDevice(0, 2, 1, 1), conv, bn)
    assert "border" in why(_OnDevice(2, 3, 1, 6), v, conv, bn)                              # H < 2
    assert "border" in why(_OnDevice(2, 3, 4, 1), v, conv, bn)                              # W < 2
    assert "plane" in why(_OnDevice(2, 3, 1 << 16, 1 << 16), v, conv, bn)
    for bad in (_OnDevice(2, 2, 4, 6), _OnDevice(2, 2, 1, 2), _OnDevice(1, 2, 1, 1), _OnDevice(2, 2), _OnDevice(2, 0, 1, 1), None):
        assert "(B, Cg, 1, 1)" in why(p, bad, conv, bn)
    vd = _OnDevice(2, 2, 1, 1)
    vd.dtype = torch.float64
    assert "v is not" in why(p, vd, conv, bn)
    ve = _OnDevice(2, 2, 1, 1)
    ve.device = torch.device("meta")
    assert "v is not" in why(p, ve, conv, bn)
    assert "nn.Conv2d" in why(p, v, nn.ConvTranspose2d(5, 4, 3, padding=1, bias=False), bn)
    assert "dense 3x3" in why(p, v, _modules(kernel_size=1, padding=0)[0], bn)
    assert "dense 3x3" in why(p, v, _modules(stride=2)[0], bn)
    assert "dense 3x3" in why(p, v, _modules(dilation=2, padding=2)[0], bn)
    assert "dense 3x3" in why(_OnDevice(2, 4, 4, 6), v, _modules(cin=6, groups=2)[0], bn)
    assert "ring of zeros" in why(p, v, _modules(padding=0)[0], bn)
    assert "ring of zeros" in why(p, v, _modules(padding_mode="reflect")[0], bn)
    assert "bias" in why(p, v, _modules(bias=True)[0], bn)
    assert "channels" in why(p, v, _modules(cin=6)[0], bn)                                  # in_channels is not Cx + Cg
    assert "conv.weight" in why(p, v, _modules()[0].double(), bn)
    assert "FrozenBatchNorm2d" in why(p, v, conv, nn.BatchNorm2d(4).eval())                 # section 15's envelope: a frozen norm ...
    assert "shape" in why(p, v, conv, R.FrozenBatchNorm2d(5))                               # ... of the conv's output channels ...
    assert "float32" in why(p, v, conv, R.FrozenBatchNorm2d(4).double())                    # ... with float32 buffers
    assert "nn.ReLU" in why(p, v, conv, bn, nn.ReLU6()) and "nn.ReLU" in why(p, v, conv, bn, nn.LeakyReLU())
    monkeypatch.setattr(aspp, "EXCLUDED_SHAPES", {(2, 4, 6)})                               # the speed rule of the measurements
    assert "measured" in why(p, v, conv, bn) and why(_OnDevice(1, 3, 4, 6), _OnDevice(1, 2, 1, 1), conv, bn) is None
    monkeypatch.undo()
    assert "ROCm device" in why(torch.zeros(2, 3, 4, 6), torch.zeros(2, 2, 1, 1), conv, bn)  # CPU tensors


def _fold64(p, v, W, Cx):
    """the operator's statements in float64: the conv over the pyramid plus the class table"""
    from halo_amd.aspp import class_to_tap_matrix
    B, _, H, Wd = p.shape
    Co, Cg = W.shape[0], W.shape[1] - Cx
    S = torch.einsum("ock,bc->bok", W[:, Cx:].reshape(Co, Cg, 9), v.reshape(B, Cg))
    T = (S @ class_to_tap_matrix().T).reshape(B, Co, 3, 3)
    rc = torch.ones(H, dtype=torch.long)
    rc[0], rc[-1] = 0, 2
    cc = torch.ones(Wd, dtype=torch.long)
    cc[0], cc[-1] = 0, 2
    return F.conv2d(p, W[:, :Cx], padding=1) + T[:, :, rc][:, :, :, cc], (rc, cc)


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (5, 4)])
def test_identity_and_class_algebra_in_float64(H, W):
    """conv2d of the concatenation equals the conv over the pyramid plus the 9-class table, and the gradients of the pooled branch
    follow from the 9 class sums of the output gradient.  Both sides are float64 sums of the same 9 (Cx + Cg) products in different
    orders: they agree to a few 2^-53 of the sum of the products' magnitudes."""
    from halo_amd.aspp import class_to_tap_matrix
    torch.manual_seed(H * 10 + W)
    B, Cx, Cg, Co = 2, 3, 2, 4
    p = torch.randn(B, Cx, H, W, dtype=torch.float64)
    v = torch.randn(B, Cg, 1, 1, dtype=torch.float64, requires_grad=True)
    Wt = torch.randn(Co, Cx + Cg, 3, 3, dtype=torch.float64, requires_grad=True)
    x = torch.cat([p, v.expand(-1, -1, H, W)], 1)
    want = F.conv2d(x, Wt, padding=1)
    mag = F.conv2d(x.detach().abs(), Wt.detach().abs(), padding=1)
    got, (rc, cc) = _fold64(p, v.detach(), Wt.detach(), Cx)
    ratio = ((got - want.detach()).abs() / mag).max().item()
    print("identity at %d x %d: max |delta| / sum|W||x| = %.3g" % (H, W, ratio))
    assert ratio <= 8 * U64
    # the gradients of the pooled branch from the class sums of g
    g = torch.randn(B, Co, H, W, dtype=torch.float64)
    gv_want, gW_want = torch.autograd.grad(want, [v, Wt], g)
    cls = (rc[:, None] * 3 + cc[None, :]).reshape(-1)
    g_T = torch.zeros(B, Co, 9, dtype=torch.float64).index_add_(2, cls, g.reshape(B, Co, H * W))
    g_Ta = torch.zeros(B, Co, 9, dtype=torch.float64).index_add_(2, cls, g.abs().reshape(B, Co, H * W))
    M = class_to_tap_matrix()
    g_S, g_Sa = g_T @ M, g_Ta @ M
    Wg, vv = Wt.detach()[:, Cx:].reshape(Co, Cg, 9), v.detach().reshape(B, Cg)
    gv = torch.einsum("ock,bok->bc", Wg, g_S)
    gW = torch.einsum("bok,bc->ock", g_S, vv)
    gv_mag = torch.einsum("ock,bok->bc", Wg.abs(), g_Sa)
    gW_mag = torch.einsum("bok,bc->ock", g_Sa, vv.abs())
    assert ((gv - gv_want.reshape(B, Cg)).abs() / gv_mag).max().item() <= 8 * U64
    assert ((gW - gW_want[:, Cx:].reshape(Co, Cg, 9)).abs() / gW_mag).max().item() <= 8 * U64
    # every tap of every class is counted once: the classes of an all-ones plane sum to the tap counts of a padded 3x3 window
    assert (M.sum(1).reshape(3, 3) == torch.tensor([[4., 6., 4.], [6., 9., 6.], [4., 6., 4.]], dtype=torch.float64)).all()


def _frozen(n):
    bn = R.FrozenBatchNorm2d(n)
    bn.weight.copy_(0.5 + torch.rand(n)), bn.bias.copy_(0.2 * torch.randn(n)), bn.running_mean.copy_(0.3 * torch.randn(n))
    bn.running_var.copy_(0.5 + torch.rand(n))
    return bn


class _Stage(nn.Module):
    """the modules of a v3+ head that v3plus_decoder reads"""

    def __init__(self):
        super().__init__()
        self.bottleneck = nn.Sequential(nn.Conv2d(5, 4, 3, padding=1, bias=False), _frozen(4), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(3, 2, 1, bias=False), _frozen(2), nn.ReLU(inplace=True))
        self.decoder = nn.Sequential(nn.Conv2d(6, 4, 3, padding=1, bias=False), _frozen(4), nn.ReLU(inplace=True))


def test_hook_marks_only_classes_with_a_package_forward_and_cpu_tensors_run_the_stock_statements():
    from halo_amd import hooks
    from halo_amd.aspp import pooled_bottleneck
    from halo_amd.core.models.classifier import folded_pooling, v3plus_decoder, v3plus_hyper_forward
    from halo_amd.hooks import fused_v3plus_hyper_forward, use_folded_image_pooling

    class Plain(nn.Module):
        def forward(self, x):
            return x

    class Head(_Stage):
        forward = v3plus_hyper_forward

    class Reweighting(_Stage):
        forward = fused_v3plus_hyper_forward

    class Child(Head):
        pass

    class Unmarked(_Stage):
        forward = v3plus_hyper_forward

    for bad in (Plain, nn.Conv2d, Plain(), "Head"):
        with pytest.raises(TypeError):
            use_folded_image_pooling(bad)
    assert not hasattr(Head, "_halo_folded_image_pooling")
    assert use_folded_image_pooling(Head) is Head and use_folded_image_pooling(Head) is Head and Head._halo_folded_image_pooling is True
    assert use_folded_image_pooling(Reweighting) is Reweighting and use_folded_image_pooling(Child) is Child
    assert Head.forward is v3plus_hyper_forward and Reweighting.forward is fused_v3plus_hyper_forward      # the forwards stay bound
    assert not hasattr(Unmarked, "_halo_folded_image_pooling") and not hasattr(_Stage, "_halo_folded_image_pooling")
    assert "use_folded_image_pooling" not in open(hooks.__file__.replace("hooks.py", "_install.py")).read()   # install() does not bind it

    torch.manual_seed(3)
    with torch.no_grad():
        marked, plain = Head(), Unmarked()
    plain.load_state_dict(marked.state_dict())
    keys = list(marked.state_dict())
    pyramid = [torch.randn(2, 2, 4, 6), torch.randn(2, 1, 4, 6)]
    pooled, low = torch.randn(2, 2, 1, 1), torch.randn(2, 3, 8, 12)
    assert folded_pooling(marked, pooled) and not folded_pooling(plain, pooled) and not folded_pooling(marked, torch.randn(2, 2, 2, 2))
    with torch.no_grad():
        # today's statements, written out
        wide = F.interpolate(pooled, size=(4, 6), mode="bilinear", align_corners=True)
        fused = plain.bottleneck(torch.cat(pyramid + [wide], dim=1))
        fused = F.interpolate(fused, size=low.shape[2:], mode="bilinear", align_corners=True)
        want = plain.decoder(torch.cat([fused, plain.shortcut(low)], dim=1))
        assert torch.equal(v3plus_decoder(plain, pyramid + [wide], low, None), want)
        # CPU tensors are outside the envelope: a marked head runs the same statements, and so does the operator
        assert torch.equal(v3plus_decoder(marked, list(pyramid), low, None, pooled=pooled), want)
        y = pooled_bottleneck(torch.cat(pyramid, 1), pooled, *marked.bottleneck)
        assert torch.equal(y, plain.bottleneck(torch.cat(pyramid + [wide], dim=1)))
    assert list(marked.state_dict()) == keys


def test_a_strided_or_expanded_pooled_map_and_a_replaced_weight():
    """v need not be dense: the envelope accepts a channel slice and a batch-expanded row, and the operator reads a dense copy
    (fold_table and the autograd function both make one).  On the CPU that is the stock statement either way.  The cached weight
    slice follows an assignment to `.data`, which moves neither the parameter object nor its version."""
    from halo_amd import aspp
    torch.manual_seed(7)
    conv, bn = _modules()
    p = torch.randn(2, 3, 4, 6)
    wide = torch.randn(2, 5, 1, 1)
    for v in (wide[:, 1:3], torch.randn(1, 2, 1, 1).expand(2, -1, -1, -1)):
        assert not v.is_contiguous()
        why = aspp.pool_fold_fallback_reason(p, v, conv, bn)
        assert why is not None and "ROCm device" in why                                   # the CPU, nothing about v
        with torch.no_grad():
            assert torch.equal(aspp.pooled_bottleneck(p, v, conv, bn), aspp.torch_statement(p, v.contiguous(), conv, bn))
    with torch.no_grad():
        first = aspp.main_weight(conv, 3)
        assert aspp.main_weight(conv, 3) is first and torch.equal(first, conv.weight[:, :3])
        version = conv.weight._version
        conv.weight.data = torch.randn_like(conv.weight)
        assert conv.weight._version == version                                            # torch does not version this write ...
        second = aspp.main_weight(conv, 3)
        assert second is not first and torch.equal(second, conv.weight[:, :3])            # ... the address in the key sees it
        assert aspp.main_weight(conv, 2) is not second and aspp.main_weight(conv, 2).shape[1] == 2
        aspp.forget(conv)
        assert aspp.main_weight(conv, 3) is not second
