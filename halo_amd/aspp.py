"""The image-pooling branch of the v3+ heads folded into the bottleneck's epilogue (core/models/classifier.py:515-520).

The heads concatenate four parallel branches (Cx channels) with the pooled branch (Cg channels), one value per (image, channel)
broadcast over the map, and run `bottleneck = Sequential(Conv2d 3x3 zero-padded, FrozenBatchNorm2d, ReLU)` over the result.  A
3x3 zero-padded conv over a constant plane takes 9 values per (image, output channel) -- 3 row classes (top row, interior, bottom
row) x 3 column classes, by which taps fall inside the map -- so with Wm = weight[:, :Cx], Wg = weight[:, Cx:]

    S[b,o,ky,kx] = sum_c Wg[o,c,ky,kx] v[b,c]                                  float64
    T[b,o,rc,cc] = fl32(sum_{ky in R(rc)} sum_{kx in C(cc)} S[b,o,ky,kx])      R(top) = {1,2}, R(interior) = {0,1,2}, R(bottom) = {0,1}
    z            = conv2d(p, Wm, padding=1)                                    the library's conv over Cx channels
    y            = relu(fl(fl(fl(z + T[b,o,rc(i),cc(j)]) scale[o]) + shift[o]))

`pooled_bottleneck(p, v, conv, bn)` computes that with halo_norm.hip's halo_pool_fold_* kernels: the broadcast, the Cg channels of
the concatenation and a fifth of the conv's multiply-adds, forward and backward, are never made.  In the backward the device pass
reads g and y once and writes g_z = fl([y > 0] g scale) and the 9 class sums g_T of g_z per plane in float64 (a fixed order, no
atomics); the class algebra and the two small contractions

    g_S[b,o,ky,kx] = sum of g_T over the classes whose tap set holds (ky,kx)
    g_v[b,c] = sum_{o,k} Wg[o,c,k] g_S[b,o,k];      g_Wg[o,c,k] = sum_b g_S[b,o,k] v[b,c]

are float64 torch ops on the device, rounded once; g_z goes back through the conv's own autograd.  Saved for the backward: y, v,
scale, the weight parameter itself and what the conv saves -- nothing of the broadcast's or the (B, Cx + Cg, H, W) size.

The result is not the stock chain's bits (the Cg channels' share is summed in float64 and rounded once; the conv sums Cx instead
of Cx + Cg channels); it lies at the same distance from the exact value.  Outside the envelope (pool_fold_fallback_reason) the
stock statements run: broadcast, cat, conv, norm, activation.
"""
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .hfr import _autocast
from .norm import _norm_reason, cached_scale_shift

launches = {"table": 0, "fwd": 0, "bwd": 0}    # device passes issued by this module (tests count them)
_slices = weakref.WeakKeyDictionary()          # conv module -> (weight object, (version, address, device, Cx), weight[:, :Cx] contiguous)
# Shapes (B, H, W) at which the timing tool measured the folded stage no faster than the stock statements by more than the stock
# side's own window spread: they run the stock statements.  A speed rule alone: either side is a correct result.
EXCLUDED_SHAPES = set()


def torch_statement(p, v, conv, bn, act=None):
    """the stock statements: broadcast of the pooled map (what F.interpolate(align_corners=True) returns for a 1 x 1 map), cat,
    conv, norm, activation"""
    x = torch.cat([p, v.expand(-1, -1, p.shape[2], p.shape[3])], dim=1)
    out = bn(conv(x))
    return F.relu(out, inplace=True) if act is None else act(out)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def pool_fold_fallback_reason(p, v, conv, bn, act=None):
    """why pooled_bottleneck(p, v, conv, bn, act) runs the stock statements (None: the folded path serves it).  Reads no device
    memory."""
    if not torch.is_tensor(p) or p.dim() != 4:
        return "p is not a (B, Cx, H, W) tensor"
    if p.dtype != torch.float32:
        return "p is %s, not float32" % p.dtype
    if _autocast():
        return "autocast is enabled"
    if not p.is_cuda:
        return "p is not on a ROCm device"
    if not p.is_contiguous():
        return "p is not contiguous NCHW"
    B, Cx, H, W = p.shape
    if B == 0 or Cx == 0:
        return "empty input"
    if H < 2 or W < 2:
        return "a %d x %d map has no separate border classes" % (H, W)
    if H * W > 2 ** 31 - 1025:
        return "plane of %d x %d" % (H, W)
    if not torch.is_tensor(v) or v.dim() != 4 or v.shape[0] != B or tuple(v.shape[2:]) != (1, 1) or v.shape[1] == 0:
        return "v is not a (B, Cg, 1, 1) tensor"
    if v.dtype != p.dtype or v.device != p.device:
        return "v is not %s on %s" % (p.dtype, p.device)
    Cg = v.shape[1]
    if type(conv) is not nn.Conv2d:
        return "conv is not nn.Conv2d"
    if _pair(conv.kernel_size) != (3, 3) or _pair(conv.stride) != (1, 1) or _pair(conv.dilation) != (1, 1) or conv.groups != 1:
        return "conv is not a dense 3x3 at stride 1 and dilation 1"
    if _pair(conv.padding) != (1, 1) or conv.padding_mode != "zeros":
        return "conv does not pad one ring of zeros"
    if conv.bias is not None:
        return "conv has a bias"
    if conv.in_channels != Cx + Cg:
        return "conv reads %d channels, p and v bring %d + %d" % (conv.in_channels, Cx, Cg)
    w = conv.weight
    if w.dtype != torch.float32 or w.device != p.device or not w.is_contiguous():
        return "conv.weight is not contiguous float32 on %s" % p.device
    r = _norm_reason(bn, conv.out_channels, p.device, "bn")
    if r is not None:
        return r
    if act is not None and type(act) is not nn.ReLU:
        return "the activation is not nn.ReLU"
    if (B, H, W) in EXCLUDED_SHAPES:
        return "%d images of %d x %d: measured no faster than the stock statements" % (B, H, W)
    return None


def main_weight(conv, Cx):
    """weight[:, :Cx] for the conv over the pyramid.  Under no_grad (or a weight that needs no gradient) the contiguous slice of the
    previous call, kept while the weight is the same object at the same version, address and device -- `conv.weight.data = other`
    and `module.to(device)` move neither the object nor its version, but they move the address; under autograd the view, whose
    gradient flows back into the parameter.  The one write this does not see is one through a detached alias
    (`conv.weight.data.mul_()`): call forget(conv) after it."""
    w = conv.weight
    if torch.is_grad_enabled() and w.requires_grad:
        return w[:, :Cx]
    try:
        version = w._version
    except RuntimeError:                       # an inference tensor carries no version counter: nothing to key on
        _slices.pop(conv, None)
        return w.detach()[:, :Cx].contiguous()
    key = (version, w.data_ptr(), w.device, Cx)
    hit = _slices.get(conv)
    if hit is not None and hit[0] is w and hit[1] == key:
        return hit[2]
    part = w.detach()[:, :Cx].contiguous()
    _slices[conv] = (w, key, part)
    return part


def forget(conv=None):
    """drop the cached weight slice of one conv, or of all (after an in-place write through a detached alias such as
    `conv.weight.data.mul_()`, which torch does not version and which leaves the address where it was)"""
    if conv is None:
        _slices.clear()
    else:
        _slices.pop(conv, None)


def fold_table(weight, v, Cx):
    """T (B, Co, 3, 3) float32 from the (Co, Cx + Cg, 3, 3) weight, read in place from channel Cx on, and v (B, Cg, 1, 1)"""
    B, Cg = v.shape[0], v.shape[1]
    Co = weight.shape[0]
    v = v.contiguous()                                         # a slice or an expanded view is not the dense (B, Cg) block the pass reads
    if not weight.is_contiguous():
        raise ValueError("fold_table: the (Co, Cx + Cg, 3, 3) weight must be contiguous")
    T = torch.empty((B, Co, 3, 3), device=v.device, dtype=torch.float32)
    launches["table"] += 1
    _lib.check(_lib.lib().halo_pool_fold_table(_lib.ptr(weight), _lib.ptr(v), _lib.ptr(T), B, Co, Cg, Cx, weight.stride(0),
                                               _lib.stream_ptr(v.device)), "halo_pool_fold_table")
    return T


def fold_forward(z, T, scale, shift):
    """y = relu(((z + T[class]) * scale) + shift) for z (B, Co, H, W) contiguous"""
    B, Co, H, W = z.shape
    y = torch.empty((B, Co, H, W), device=z.device, dtype=torch.float32)
    launches["fwd"] += 1
    _lib.check(_lib.lib().halo_pool_fold_affine_relu_fwd(_lib.ptr(z), _lib.ptr(T), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, Co, H, W,
                                                         _lib.stream_ptr(z.device)), "halo_pool_fold_affine_relu_fwd")
    return y


def fold_backward(g, y, scale, want_z=True, want_T=True):
    """(g_z float32 or None, g_T (B, Co, 3, 3) float64 or None); nothing is launched when neither is wanted"""
    if not want_z and not want_T:
        return None, None
    B, Co, H, W = y.shape
    g_z = torch.empty_like(y) if want_z else None
    g_T = ws = None
    nbytes = 0
    if want_T:
        g_T = torch.empty((B, Co, 3, 3), device=y.device, dtype=torch.float64)
        nbytes = _lib.lib().halo_pool_fold_workspace_bytes(B, Co, H, W)
        ws = torch.empty(nbytes, device=y.device, dtype=torch.uint8)
    launches["bwd"] += 1
    _lib.check(_lib.lib().halo_pool_fold_affine_relu_bwd(_lib.ptr(g), _lib.ptr(y), _lib.ptr(scale), _lib.ptr(g_z), _lib.ptr(g_T), B, Co, H, W,
                                                         _lib.ptr(ws), nbytes, _lib.stream_ptr(y.device)), "halo_pool_fold_affine_relu_bwd")
    return g_z, g_T


def class_to_tap_matrix(device=None, dtype=torch.float64):
    """M (9 classes, 9 taps): 1 where the class's tap set R(rc) x C(cc) holds (ky, kx).  T = S M^T and g_S = g_T M."""
    taps = ((1, 2), (0, 1, 2), (0, 1))
    M = torch.zeros(9, 9, dtype=dtype)
    for rc in range(3):
        for cc in range(3):
            for ky in taps[rc]:
                for kx in taps[cc]:
                    M[rc * 3 + cc, ky * 3 + kx] = 1
    return M.to(device) if device is not None else M


class _PoolFoldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, v, weight, scale, shift, Cx):
        z, v = z.contiguous(), v.contiguous()                 # the kernels read dense blocks; v is B * Cg floats
        y = fold_forward(z, fold_table(weight, v, Cx), scale, shift)
        ctx.Cx = Cx
        ctx.save_for_backward(y, v, weight, scale)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y, v, weight, scale = ctx.saved_tensors
        Cx = ctx.Cx
        want_z, want_v, want_w = ctx.needs_input_grad[:3]
        g_v = g_w = None
        if want_z or want_v or want_w:
            g = g.to(device=y.device, dtype=torch.float32).contiguous()
        g_z, g_T = fold_backward(g, y, scale, want_z, want_v or want_w)
        if g_T is not None:
            B, Co = g_T.shape[:2]
            g_S = g_T.reshape(B, Co, 9) @ class_to_tap_matrix(y.device)                   # (B, Co, 9 taps), float64
            Cg = v.shape[1]
            if want_v:
                Wg = weight[:, Cx:].reshape(Co, Cg, 9).double()
                g_v = torch.einsum("ock,bok->bc", Wg, g_S).to(torch.float32).reshape(v.shape)
            if want_w:
                g_Wg = torch.einsum("bok,bc->ock", g_S, v.reshape(B, Cg).double())
                g_w = weight.new_zeros(weight.shape)
                g_w[:, Cx:] = g_Wg.reshape(Co, Cg, 3, 3)                                   # rounded once, by the copy
        return g_z, g_v, g_w, None, None, None


def pooled_bottleneck(p, v, conv, bn, act=None):
    """relu(bn(conv(cat([p, broadcast(v)], 1)))) for the pyramid p (B, Cx, H, W), the pooled branch's output v (B, Cg, 1, 1), a dense
    3x3 zero-padded conv of Cx + Cg input channels without bias and a FrozenBatchNorm2d: the conv runs over p alone, v's share enters
    the norm + ReLU pass as a 9-entry table per plane.  Differentiable once w.r.t. p, v and conv.weight.  Outside the envelope
    (pool_fold_fallback_reason) it returns torch_statement(p, v, conv, bn, act)."""
    if pool_fold_fallback_reason(p, v, conv, bn, act) is not None:
        return torch_statement(p, v, conv, bn, act)
    return fused_pooled_bottleneck(p, v, conv, bn)


def fused_pooled_bottleneck(p, v, conv, bn):
    """pooled_bottleneck for arguments that pool_fold_fallback_reason has accepted"""
    Cx = p.shape[1]
    z = F.conv2d(p, main_weight(conv, Cx), padding=1)
    scale, shift = cached_scale_shift(bn)
    return _PoolFoldFn.apply(z, v, conv.weight, scale, shift, Cx)


__all__ = ["pooled_bottleneck", "fused_pooled_bottleneck", "pool_fold_fallback_reason", "torch_statement", "main_weight", "forget", "fold_table", "fold_forward",
           "fold_backward", "class_to_tap_matrix"]
