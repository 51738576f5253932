"""The ASPP fan-out: the backbone's output `top` has five readers in the v3+ heads -- the dilated separable blocks that
halo_amd.dwconv.multi_depthwise_bn_relu serves, a 1 x 1 conv and the image-pooling branch -- and every reader sends a gradient of
top's size back, which the autograd engine adds with full-size passes of its own.

`fan_depthwise_bn_relu(x, blocks, readers)` returns (ys, xs): ys is multi_depthwise_bn_relu(x, blocks), with its bits; xs are
`readers` tensors that alias x (same values, same storage: write in place to none of them), one for each further reader of x.  All
come from one autograd node, whose backward makes one launch of halo_fan_dwconv3x3_affine_relu_bwd_data (halo_dwconv.hip):

    g_x = ((((gx_0 + gx_1) + gx_2) + e_0) + e_1) ...      float32 adds in list order, what did not arrive left out

gx_i the blocks' shares, e_j the gradient that arrived at xs[j].  The e_j join where the blocks' sum leaves LDS for memory.  A
gradient whose strides over H and W are 0 (what `plane_mean` sends back: one value per plane, never materialised) travels as its
(B, C) values; any other gradient travels dense.  g_w_i are multi_depthwise_bn_relu's calls.  When only extras arrive there is no
launch: they are added with torch.

`plane_mean(x)` is x.mean((-1, -2), keepdim=True) -- ATen's own statement for nn.AdaptiveAvgPool2d((1, 1)), so its bits -- with the
backward (g / (H W)).expand(x.shape): the stock gradient's values, bit for bit, without MeanBackward1's full-size write.

Outside the envelope (`fan_fallback_reason`) the operator returns multi_depthwise_bn_relu(x, blocks) and x itself `readers` times.
When a gradient will be asked for x, the aliases there come from a node of torch adds that joins the gradients in the contract's
order, so g_x keeps the association above on every path (the engine alone adds in arrival order: the readers made last first).
"""
import ctypes

import torch

from . import _lib
from .dwconv import multi_depthwise_bn_relu, multi_fallback_reason, multi_forward, multi_operands, multi_weight_grads

launches = {"fan_bwd": 0}                      # launches of halo_fan_dwconv3x3_affine_relu_bwd_data (the forward counts as dwconv's multi_fwd)
FAN_MIN, FAN_MAX = 1, 4                        # DWM_MAX_FAN of halo_dwconv.hip


def fan_fallback_reason(x, blocks, readers):
    """why fan_depthwise_bn_relu(x, blocks, readers) runs the composition (None: the fused passes serve it): multi_fallback_reason's
    envelope, 1 <= readers <= 4, and a gradient that will be asked for x.  Reads no device memory."""
    if not isinstance(readers, int) or isinstance(readers, bool) or not FAN_MIN <= readers <= FAN_MAX:
        return "%r further readers, %d to %d are served" % (readers, FAN_MIN, FAN_MAX)
    why = multi_fallback_reason(x, blocks)
    if why is not None:
        return why
    if not (torch.is_grad_enabled() and x.requires_grad):
        return "no gradient will be asked for x: there is nothing to join"
    return None


def is_per_plane(g):
    """whether a (B, C, H, W) gradient holds one value per plane without storing it H W times: strides 0 over H and W (over those of
    the two that are longer than 1: a stride says nothing about an axis of one element)"""
    return g.dim() == 4 and all(g.size(k) == 1 or g.stride(k) == 0 for k in (2, 3))


def joined(total, extras):
    """((total + e_0) + e_1) ... in torch float32 adds, None left out; total may be None"""
    for e in extras:
        if e is not None:
            total = e if total is None else total + e
    return total


def fan_bwd_data(gs, y, w, scale, dil, extras):
    """g_x of one halo_fan_dwconv3x3_affine_relu_bwd_data launch.  gs: the n gradients of y (n, B, C, H, W), contiguous float32 or
    None, at least one not None; extras: up to four (B, C, H, W) gradients or None, in the order they are added."""
    n, B, C, H, W = y.shape
    m = len(extras)
    keep, ptrs, flags = [], [], []
    for e in extras:
        if e is None:
            ptrs.append(None), flags.append(0)
            continue
        e = e.to(device=y.device, dtype=torch.float32)
        plane = is_per_plane(e)
        e = e[:, :, 0, 0].contiguous() if plane else e.contiguous()
        keep.append(e), ptrs.append(e.data_ptr()), flags.append(int(plane))
    gx = torch.empty((B, C, H, W), dtype=torch.float32, device=y.device)
    _lib.check(_lib.lib().halo_fan_dwconv3x3_affine_relu_bwd_data(
        (ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in gs]), _lib.ptr(y), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gx),
        B, C, H, W, n, (ctypes.c_int64 * n)(*dil), m, (ctypes.c_void_p * max(m, 1))(*ptrs), (ctypes.c_int32 * max(m, 1))(*flags),
        _lib.stream_ptr(y.device)), "halo_fan_dwconv3x3_affine_relu_bwd_data")
    launches["fan_bwd"] += 1
    return gx


class _FanDepthwiseBnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift, dil, readers, *ws):
        w, y = multi_forward(x, scale, shift, dil, ws)
        ctx.save_for_backward(x, y, w, scale)
        ctx.dil, ctx.n = dil, len(ws)
        ctx.set_materialize_grads(False)
        return tuple(y.unbind(0)) + tuple(x.view_as(x) for _ in range(readers))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        x, y, w, scale = ctx.saved_tensors
        n, dil = ctx.n, ctx.dil
        gs = [None if g is None else g.to(device=x.device, dtype=torch.float32).contiguous() for g in grads[:n]]
        extras = list(grads[n:])
        gx = None
        if ctx.needs_input_grad[0]:
            if all(g is None for g in gs):
                gx = joined(None, extras)                                  # no block's gradient arrived: nothing to launch, torch adds in list order
            else:
                gx = fan_bwd_data(gs, y, w, scale, dil, extras)
        return (gx, None, None, None, None) + tuple(multi_weight_grads(gs, x, y, scale, dil, ctx.needs_input_grad[5:]))


class _JoinFn(torch.autograd.Function):
    """x -> 1 + readers aliases of x; the backward adds the gradient of the first and then the others', in list order (torch adds)"""

    @staticmethod
    def forward(ctx, x, readers):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(1 + readers))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, first, *extras):
        return joined(first, extras), None


def fan_depthwise_bn_relu(x, blocks, readers):
    """(ys, xs): ys = multi_depthwise_bn_relu(x, blocks), its bits; xs = `readers` aliases of x for x's further readers (write in place
    to none).  One autograd node; its backward adds the blocks' input gradients and the gradients that arrived at xs, in that order,
    in one HIP pass (see the module's text).  Outside the envelope (fan_fallback_reason) it returns the composition."""
    blocks = [tuple(b) for b in blocks]
    if fan_fallback_reason(x, blocks, readers) is not None:
        if not (torch.is_tensor(x) and torch.is_grad_enabled() and x.requires_grad):
            return tuple(multi_depthwise_bn_relu(x, blocks)), (x,) * readers
        first, *xs = _JoinFn.apply(x, readers)
        return tuple(multi_depthwise_bn_relu(first, blocks)), tuple(xs)
    x, scale, shift, dil, ws = multi_operands(x, blocks)
    out = _FanDepthwiseBnReluFn.apply(x, scale, shift, dil, readers, *ws)
    return tuple(out[:len(blocks)]), tuple(out[len(blocks):])


class _PlaneMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = x.shape
        return x.mean((-1, -2), keepdim=True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return (g / (ctx.shape[-1] * ctx.shape[-2])).expand(ctx.shape)


def plane_mean(x):
    """x.mean((-1, -2), keepdim=True) for x (B, C, H, W): nn.AdaptiveAvgPool2d((1, 1))'s value and gradient, bit for bit; the
    gradient is the expanded (B, C, 1, 1) quotient, strides 0 over H and W, never stored at x's size"""
    return _PlaneMeanFn.apply(x)


__all__ = ["fan_depthwise_bn_relu", "fan_fallback_reason", "fan_bwd_data", "plane_mean", "is_per_plane", "joined", "launches"]
