"""Differentiable bilinear resize, align_corners=True, forward and backward on HIP kernels.

    y = bilinear_resize(x, size)          # x (..., h, w) float32 / float64 on the device; size = (H, W), H >= h, W >= w

The forward is halo_amd.core.utils.hyperbolic.bilinear_align_corners (halo_bilinear_upsample: ATen's CPU arithmetic bit for
bit); the backward is its adjoint as a gather (halo_bilinear_upsample_bwd, halo_resize.hip): no atomics, every gradient
element summed by one thread in a fixed order, so two backward passes over the same operands return identical bits -- which
ATen's device backward of F.interpolate (four float atomic adds per output element) does not promise.  Double backward is not
provided.  There is no CPU route and no fallback: inputs outside the served envelope raise before anything is allocated.

`resize_or_interpolate` is what the package's own training paths call under `halo_amd.hooks.use_device_resize`: the same
function where it serves the operands, F.interpolate where it does not (a training step must not raise over a dtype).
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

_DTYPES = (torch.float32, torch.float64)


def _refusal(x, size):
    """(exception class, message) when bilinear_resize does not serve (x, size), else None.  Touches no device memory."""
    if not torch.is_tensor(x):
        return TypeError, "halo_amd.resize: x must be a tensor, got %s" % type(x).__name__
    if x.dtype not in _DTYPES:
        return TypeError, "halo_amd.resize: x must be float32 or float64, got %s" % x.dtype
    if not x.is_cuda:
        return ValueError, "halo_amd.resize: x must be on a ROCm device (got %s); there is no CPU route" % x.device
    if x.dim() < 2:
        return ValueError, "halo_amd.resize: x must be (..., h, w), got %s" % (tuple(x.shape),)
    try:
        H, W = (int(s) for s in size)
    except (TypeError, ValueError):
        return ValueError, "halo_amd.resize: size must be (H, W), got %r" % (size,)
    h, w = x.shape[-2:]
    if h < 1 or w < 1:
        return ValueError, "halo_amd.resize: empty planes %s" % (tuple(x.shape),)
    if H < h or W < w:
        return ValueError, "halo_amd.resize: size %s is smaller than the input's %s; this operator upsamples only" % ((H, W), (h, w))
    return None


class _BilinearResizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W):
        from .core.utils.hyperbolic import bilinear_align_corners
        ctx.in_shape = tuple(x.shape)
        return bilinear_align_corners(x, (H, W))          # grad mode is off inside forward: the inference-only op accepts x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        shape = ctx.in_shape
        h, w = shape[-2:]
        H, W = g.shape[-2:]
        dev = _lib.require_device(g)
        g = g.contiguous()
        grad = torch.empty(shape, dtype=g.dtype, device=dev)
        if grad.numel():
            _lib.check(_lib.lib().halo_bilinear_upsample_bwd(_lib.ptr(g), _lib.ptr(grad), _lib.dtype_code(g), grad.numel() // (h * w), h, w,
                                                             H, W, _lib.stream_ptr(dev)), "halo_bilinear_upsample_bwd")
        return grad, None, None


def bilinear_resize(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) for float32 / float64 (..., h, w) on the device, upsampling
    only, differentiable once.  The values are bilinear_align_corners's; the gradient comes back in x's dtype and shape.
    TypeError: not a tensor, another dtype; ValueError: a CPU tensor, fewer than two dimensions, H < h or W < w."""
    bad = _refusal(x, size)
    if bad is not None:
        raise bad[0](bad[1])
    H, W = (int(s) for s in size)
    if torch.is_grad_enabled() and x.requires_grad:
        return _BilinearResizeFn.apply(x, H, W)
    from .core.utils.hyperbolic import bilinear_align_corners
    with torch.no_grad():
        return bilinear_align_corners(x, (H, W))


def resize_or_interpolate(x, size):
    """bilinear_resize where it serves (x, size), F.interpolate(mode='bilinear', align_corners=True) otherwise."""
    if _refusal(x, size) is None:
        return bilinear_resize(x, size)
    return F.interpolate(x, size=size, mode="bilinear", align_corners=True)


__all__ = ["bilinear_resize", "resize_or_interpolate"]
