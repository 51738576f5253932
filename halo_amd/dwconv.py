"""The depthwise half of a DepthwiseSeparableConv2d block (core/models/classifier.py:78-81) on the device.

Every shipped config trains deeplabv3plus_resnet101 with MODEL.FREEZE_BN, so the five DepthwiseSeparableConv2d blocks of the
v3+ head run

    x = self.depthwise_conv(x)      # 3x3, groups = C, dilation d, padding d, bias=False
    x = self.depthwise_bn(x)        # FrozenBatchNorm2d: x * scale + bias
    x = self.depthwise_activate(x)  # ReLU(inplace=True)

as four bandwidth-bound passes over a 200 MB tensor.  `depthwise_bn_relu(x, conv, bn)` computes the three statements and the
gradients for x and conv.weight with halo_dwconv.hip: one read and one write forward; the backward keeps x and y only, writes
every g_x element once (a gather with the mirrored taps) and sums g_w in float64 in a fixed order, without atomics.

The norm is (a) a frozen norm -- a module whose type is named FrozenBatchNorm2d with the buffers weight, bias, running_mean,
running_var (core/models/layers.py); scale and shift come from its own two statements, `weight * running_var.rsqrt()` and
`bias - running_mean * scale`, run as torch ops on the device (no eps, as there) -- or (b) nn.BatchNorm2d / nn.SyncBatchNorm in
eval mode with running statistics whose parameters need no gradient: scale = weight / sqrt(running_var + eps).

Anything outside the served envelope (fallback_reason) runs the three stock module calls (torch_statement), so torch's results
and errors are kept there: batch statistics, a conv bias, other kernel sizes / strides / padding, other dtypes, autocast, CPU
tensors.
"""
import torch
import torch.nn as nn

from . import _lib
from .hfr import _autocast


def torch_statement(x, conv, bn, act=None):
    """the three stock statements of the block's forward (classifier.py:79-81)"""
    x = conv(x)
    x = bn(x)
    return torch.relu(x) if act is None else act(x)


def _is_frozen(bn):
    if type(bn).__name__ != "FrozenBatchNorm2d" or not isinstance(bn, nn.Module):
        return False
    return all(torch.is_tensor(bn._buffers.get(n)) for n in ("weight", "bias", "running_mean", "running_var"))


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def fallback_reason(x, conv, bn):
    """why depthwise_bn_relu(x, conv, bn) runs the torch statements (None: the fused path serves it).  Reads no device memory."""
    if type(conv) is not nn.Conv2d:
        return "conv is not nn.Conv2d"
    C = conv.in_channels
    if conv.groups != C or conv.out_channels != C:
        return "conv is not depthwise (groups == in_channels == out_channels)"
    if _pair(conv.kernel_size) != (3, 3):
        return "kernel size %s, not (3, 3)" % (tuple(_pair(conv.kernel_size)),)
    if _pair(conv.stride) != (1, 1):
        return "stride %s, not 1" % (tuple(_pair(conv.stride)),)
    dil = _pair(conv.dilation)
    if isinstance(conv.padding, str) or dil[0] != dil[1] or dil[0] < 1 or _pair(conv.padding) != dil:
        return "dilation %s and padding %s are not one (d, d)" % (conv.dilation, conv.padding)
    if conv.padding_mode != "zeros":
        return "padding_mode %r" % conv.padding_mode
    if conv.bias is not None:
        return "conv has a bias"
    if _is_frozen(bn):
        tensors = [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        features = bn.weight.numel()
    elif type(bn) in (nn.BatchNorm2d, nn.SyncBatchNorm):
        if bn.training or bn.running_mean is None or bn.running_var is None:
            return "BatchNorm with batch statistics"
        if (bn.weight is None) != (bn.bias is None):
            return "BatchNorm with only one of weight and bias"
        if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in (bn.weight, bn.bias)):
            return "BatchNorm parameters require a gradient"
        tensors = [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        features = bn.num_features
    else:
        return "bn is neither a FrozenBatchNorm2d nor an eval-mode BatchNorm2d / SyncBatchNorm"
    if features != C:
        return "the norm has %d channels, the conv %d" % (features, C)
    if not torch.is_tensor(x) or x.dim() != 4:
        return "x is not a (B, C, H, W) tensor"
    if x.shape[1] != C:
        return "x has %d channels, the conv %d" % (x.shape[1], C)
    if x.dtype != torch.float32:
        return "x is %s, not float32" % x.dtype
    if _autocast():
        return "autocast is enabled"
    if not x.is_cuda:
        return "x is not on a ROCm device"
    for t in [conv.weight] + tensors:
        if t is not None and (t.dtype != torch.float32 or t.device != x.device):
            return "a conv / norm tensor is not float32 on %s" % x.device
    B, _, H, W = x.shape
    if B * C * H * W == 0:
        return "empty input"
    if max(H, W, dil[0]) > 1 << 24 or H * W > 2 ** 31 - 1:
        return "plane of %d x %d, dilation %d" % (H, W, dil[0])
    return None


def scale_shift(bn):
    """(scale, shift) of a served norm, as torch ops on its device"""
    with torch.no_grad():
        if _is_frozen(bn):
            scale = bn.weight * bn.running_var.rsqrt()                  # layers.py: FrozenBatchNorm2d.forward's two statements
            shift = bn.bias - bn.running_mean * scale
        else:
            scale = torch.rsqrt(bn.running_var + bn.eps)
            if bn.weight is not None:
                scale = bn.weight * scale
            shift = -bn.running_mean * scale
            if bn.bias is not None:
                shift = bn.bias + shift
    return scale.contiguous(), shift.contiguous()


class _DepthwiseBnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, scale, shift, d):
        B, C, H, W = x.shape
        L = _lib.lib()
        y = torch.empty_like(x)
        _lib.check(L.halo_dwconv3x3_affine_relu_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, C, H, W, d,
                                                    _lib.stream_ptr(x.device)), "halo_dwconv3x3_affine_relu_fwd")
        ctx.save_for_backward(x, y, w, scale)
        ctx.d = d
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, y, w, scale = ctx.saved_tensors
        B, C, H, W = x.shape
        d = ctx.d
        L = _lib.lib()
        st = _lib.stream_ptr(x.device)
        g = g.to(device=x.device, dtype=torch.float32).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(L.halo_dwconv3x3_affine_relu_bwd_data(_lib.ptr(g), _lib.ptr(y), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gx), B, C, H, W, d,
                                                             st), "halo_dwconv3x3_affine_relu_bwd_data")
        if ctx.needs_input_grad[1]:
            nws = L.halo_dwconv_workspace_bytes(B, C, H, W, d)
            ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=x.device)
            gw = torch.empty_like(w)
            _lib.check(L.halo_dwconv3x3_affine_relu_bwd_weight(_lib.ptr(g), _lib.ptr(y), _lib.ptr(x), _lib.ptr(scale), _lib.ptr(gw), B, C, H, W, d,
                                                               _lib.ptr(ws), ws.numel() * 8, st), "halo_dwconv3x3_affine_relu_bwd_weight")
        return gx, gw, None, None, None


def depthwise_bn_relu(x, conv, bn, act=None):
    """relu(bn(conv(x))) of a depthwise 3x3 conv and a frozen / eval-mode norm, x (B, C, H, W).  Differentiable w.r.t. x and
    conv.weight.  Outside the served envelope (fallback_reason) it returns torch_statement(x, conv, bn, act)."""
    if fallback_reason(x, conv, bn) is not None:
        return torch_statement(x, conv, bn, act)
    scale, shift = scale_shift(bn)
    return _DepthwiseBnReluFn.apply(x.contiguous(), conv.weight.contiguous(), scale, shift, int(_pair(conv.dilation)[0]))


__all__ = ["depthwise_bn_relu", "torch_statement", "fallback_reason", "scale_shift"]
