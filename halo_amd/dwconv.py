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
tensors.  Under torch.autocast `depthwise_bn_relu_autocast(x, conv, bn)` serves the same block half with a float32 or half x and
the half output autocast would hand the pointwise conv (the section behind depthwise_bn_relu; halo_amd.hooks.use_autocast_depthwise).

The front of the v3+ decoder feeds such a block with `torch.cat([resize(a, s.shape[2:]), s], 1)`.
`upsample_cat_depthwise_bn_relu(a, s, conv, bn)` computes that block's depthwise half without storing the resized or the
concatenated tensor: the kernel reads its window from a (interpolated in place, halo_bilinear_upsample's bits) or from s, the
backward keeps a, s and y, recomputes the conv's input for the weight gradient and writes the data gradient as two dense tensors,
the first of which halo_bilinear_upsample_bwd turns into g_a.  Its results are those of depthwise_bn_relu over the stored
concatenation, bit for bit; outside its envelope (upcat_fallback_reason) it runs that composition.

The ASPP pyramid hands one tensor to three such blocks.  `multi_depthwise_bn_relu(x, blocks)` computes their depthwise halves in one
pass each way over a plane held in LDS, with the bits of one depthwise_bn_relu per block (the section at the end of this file).
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


def _module_reason(conv, bn):
    """(reason, the norm's tensors): the part of fallback_reason that looks at the modules alone"""
    if type(conv) is not nn.Conv2d:
        return "conv is not nn.Conv2d", None
    C = conv.in_channels
    if conv.groups != C or conv.out_channels != C:
        return "conv is not depthwise (groups == in_channels == out_channels)", None
    if _pair(conv.kernel_size) != (3, 3):
        return "kernel size %s, not (3, 3)" % (tuple(_pair(conv.kernel_size)),), None
    if _pair(conv.stride) != (1, 1):
        return "stride %s, not 1" % (tuple(_pair(conv.stride)),), None
    dil = _pair(conv.dilation)
    if isinstance(conv.padding, str) or dil[0] != dil[1] or dil[0] < 1 or _pair(conv.padding) != dil:
        return "dilation %s and padding %s are not one (d, d)" % (conv.dilation, conv.padding), None
    if conv.padding_mode != "zeros":
        return "padding_mode %r" % conv.padding_mode, None
    if conv.bias is not None:
        return "conv has a bias", None
    if _is_frozen(bn):
        tensors = [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        features = bn.weight.numel()
    elif type(bn) in (nn.BatchNorm2d, nn.SyncBatchNorm):
        if bn.training or bn.running_mean is None or bn.running_var is None:
            return "BatchNorm with batch statistics", None
        if (bn.weight is None) != (bn.bias is None):
            return "BatchNorm with only one of weight and bias", None
        if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in (bn.weight, bn.bias)):
            return "BatchNorm parameters require a gradient", None
        tensors = [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        features = bn.num_features
    else:
        return "bn is neither a FrozenBatchNorm2d nor an eval-mode BatchNorm2d / SyncBatchNorm", None
    if features != C:
        return "the norm has %d channels, the conv %d" % (features, C), None
    return None, tensors


def _operand_reason(shape, dtype, is_cuda, device, conv, tensors):
    """the part of fallback_reason that looks at the conv's input, given as its (B, C, H, W) shape, dtype and placement"""
    C, dil = conv.in_channels, _pair(conv.dilation)
    if shape[1] != C:
        return "x has %d channels, the conv %d" % (shape[1], C)
    if dtype != torch.float32:
        return "x is %s, not float32" % dtype
    if _autocast():
        return "autocast is enabled"
    if not is_cuda:
        return "x is not on a ROCm device"
    for t in [conv.weight] + tensors:
        if t is not None and (t.dtype != torch.float32 or t.device != device):
            return "a conv / norm tensor is not float32 on %s" % device
    B, _, H, W = shape
    if B * C * H * W == 0:
        return "empty input"
    if max(H, W, dil[0]) > 1 << 24 or H * W > 2 ** 31 - 1:
        return "plane of %d x %d, dilation %d" % (H, W, dil[0])
    return None


def fallback_reason(x, conv, bn):
    """why depthwise_bn_relu(x, conv, bn) runs the torch statements (None: the fused path serves it).  Reads no device memory."""
    why, tensors = _module_reason(conv, bn)
    if why is not None:
        return why
    if not torch.is_tensor(x) or x.dim() != 4:
        return "x is not a (B, C, H, W) tensor"
    return _operand_reason(tuple(x.shape), x.dtype, x.is_cuda, x.device, conv, tensors)


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
        if getattr(ctx, "joint", False) and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            nws = L.halo_dwconv_workspace_bytes(B, C, H, W, d)
            ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=x.device)
            gx, gw = torch.empty_like(x), torch.empty_like(w)
            _lib.check(L.halo_joint_dwconv3x3_affine_relu_bwd(_lib.ptr(g), _lib.ptr(y), _lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gx),
                                                              _lib.ptr(gw), B, C, H, W, d, _lib.ptr(ws), ws.numel() * 8, st),
                       "halo_joint_dwconv3x3_affine_relu_bwd")
            joint_launches["plain"] += 1
            return gx, gw, None, None, None
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


class _DepthwiseBnReluFnJoint(torch.autograd.Function):
    """the same node with ctx.joint set: its backward takes the joint entry when both gradients are wanted.  A sibling, not a
    subclass: it inherits nothing that a caller may have bound on _DepthwiseBnReluFn (tests wrap its `apply`)"""
    @staticmethod
    def forward(ctx, *args):
        ctx.joint = True
        return _DepthwiseBnReluFn.forward(ctx, *args)

    backward = staticmethod(_DepthwiseBnReluFn.backward)


# ---------------------------------------------------------------- both gradients from one backward pass (opt-in)
# With joint_backward=True a node whose differentiable inputs ALL need a gradient runs halo_joint_*_bwd: g, y and x are read once
# for g_x and g_w, with the bits of the two calls it replaces (include/halo_hip.h).  Any other combination of needs runs those two
# calls as before.  Counted per call of the joint entry:
joint_launches = {"plain": 0, "upcat": 0}
# A speed rule only (both sides return the same bits; the GPU tests switch it off with 0 everywhere).  Per route, the smallest
# B * C * H * W at which the joint pass won against the two calls in both processes of profiles/r25_time_joint_depthwise.txt;
# None: the route lost, or was not timed, and is not served.  Routes: "d1" and "dilated" are the 16-byte routes (W % 4 == 0) at
# d = 1 and d > 1, "column" is the one-column route (any other W), "upcat" the decoder front (W % 4 == 0; C = Ca + Cs).
#   d1       won at 1 and 2 x 512 x 160 x 320 (x1.39 / x1.41 and x1.24 / x1.22)
#   dilated  lost at every shape timed (2048 x 80 x 160 and 2048 x 90 x 160, d = 6, 12, 18, B = 1 and 2: x0.83 to x0.99)
#   column   not timed
#   upcat    won at 1 and 2 x (512 + 48) x 160 x 320 and x 180 x 320 (x1.05 to x1.18)
JOINT_MIN_ELEMENTS = {"d1": 1 * 512 * 160 * 320, "dilated": None, "column": None, "upcat": 1 * 560 * 160 * 320}


def _joint_rule_reason(route, elements):
    least = JOINT_MIN_ELEMENTS.get(route)
    if least is None:
        return "the joint backward's %r route is not served (a speed rule: it lost or was not timed)" % route
    if elements < least:
        return "%d elements, fewer than JOINT_MIN_ELEMENTS[%r] = %d (a speed rule: nothing smaller won)" % (elements, route, least)
    return None


def joint_fallback_reason(x, conv, bn):
    """why depthwise_bn_relu(x, conv, bn, joint_backward=True) runs its backward as two calls, or the torch statements (None: a
    backward that wants both gradients runs the joint entry).  The block's own fallback_reason, or the speed rule.  Reads no
    device memory."""
    why = fallback_reason(x, conv, bn)
    if why is not None:
        return why
    B, C, H, W = x.shape
    d = int(_pair(conv.dilation)[0])
    return _joint_rule_reason("column" if W % 4 else ("d1" if d == 1 else "dilated"), B * C * H * W)


def upcat_joint_fallback_reason(a, s, conv, bn):
    """joint_fallback_reason for upsample_cat_depthwise_bn_relu(a, s, conv, bn, joint_backward=True)"""
    why = upcat_fallback_reason(a, s, conv, bn)
    if why is not None:
        return why
    B, Cs, H, W = s.shape
    return _joint_rule_reason("column" if W % 4 else "upcat", B * (a.shape[1] + Cs) * H * W)


def depthwise_bn_relu(x, conv, bn, act=None, joint_backward=False):
    """relu(bn(conv(x))) of a depthwise 3x3 conv and a frozen / eval-mode norm, x (B, C, H, W).  Differentiable w.r.t. x and
    conv.weight.  Outside the served envelope (fallback_reason) it returns torch_statement(x, conv, bn, act).
    joint_backward=True: a backward that wants both gradients computes them in one pass (joint_fallback_reason; the same bits)."""
    if fallback_reason(x, conv, bn) is not None:
        return torch_statement(x, conv, bn, act)
    scale, shift = scale_shift(bn)
    fn = _DepthwiseBnReluFnJoint if joint_backward and joint_fallback_reason(x, conv, bn) is None else _DepthwiseBnReluFn
    return fn.apply(x.contiguous(), conv.weight.contiguous(), scale, shift, int(_pair(conv.dilation)[0]))


# ---------------------------------------------------------------- the block half under torch.autocast
# Under autocast the stock statements cast x and the conv's weight to half (float16 or bfloat16), the library's half conv returns
# half, the frozen norm promotes to float32, the ReLU stays float32 and autocast rounds its result to half in front of the pointwise
# conv: six passes where depthwise_bn_relu_autocast makes one (halo_half_dwconv3x3_* of halo_dwconv.hip: x float32 or half in, y16
# out, every stage rounded where the chain rounds it).  The node's only output is y16 = what autocast's cast would hand the
# pointwise conv; its backward keeps x, y16, w and scale and reads the ReLU's gate off y16 (include/halo_hip.h: where 0 < y32 rounds
# to a half zero the gradient is 0, autograd's passes; the pointwise conv saw 0 there on both sides).  As with depthwise_bn_relu
# the sums are the chain walk's, not the library conv's bits.

autocast_launches = {"fwd": 0, "bwd_data": 0, "bwd_weight": 0}


def _half_code(dtype):
    return {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}.get(dtype)


def _autocast_dtype():
    from .norm import _autocast_dtype as device_autocast_dtype
    return device_autocast_dtype()


def autocast_statement(x, conv, bn, act=None):
    """torch_statement under the current autocast state, then the cast autocast makes in front of the pointwise conv (to the
    device's autocast dtype; to a half x's own dtype, i.e. nothing, with autocast off).  The fallback of
    depthwise_bn_relu_autocast and the stock side of its tests and timings."""
    dt = _autocast_dtype()
    y = torch_statement(x, conv, bn, act)
    return y.to(dt) if dt is not None and y.is_floating_point() else y


def autocast_fallback_reason(x, conv, bn):
    """why depthwise_bn_relu_autocast(x, conv, bn) runs autocast_statement (None: the fused pass serves it).  Reads no device
    memory."""
    why, tensors = _module_reason(conv, bn)
    if why is not None:
        return why
    if not torch.is_tensor(x) or x.dim() != 4:
        return "x is not a (B, C, H, W) tensor"
    dt = _autocast_dtype()
    if dt is None:
        return "autocast is not enabled on the device"
    if _half_code(dt) is None:
        return "the autocast dtype is %s, not float16 or bfloat16" % dt
    if not _is_frozen(bn):                 # nn.BatchNorm2d on a half input is the library's batch norm: one rounding, another chain
        return "under autocast the norm must be a FrozenBatchNorm2d, whose statements promote to float32"
    C, dil = conv.in_channels, _pair(conv.dilation)
    if x.shape[1] != C:
        return "x has %d channels, the conv %d" % (x.shape[1], C)
    if x.dtype != torch.float32 and x.dtype != dt:
        return "x is %s, neither float32 nor the autocast dtype %s" % (x.dtype, dt)
    if not x.is_cuda:
        return "x is not on a ROCm device"
    if not x.is_contiguous():
        return "x is not contiguous NCHW"
    for t in [conv.weight] + tensors:
        if t is not None and (t.dtype != torch.float32 or t.device != x.device):
            return "a conv / norm tensor is not float32 on %s" % x.device
    B, _, H, W = x.shape
    if B * C * H * W == 0:
        return "empty input"
    if max(H, W, dil[0]) > 1 << 24 or H * W > 2 ** 31 - 1:
        return "plane of %d x %d, dilation %d" % (H, W, dil[0])
    return None


class _DepthwiseBnReluAutocastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, scale, shift, d, half):
        B, C, H, W = x.shape
        code = _half_code(half)
        y16 = torch.empty(x.shape, dtype=half, device=x.device)
        _lib.check(_lib.lib().halo_half_dwconv3x3_affine_relu_fwd(_lib.ptr(x), _lib.F32 if x.dtype == torch.float32 else code, _lib.ptr(w),
                                                                  _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y16), code, B, C, H, W, d,
                                                                  _lib.stream_ptr(x.device)), "halo_half_dwconv3x3_affine_relu_fwd")
        autocast_launches["fwd"] += 1
        ctx.save_for_backward(x, y16, w, scale)
        ctx.d, ctx.half = d, half
        return y16

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, y16, w, scale = ctx.saved_tensors
        B, C, H, W = x.shape
        d, code = ctx.d, _half_code(ctx.half)
        x_code = _lib.F32 if x.dtype == torch.float32 else code
        L = _lib.lib()
        st = _lib.stream_ptr(x.device)
        g = g.to(device=x.device, dtype=ctx.half).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(L.halo_half_dwconv3x3_affine_relu_bwd_data(_lib.ptr(g), _lib.ptr(y16), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gx), x_code,
                                                                  code, B, C, H, W, d, st), "halo_half_dwconv3x3_affine_relu_bwd_data")
            autocast_launches["bwd_data"] += 1
        if ctx.needs_input_grad[1]:
            nws = L.halo_dwconv_workspace_bytes(B, C, H, W, d)
            ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=x.device)
            gw = torch.empty_like(w)
            _lib.check(L.halo_half_dwconv3x3_affine_relu_bwd_weight(_lib.ptr(g), _lib.ptr(y16), _lib.ptr(x), x_code, _lib.ptr(scale), _lib.ptr(gw),
                                                                    code, B, C, H, W, d, _lib.ptr(ws), ws.numel() * 8, st),
                       "halo_half_dwconv3x3_affine_relu_bwd_weight")
            autocast_launches["bwd_weight"] += 1
        return gx, gw, None, None, None, None


def depthwise_bn_relu_autocast(x, conv, bn, act=None):
    """relu(bn(conv(x))) of a depthwise 3x3 conv and a frozen / eval-mode norm under torch.autocast, rounded to the autocast dtype
    as the cast in front of the next convolution rounds it: y16 (B, C, H, W), float16 or bfloat16, for an x that is float32 or
    that dtype.  Differentiable once w.r.t. x (the gradient has x's dtype and holds half values) and conv.weight (float32, a
    half's value).  Every stage is rounded where the stock chain rounds it; the nine-term sums are the chain walk's, so a result
    is the stock chain's except where a sum lies within the float32 accumulation error of a half rounding boundary, and then its
    neighbour.  Outside the served envelope (autocast_fallback_reason) it returns autocast_statement(x, conv, bn, act)."""
    if autocast_fallback_reason(x, conv, bn) is not None:
        return autocast_statement(x, conv, bn, act)
    scale, shift = scale_shift(bn)
    return _DepthwiseBnReluAutocastFn.apply(x, conv.weight.contiguous(), scale, shift, int(_pair(conv.dilation)[0]), _autocast_dtype())


def upcat_fallback_reason(a, s, conv, bn):
    """why upsample_cat_depthwise_bn_relu(a, s, conv, bn) runs the composition (None: the fused path serves it).  Reads no device
    memory."""
    why, tensors = _module_reason(conv, bn)
    if why is not None:
        return why
    if _pair(conv.dilation) != (1, 1):
        return "dilation %s, not 1" % (conv.dilation,)
    for name, t in (("a", a), ("s", s)):
        if not torch.is_tensor(t) or t.dim() != 4:
            return "%s is not a (B, C, H, W) tensor" % name
        if t.dtype != torch.float32:
            return "%s is %s, not float32" % (name, t.dtype)
        if not t.is_cuda:
            return "%s is not on a ROCm device" % name
    if a.device != s.device:
        return "a is on %s, s on %s" % (a.device, s.device)
    (B, Ca, h, w), (Bs, Cs, H, W) = a.shape, s.shape
    if B != Bs:
        return "a has %d images, s %d" % (B, Bs)
    if B * Ca * h * w == 0 or B * Cs * H * W == 0:
        return "empty input"
    if H < h or W < w:
        return "s's planes %s are smaller than a's %s: an upsampling only" % ((H, W), (h, w))
    if B * Ca > 1 << 40:                     # halo_bilinear_upsample_bwd's plane count; its H and W limits lie above dw_check's
        return "%d planes to resize" % (B * Ca)
    return _operand_reason((B, Ca + Cs, H, W), torch.float32, True, s.device, conv, tensors)   # the concatenated tensor, which is never made


class _UpCatDepthwiseBnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, s, w, scale, shift):
        (B, Ca, h, wi), (_, Cs, H, W) = a.shape, s.shape
        L = _lib.lib()
        y = torch.empty((B, Ca + Cs, H, W), dtype=torch.float32, device=s.device)
        _lib.check(L.halo_upcat_dwconv3x3_affine_relu_fwd(_lib.ptr(a), _lib.ptr(s), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y),
                                                          B, Ca, Cs, h, wi, H, W, _lib.stream_ptr(s.device)),
                   "halo_upcat_dwconv3x3_affine_relu_fwd")
        ctx.save_for_backward(a, s, y, w, scale)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        a, s, y, w, scale = ctx.saved_tensors
        (B, Ca, h, wi), (_, Cs, H, W) = a.shape, s.shape
        L = _lib.lib()
        st = _lib.stream_ptr(s.device)
        g = g.to(device=s.device, dtype=torch.float32).contiguous()
        need_a, need_s, need_w = ctx.needs_input_grad[:3]
        ga = gs = gw = None
        if getattr(ctx, "joint", False) and need_a and need_s and need_w:
            nws = L.halo_dwconv_workspace_bytes(B, Ca + Cs, H, W, 1)
            ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=s.device)
            gup = torch.empty((B, Ca, H, W), dtype=torch.float32, device=s.device)
            gs, gw, ga = torch.empty_like(s), torch.empty_like(w), torch.empty_like(a)
            _lib.check(L.halo_joint_upcat_dwconv3x3_affine_relu_bwd(_lib.ptr(g), _lib.ptr(y), _lib.ptr(a), _lib.ptr(s), _lib.ptr(w),
                                                                    _lib.ptr(scale), _lib.ptr(gup), _lib.ptr(gs), _lib.ptr(gw), B, Ca, Cs, h,
                                                                    wi, H, W, _lib.ptr(ws), ws.numel() * 8, st),
                       "halo_joint_upcat_dwconv3x3_affine_relu_bwd")
            joint_launches["upcat"] += 1
            _lib.check(L.halo_bilinear_upsample_bwd(_lib.ptr(gup), _lib.ptr(ga), _lib.dtype_code(gup), B * Ca, h, wi, H, W, st),
                       "halo_bilinear_upsample_bwd")
            return ga, gs, gw, None, None
        if need_a or need_s:
            gup = torch.empty((B, Ca, H, W), dtype=torch.float32, device=s.device) if need_a else None
            gs = torch.empty_like(s) if need_s else None
            _lib.check(L.halo_upcat_dwconv3x3_affine_relu_bwd_data(_lib.ptr(g), _lib.ptr(y), _lib.ptr(w), _lib.ptr(scale),
                                                                   _lib.ptr(gup) if need_a else None, _lib.ptr(gs) if need_s else None,
                                                                   B, Ca, Cs, H, W, st), "halo_upcat_dwconv3x3_affine_relu_bwd_data")
            if need_a:
                ga = torch.empty_like(a)
                _lib.check(L.halo_bilinear_upsample_bwd(_lib.ptr(gup), _lib.ptr(ga), _lib.dtype_code(gup), B * Ca, h, wi, H, W, st),
                           "halo_bilinear_upsample_bwd")
                del gup
        if need_w:
            nws = L.halo_dwconv_workspace_bytes(B, Ca + Cs, H, W, 1)
            ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=s.device)
            gw = torch.empty_like(w)
            _lib.check(L.halo_upcat_dwconv3x3_affine_relu_bwd_weight(_lib.ptr(g), _lib.ptr(y), _lib.ptr(a), _lib.ptr(s), _lib.ptr(scale),
                                                                     _lib.ptr(gw), B, Ca, Cs, h, wi, H, W, _lib.ptr(ws), ws.numel() * 8, st),
                       "halo_upcat_dwconv3x3_affine_relu_bwd_weight")
        return ga, gs, gw, None, None


class _UpCatDepthwiseBnReluFnJoint(torch.autograd.Function):
    """the same node with ctx.joint set: its backward takes the joint entry when all three gradients are wanted (a sibling, as above)"""
    @staticmethod
    def forward(ctx, *args):
        ctx.joint = True
        return _UpCatDepthwiseBnReluFn.forward(ctx, *args)

    backward = staticmethod(_UpCatDepthwiseBnReluFn.backward)


def upsample_cat_depthwise_bn_relu(a, s, conv, bn, act=None, joint_backward=False):
    """relu(bn(conv(cat([resize(a, s.shape[2:]), s], 1)))) for a (B, Ca, h, w), s (B, Cs, H, W), a depthwise 3x3 conv of Ca + Cs
    channels at dilation 1 and a frozen / eval-mode norm: y (B, Ca + Cs, H, W), the resize bilinear with align_corners=True.
    Neither the resized nor the concatenated tensor is stored, forward or backward.  Differentiable once w.r.t. a, s and
    conv.weight.  The bits are those of depthwise_bn_relu(torch.cat([bilinear_resize(a, (H, W)), s], 1), conv, bn): not those of
    the stock F.interpolate / nn.Conv2d chain.  Outside the served envelope (upcat_fallback_reason) it returns
    depthwise_bn_relu(torch.cat([resize_or_interpolate(a, (H, W)), s], 1), conv, bn, act), which has its own fallbacks.
    joint_backward=True: a backward that wants the gradients of a, s and conv.weight computes them in one pass
    (upcat_joint_fallback_reason; the same bits); the composition outside the envelope gets the keyword as well."""
    if upcat_fallback_reason(a, s, conv, bn) is not None:
        from .resize import resize_or_interpolate
        return depthwise_bn_relu(torch.cat([resize_or_interpolate(a, tuple(s.shape[2:])), s], 1), conv, bn, act, joint_backward)
    scale, shift = scale_shift(bn)
    fn = _UpCatDepthwiseBnReluFnJoint if joint_backward and upcat_joint_fallback_reason(a, s, conv, bn) is None else _UpCatDepthwiseBnReluFn
    return fn.apply(a.contiguous(), s.contiguous(), conv.weight.contiguous(), scale, shift)


# ---------------------------------------------------------------- the ASPP pyramid: N dilations over one input
# Both v3+ heads hand one tensor to three dilated blocks.  multi_depthwise_bn_relu(x, blocks) runs their depthwise halves as one
# pass each way (halo_multi_dwconv3x3_* of halo_dwconv.hip: a workgroup keeps a plane in LDS): x is read once for the N outputs,
# and the N input gradients are added in LDS and written once.  Every result carries the bits of the composition
#     y_i = depthwise_bn_relu(x, conv_i, bn_i);  g_x = ((gx_0 + gx_1) + gx_2) ... (torch float32 adds in list order, the outputs
#     that were not used left out);  g_w_i: the same halo_dwconv3x3_affine_relu_bwd_weight call over the same operands
# so the fallback, which is that composition, never changes a bit.

launches = {"multi_fwd": 0, "multi_bwd": 0}
MULTI_MIN, MULTI_MAX = 2, 4                                          # DWM_MAX_N of halo_dwconv.hip
# A speed rule only (both sides return the same bits; the GPU tests switch it off): the smallest input timed against the
# composition, 1 x 2048 x 80 x 160 (profiles/r23_time_aspp_depthwise.txt).  Nothing smaller was measured, so nothing smaller is served.
MULTI_MIN_ELEMENTS = 1 * 2048 * 80 * 160


def multi_max_plane():
    """the largest H * W the multi-dilation passes serve: two float32 planes of it fill a CU's LDS (a host-only query)"""
    return int(_lib.lib().halo_multi_dwconv_max_plane())


def multi_fallback_reason(x, blocks):
    """why multi_depthwise_bn_relu(x, blocks) runs one depthwise_bn_relu per block (None: the fused passes serve it).  blocks: a
    sequence of (conv, bn) or (conv, bn, act).  Reads no device memory."""
    blocks = [tuple(b) for b in blocks]
    if not MULTI_MIN <= len(blocks) <= MULTI_MAX:
        return "%d blocks, %d to %d are served" % (len(blocks), MULTI_MIN, MULTI_MAX)
    if any(len(b) not in (2, 3) for b in blocks):
        return "a block is not (conv, bn) or (conv, bn, act)"
    channels = [getattr(b[0], "in_channels", None) for b in blocks]
    if len(set(channels)) != 1:
        return "the blocks' channel counts differ: %s" % (channels,)
    for i, b in enumerate(blocks):
        why = fallback_reason(x, b[0], b[1])
        if why is not None:
            return "block %d: %s" % (i, why)
    B, C, H, W = x.shape
    if H * W > multi_max_plane():
        return "plane of %d x %d = %d elements, above the %d that fit the LDS twice" % (H, W, H * W, multi_max_plane())
    if B * C * H * W < MULTI_MIN_ELEMENTS:
        return "%d elements, fewer than MULTI_MIN_ELEMENTS = %d (a speed rule: nothing smaller was timed)" % (B * C * H * W, MULTI_MIN_ELEMENTS)
    return None


def multi_forward(x, scale, shift, dil, ws):
    """the forward launch over contiguous x: (w (n, C, 9) stacked, y (n, B, C, H, W)); counted as launches["multi_fwd"]"""
    import ctypes
    B, C, H, W = x.shape
    n = len(ws)
    w = torch.stack([wi.reshape(C, 9) for wi in ws])
    y = torch.empty((n, B, C, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().halo_multi_dwconv3x3_affine_relu_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, C, H, W,
                                                               n, (ctypes.c_int64 * n)(*dil), _lib.stream_ptr(x.device)),
               "halo_multi_dwconv3x3_affine_relu_fwd")
    launches["multi_fwd"] += 1
    return w, y


def multi_weight_grads(gs, x, y, scale, dil, wanted):
    """[g_w_i or None]: one halo_dwconv3x3_affine_relu_bwd_weight call per gradient that arrived (gs[i] contiguous float32, or None)
    and is wanted"""
    B, C, H, W = x.shape
    L = _lib.lib()
    st = _lib.stream_ptr(x.device)
    gws = [None] * len(gs)
    for i, g in enumerate(gs):
        if g is None or not wanted[i]:
            continue
        nws = L.halo_dwconv_workspace_bytes(B, C, H, W, dil[i])
        ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=x.device)
        gws[i] = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=x.device)
        _lib.check(L.halo_dwconv3x3_affine_relu_bwd_weight(_lib.ptr(g), _lib.ptr(y[i]), _lib.ptr(x), _lib.ptr(scale[i]), _lib.ptr(gws[i]), B, C,
                                                           H, W, dil[i], _lib.ptr(ws), ws.numel() * 8, st),
                   "halo_dwconv3x3_affine_relu_bwd_weight")
    return gws


class _MultiDepthwiseBnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift, dil, *ws):
        w, y = multi_forward(x, scale, shift, dil, ws)
        ctx.save_for_backward(x, y, w, scale)
        ctx.dil = dil
        ctx.set_materialize_grads(False)
        return tuple(y.unbind(0))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        import ctypes
        x, y, w, scale = ctx.saved_tensors
        B, C, H, W = x.shape
        n, dil = len(gs), ctx.dil
        gs = [None if g is None else g.to(device=x.device, dtype=torch.float32).contiguous() for g in gs]
        gx = None
        if all(g is None for g in gs):
            return (None,) * (4 + n)
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            ptrs = (ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in gs])
            _lib.check(_lib.lib().halo_multi_dwconv3x3_affine_relu_bwd_data(ptrs, _lib.ptr(y), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(gx), B, C, H,
                                                                            W, n, (ctypes.c_int64 * n)(*dil), _lib.stream_ptr(x.device)),
                       "halo_multi_dwconv3x3_affine_relu_bwd_data")
            launches["multi_bwd"] += 1
        return (gx, None, None, None) + tuple(multi_weight_grads(gs, x, y, scale, dil, ctx.needs_input_grad[4:]))


def multi_operands(x, blocks):
    """(x contiguous, scale (n, C), shift (n, C), the dilations, the contiguous weights): what the passes read of served blocks"""
    pairs = [scale_shift(b[1]) for b in blocks]
    scale, shift = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    dil = tuple(int(_pair(b[0].dilation)[0]) for b in blocks)
    return x.contiguous(), scale, shift, dil, [b[0].weight.contiguous() for b in blocks]


def multi_depthwise_bn_relu(x, blocks):
    """(relu(bn_i(conv_i(x))) for every block) of N = 2..4 depthwise 3x3 convs with frozen / eval-mode norms over one x (B, C, H, W):
    a tuple of N tensors.  blocks: a sequence of (conv, bn) or (conv, bn, act).  Differentiable once w.r.t. x and every
    conv.weight; one launch forward, one for g_x, one halo_dwconv3x3_affine_relu_bwd_weight per weight.  The bits are those of
    tuple(depthwise_bn_relu(x, *block) for block in blocks) and of its autograd (g_x added in list order), which is what runs
    outside the served envelope (multi_fallback_reason)."""
    blocks = [tuple(b) for b in blocks]
    if multi_fallback_reason(x, blocks) is not None:
        # called last block first: the engine runs the nodes made last first and adds the gradients of x as they arrive, so the
        # composition's g_x is ((gx_0 + gx_1) + gx_2) ... as well
        return tuple(reversed([depthwise_bn_relu(x, *b) for b in reversed(blocks)]))
    x, scale, shift, dil, ws = multi_operands(x, blocks)
    return _MultiDepthwiseBnReluFn.apply(x, scale, shift, dil, *ws)


__all__ = ["depthwise_bn_relu", "torch_statement", "fallback_reason", "scale_shift", "upsample_cat_depthwise_bn_relu", "upcat_fallback_reason",
           "multi_depthwise_bn_relu", "multi_fallback_reason", "multi_max_plane", "launches", "joint_fallback_reason",
           "upcat_joint_fallback_reason", "joint_launches", "JOINT_MIN_ELEMENTS", "depthwise_bn_relu_autocast", "autocast_fallback_reason",
           "autocast_statement", "autocast_launches"]
