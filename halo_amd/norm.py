"""A frozen norm, the residual add and the ReLU of a ResNet block (core/models/resnet.py:53-69, 92-112) on the device.

Every shipped config trains deeplabv3plus_resnet101 with MODEL.FREEZE_BN, so every norm of the backbone and every dense norm of
the heads is a FrozenBatchNorm2d (core/models/layers.py) whose forward is torch statements: four tiny kernels for scale and bias,
a broadcast mul and a broadcast add over the activation, then an in-place ReLU -- and, at the end of a residual block, an in-place
`out += identity` and another ReLU.  `norm_relu(x, bn, residual=None, residual_bn=None)` computes

    out = bn(x);   out += residual_bn(residual)  or  out += residual;   relu(out)

and the gradients for x and residual with halo_norm.hip: one read of every operand and one write, forward and backward; the
backward keeps y, scale and r_scale and nothing else.  The kernel runs the chain's own operations with the chain's roundings
(product, sum, sum, comparison; no fma), so its results are the chain's bits, not an approximation of them.

Served (fallback_reason is None): x float32 (B, C, H, W) on the device, contiguous NCHW, non-empty, no autocast; bn (and
residual_bn) a module whose type is named FrozenBatchNorm2d with its four float32 buffers of C channels on x's device; residual
of x's shape, dtype and device, contiguous.  Anything else -- eval-mode nn.BatchNorm2d (one ATen kernel with another rounding
order), channels-last, other dtypes, CPU tensors -- runs the stock statements (torch_statement), which keep torch's results and
errors.  One rule is about speed alone: a small tensor that needs a gradient runs the stock statements too (AUTOGRAD_MIN_ELEMENTS).

scale and shift are the module's own two statements as torch ops (halo_amd.dwconv.scale_shift: no eps).  The stock module
recomputes them on every call; here the pair is cached per norm instance, keyed on the identity and the `_version` of the four
buffers, which the entry holds references to.  load_state_dict and every in-place write through the buffer bump `_version`;
.to() / .cuda() / an assignment replace the tensor object: each makes the next call recompute.  The one write torch does not
version is one through a detached alias (`bn.weight.data.mul_()`, or a write through a tensor obtained with .detach() under
inference mode); call `forget(bn)` after such a write.  A buffer without a version counter (an inference-mode tensor) is never
cached.

`norm_relu_fork(x, bn, residual, residual_bn)` is norm_relu for a result that two consumers read (a block output inside a ResNet
layer): it returns the tensor twice from one autograd node, whose backward adds the two arriving gradients inside its own pass.

`norm_relu_dropout2d(x, bn, drop)` further down is the same pass with nn.Dropout2d's per-plane multiplier folded in: the tail of a
separable block and the dropout module behind it (the hyperbolic v3+ head's decoder[1], decoder[2]).
`norm_relu_dropout2d_pair(x, bn, drop)` returns the tensor in front of the dropout as well (the Euclidean v3+ head's old decoder
layout, which hands both on).

`norm_relu_maxpool(x, bn, pool)` at the end is the backbone's stem behind its convolution: the norm, the ReLU and
nn.MaxPool2d(3, 2, 1) in one pass each way (halo_maxpool.hip), which keeps one byte per output element for the backward.
"""
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .dwconv import _is_frozen, scale_shift
from .hfr import _autocast

_BUFFERS = ("weight", "bias", "running_mean", "running_var")
_cache = weakref.WeakKeyDictionary()          # norm module -> (the four keyed buffers, their versions, (scale, shift))
# device launches issued by this module (tests count them): "fwd" / "bwd" of norm_relu, "masked_fwd" / "masked_bwd" of
# norm_relu_dropout2d's own kernels, "pair_fwd" / "pair_bwd" of norm_relu_dropout2d_pair's, "pool_fwd" / "pool_bwd" of
# norm_relu_maxpool's ("pool_taps": the pool_fwd launches that kept the tap codes for a backward), "fork_bwd" of norm_relu_fork's
# two-gradient backward (its forward and its one-gradient backward are norm_relu's launches and count as "fwd" / "bwd"), "ac_fwd" /
# "ac_bwd" of norm_relu_autocast's
launches = {"fwd": 0, "bwd": 0, "fork_bwd": 0, "masked_fwd": 0, "masked_bwd": 0, "pair_fwd": 0, "pair_bwd": 0, "pool_fwd": 0, "pool_bwd": 0, "pool_taps": 0,
            "ac_fwd": 0, "ac_bwd": 0}
# A speed rule, not a correctness rule (both sides return the same bits).  When a gradient will be asked for, a forward + backward
# pair through the Python autograd node costs about 0.16 ms of host time whatever the size; measured alone, back to back, the stock
# chain's pair is shorter than that below these element counts (2 x 512 x 80 x 160 loses without a residual_bn
# and wins with one, 2 x 1024 x 80 x 160 wins in every variant).  Smaller tensors that require a gradient run the stock statements;
# without a gradient (no_grad, inputs that need none) every size is served.  Set both to 0 to serve every size.
# "masked" is norm_relu_dropout2d's pass with nn.Dropout2d in training mode: the smallest size timed that wins in two separate runs
# (2 x 512 x 80 x 160 wins by 2 to 7 %, 1 x 512 x 90 x 160 loses, the decoder's 2 x 512 x 160 x 320 wins x2.8).
AUTOGRAD_MIN_ELEMENTS = {"plain": 2 * 1024 * 80 * 160, "affine": 2 * 512 * 80 * 160, "masked": 2 * 512 * 80 * 160}


def torch_statement(x, bn, residual=None, residual_bn=None):
    """the stock statements of a block's tail (resnet.py:103-110), or of `bn, relu` alone"""
    out = bn(x)
    if residual is not None:
        out += residual if residual_bn is None else residual_bn(residual)
    return F.relu(out, inplace=True)


def _norm_reason(bn, C, device, what):
    if not _is_frozen(bn):
        return "%s is not a FrozenBatchNorm2d" % what
    for n in _BUFFERS:
        t = bn._buffers[n]
        if t.dtype != torch.float32 or t.device != device:
            return "%s.%s is not float32 on %s" % (what, n, device)
        if t.dim() != 1 or t.numel() != C:
            return "%s.%s has shape %s, x has %d channels" % (what, n, tuple(t.shape), C)
    return None


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(getattr(t, "requires_grad", False) for t in tensors)


def _speed_reason(reason, least, x, *others):
    """a *_fallback_reason behind its envelope's `reason`: the speed rule's sentence for a served x of fewer than `least` elements
    when it, or one of `others`, will be asked for a gradient"""
    if reason is None and _wants_grad(x, *others) and x.numel() < least:
        return "under autograd %d elements are fewer than the %d from which the fused pair was measured faster" % (x.numel(), least)
    return reason


def _call(key, name, device, tensors, *dims):
    """one launch, counted under launches[key]: the library's entry `name`, looked up when it is called, over the tensors'
    pointers (None: a null pointer), the dimensions and the device's current stream"""
    launches[key] += 1
    _lib.check(getattr(_lib.lib(), name)(*[_lib.ptr(t) for t in tensors], *dims, _lib.stream_ptr(device)), name)


def fallback_reason(x, bn, residual=None, residual_bn=None):
    """why norm_relu(x, bn, residual, residual_bn) runs the torch statements (None: the fused path serves it).  Reads no device
    memory."""
    return _speed_reason(_envelope_reason(x, bn, residual, residual_bn), AUTOGRAD_MIN_ELEMENTS["affine" if residual_bn is not None else "plain"],
                         x, residual)


def _envelope_reason(x, bn, residual, residual_bn):
    if not torch.is_tensor(x) or x.dim() != 4:
        return "x is not a (B, C, H, W) tensor"
    if x.dtype != torch.float32:
        return "x is %s, not float32" % x.dtype
    if _autocast():
        return "autocast is enabled"
    if not x.is_cuda:
        return "x is not on a ROCm device"
    if x.numel() == 0:
        return "empty input"
    if not x.is_contiguous():
        return "x is not contiguous NCHW"
    C = x.shape[1]
    if x.shape[2] * x.shape[3] > 2 ** 31 - 1025:
        return "plane of %d x %d" % (x.shape[2], x.shape[3])
    r = _norm_reason(bn, C, x.device, "bn")
    if r is not None:
        return r
    if residual is None:
        if residual_bn is not None:
            return "residual_bn without a residual"
        return None
    if not torch.is_tensor(residual) or residual.shape != x.shape:
        return "residual does not have x's shape"
    if residual.dtype != x.dtype or residual.device != x.device:
        return "residual is not %s on %s" % (x.dtype, x.device)
    if not residual.is_contiguous():
        return "residual is not contiguous NCHW"
    if residual_bn is not None:
        return _norm_reason(residual_bn, C, x.device, "residual_bn")
    return None


def cached_scale_shift(bn):
    """(scale, shift) of a frozen norm; the tensors of the previous call while its four buffers are the same objects at the same
    versions"""
    bufs = tuple(bn._buffers[n] for n in _BUFFERS)
    try:
        versions = tuple(t._version for t in bufs)
    except RuntimeError:                       # inference tensors carry no version counter: nothing to key on
        _cache.pop(bn, None)
        return scale_shift(bn)
    hit = _cache.get(bn)
    if hit is not None and hit[1] == versions and all(a is b for a, b in zip(hit[0], bufs)):
        return hit[2]
    pair = scale_shift(bn)
    _cache[bn] = (bufs, versions, pair)
    return pair


def forget(bn=None):
    """drop the cached (scale, shift) of one norm, or of all"""
    if bn is None:
        _cache.clear()
    else:
        _cache.pop(bn, None)


def _tail_forward(ctx, x, scale, shift, r, r_scale, r_shift):
    """the forward of both block-tail nodes"""
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    _call("fwd", "halo_affine_relu_fwd", x.device, (x, scale, shift, r, r_scale, r_shift, y), B, C, H * W)
    ctx.save_for_backward(y, scale, r_scale)
    return y


def _tail_backward(ctx, *grads):
    """the backward of both: (g_x, g_r) from the gradients that arrived at y, one pass for one of them and for two"""
    y, scale, r_scale = ctx.saved_tensors
    B, C, H, W = y.shape
    want_x, want_r = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
    grads = [g for g in grads if g is not None]
    if not (want_x or want_r) or not grads:
        return None, None
    grads = [g.to(device=y.device, dtype=torch.float32).contiguous() for g in grads]
    gx = torch.empty_like(y) if want_x else None
    gr = torch.empty_like(y) if want_r else None
    if len(grads) == 2:
        _call("fork_bwd", "halo_fork_affine_relu_bwd", y.device, (grads[0], grads[1], y, scale, r_scale, gx, gr), B, C, H * W)
    else:
        _call("bwd", "halo_affine_relu_bwd", y.device, (grads[0], y, scale, r_scale, gx, gr), B, C, H * W)
    return gx, gr


class _NormReluFn(torch.autograd.Function):
    forward = staticmethod(_tail_forward)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gx, gr = _tail_backward(ctx, g)
        return gx, None, None, gr, None, None


def _tail_operands(x, bn, residual, residual_bn):
    """the arguments of both block-tail nodes, for arguments that the envelope has accepted"""
    scale, shift = cached_scale_shift(bn)
    r_scale, r_shift = cached_scale_shift(residual_bn) if residual_bn is not None else (None, None)
    return x, scale, shift, residual, r_scale, r_shift


def norm_relu(x, bn, residual=None, residual_bn=None):
    """relu(bn(x)), relu(bn(x) + residual) or relu(bn(x) + residual_bn(residual)) of frozen norms, x (B, C, H, W): the stock
    chain's bits.  Differentiable w.r.t. x and residual; x is not modified.  Outside the served envelope (fallback_reason) it
    returns torch_statement(x, bn, residual, residual_bn)."""
    if fallback_reason(x, bn, residual, residual_bn) is not None:
        return torch_statement(x, bn, residual, residual_bn)
    return fused_norm_relu(x, bn, residual, residual_bn)


def fused_norm_relu(x, bn, residual=None, residual_bn=None):
    """norm_relu for arguments that fallback_reason has accepted"""
    return _NormReluFn.apply(*_tail_operands(x, bn, residual, residual_bn))


# ---------------------------------------------------------------- a block tail whose output is read twice
# Inside a ResNet layer the output y of block k is read twice by block k + 1: by its conv1 and as its identity.  In the backward
# two gradients arrive at y, conv1's data gradient and the g_r of block k + 1's tail, and the engine adds them with a stand-alone
# kernel before block k's tail backward reads the sum.  norm_relu_fork returns y twice, as (y, a view of y), from one autograd node
# with two outputs, so both gradients reach its backward, which adds them inside the pass (halo_fork_affine_relu_bwd): one float32
# add per element, autograd's accumulation and its bits, whichever gradient came first.

# norm_relu_fork's own speed rule, of the same kind as AUTOGRAD_MIN_ELEMENTS (a constant of its own: that dict is replaced
# wholesale by its users, and tests read it): with fewer elements than this a tensor that needs a gradient goes through norm_relu
# and its rule, and the engine adds the two gradients as before.  It is the smallest block output timed: in a
# chain of three bottlenecks the two forked tails of 2 x 512 x 80 x 160 are ahead of the parent configuration, which leaves them
# to the stock statements, in both runs, so from this size on the fork is served in every variant -- also where "plain" above is
# larger; 2 x 256 x 160 x 320, 2 x 1024 x 80 x 160 and 2 x 2048 x 80 x 160 win as well.  Nothing smaller was measured.  Set it to 0
# to serve every size.
FORK_AUTOGRAD_MIN_ELEMENTS = 2 * 512 * 80 * 160


def fork_fallback_reason(x, bn, residual=None, residual_bn=None):
    """why norm_relu_fork(x, bn, residual, residual_bn) hands on norm_relu's tensor twice (None: its own two-output node serves
    it).  The envelope is norm_relu's; the size rule is FORK_AUTOGRAD_MIN_ELEMENTS.  Reads no device memory."""
    reason = _envelope_reason(x, bn, residual, residual_bn)
    if reason is not None:
        return reason
    if not _wants_grad(x, residual):
        return "no gradient will be asked for"
    if x.numel() < FORK_AUTOGRAD_MIN_ELEMENTS:
        return "%d elements are fewer than the %d from which the two-gradient backward was measured faster" % (
            x.numel(), FORK_AUTOGRAD_MIN_ELEMENTS)
    return None


class _NormReluForkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *operands):
        y = _tail_forward(ctx, *operands)
        ctx.set_materialize_grads(False)                   # an output nobody used arrives as None and is not read
        return y, y.view_as(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_a, g_b):
        gx, gr = _tail_backward(ctx, g_a, g_b)
        return gx, None, None, gr, None, None


def norm_relu_fork(x, bn, residual=None, residual_bn=None):
    """norm_relu(x, bn, residual, residual_bn) for a result that two consumers read: returns (y, y_id), the same values twice,
    y_id a view of y.  Hand one to each consumer and write in place to neither.  When both send a gradient back, the backward adds
    the two inside its one pass (the engine's accumulation: one float32 add, the stock chain's bits); when one does, it is
    norm_relu's backward; when none does, or no input needs a gradient, nothing is launched.  Outside norm_relu's envelope, where
    no gradient will be asked for, and below FORK_AUTOGRAD_MIN_ELEMENTS (fork_fallback_reason) it returns the same tensor object
    twice, t = norm_relu(x, bn, residual, residual_bn) -- torch_statement's result wherever norm_relu runs the stock statements --
    and autograd does what it does without this operator."""
    if fork_fallback_reason(x, bn, residual, residual_bn) is not None:
        t = norm_relu(x, bn, residual, residual_bn)
        return t, t
    return _NormReluForkFn.apply(*_tail_operands(x, bn, residual, residual_bn))


# ---------------------------------------------------------------- norm + ReLU + Dropout2d
# The pointwise tail of a separable block with the nn.Dropout2d that follows it (the hyperbolic v3+ head's decoder[1], decoder[2]):
#
#     drop(F.relu(bn(x), inplace=True))
#
# ATen's feature dropout (_dropout_impl) draws one number per (image, channel) -- noise = x.new_empty((B, C, 1, 1)).bernoulli_(1 - p)
# .div_(1 - p) -- and multiplies.  norm_relu_dropout2d draws the same tensor with the same statements, so the generator moves as it
# does under nn.Dropout2d and a seeded run has nn.Dropout2d's bits, and hands it to halo_masked_affine_relu_fwd / _bwd as the
# per-plane multiplier.

def dropout_statement(x, bn, drop):
    """the stock statements: the block's pointwise norm and in-place ReLU, then the dropout module"""
    return drop(F.relu(bn(x), inplace=True))


def _drop_reason(x, bn, drop, least):
    """dropout_fallback_reason and pair_fallback_reason, which differ in the speed rule's threshold alone"""
    if not isinstance(drop, nn.Dropout2d):
        return "drop is not an nn.Dropout2d"
    if drop.inplace:
        return "the dropout is in place"
    if not drop.training or drop.p == 0:
        return fallback_reason(x, bn)                      # nothing is drawn: relu(bn(x)) alone
    if drop.p >= 1:
        return "p = 1 drops every plane"
    return _speed_reason(_envelope_reason(x, bn, None, None), least, x)


def _noise(x, drop):
    """nn.Dropout2d's multiplier per (image, channel), drawn with ATen's statements (_dropout_impl, feature dropout)"""
    B, C = x.shape[:2]
    return x.new_empty((B, C, 1, 1)).bernoulli_(1 - drop.p).div_(1 - drop.p)


def dropout_fallback_reason(x, bn, drop):
    """why norm_relu_dropout2d(x, bn, drop) runs the torch statements (None: a fused pass serves it -- the masked one when drop is
    in training mode with 0 < p < 1, norm_relu's otherwise).  Reads no device memory."""
    return _drop_reason(x, bn, drop, AUTOGRAD_MIN_ELEMENTS.get("masked", 0))


class _NormReluDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift, noise):
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        _call("masked_fwd", "halo_masked_affine_relu_fwd", x.device, (x, scale, shift, noise, y), B, C, H * W)
        ctx.save_for_backward(y, scale, noise)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y, scale, noise = ctx.saved_tensors
        B, C, H, W = y.shape
        gx = None
        if ctx.needs_input_grad[0]:
            g = g.to(device=y.device, dtype=torch.float32).contiguous()
            gx = torch.empty_like(y)
            _call("masked_bwd", "halo_masked_affine_relu_bwd", y.device, (g, y, scale, noise, gx), B, C, H * W)
        return gx, None, None, None


def norm_relu_dropout2d(x, bn, drop):
    """drop(relu(bn(x))) of a frozen norm and an nn.Dropout2d, x (B, C, H, W): the stock chain's bits, and the stock chain's use of
    the random generator (one bernoulli_ over (B, C, 1, 1) in training mode with 0 < p < 1, nothing otherwise).  Differentiable
    w.r.t. x; x is not modified; the backward keeps y, scale and the noise tensor.  One deviation, in the backward alone: the ReLU's
    mask is read off the saved y, which is 0 in a dropped plane, so a non-finite output gradient in a dropped plane gives 0 where
    autograd gives NaN; for finite gradients the bits are autograd's.  Outside the served envelope (dropout_fallback_reason) it
    returns dropout_statement(x, bn, drop)."""
    if dropout_fallback_reason(x, bn, drop) is not None:
        return dropout_statement(x, bn, drop)
    if not drop.training or drop.p == 0:
        return fused_norm_relu(x, bn)
    return _NormReluDropFn.apply(x, *cached_scale_shift(bn), _noise(x, drop))


# ---------------------------------------------------------------- norm + ReLU + Dropout2d, both tensors kept
# The Euclidean v3+ head's old decoder layout (classifier.py:308-312) returns decoder[1]'s output as `decoder_out` and feeds the
# tensor behind decoder[2], an nn.Dropout2d, to the classifier conv:
#
#     y = F.relu(bn(x), inplace=True);   z = drop(y)
#
# norm_relu_dropout2d_pair writes both from one read of x (halo_dropout_pair_fwd) and folds the two incoming gradients, either of
# which may be absent, into one backward pass (halo_dropout_pair_bwd).  The noise tensor is drawn as above.

# norm_relu_dropout2d_pair's own speed rule, of the same kind as AUTOGRAD_MIN_ELEMENTS (a constant of its own: that dict is
# replaced wholesale by its users): below this many elements an x that needs a gradient runs the stock statements.  It is the
# smallest size timed (1 x 512 x 90 x 160 wins against the stock statements by 10 to 25 % in both runs, the
# decoder's 2 x 512 x 160 x 320 by x2.2 to x2.3); nothing smaller was measured.  Set it to 0 to serve every size.
PAIR_AUTOGRAD_MIN_ELEMENTS = 1 * 512 * 90 * 160


def pair_statement(x, bn, drop):
    """the stock statements: (the block's pointwise norm and in-place ReLU, the dropout module over that)"""
    y = F.relu(bn(x), inplace=True)
    return y, drop(y)


def pair_fallback_reason(x, bn, drop):
    """why norm_relu_dropout2d_pair(x, bn, drop) runs the torch statements (None: a fused pass serves it -- the two-output one when
    drop is in training mode with 0 < p < 1, norm_relu's otherwise).  The envelope is norm_relu_dropout2d's.  Reads no device
    memory."""
    return _drop_reason(x, bn, drop, PAIR_AUTOGRAD_MIN_ELEMENTS)


class _NormReluDropPairFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift, noise):
        B, C, H, W = x.shape
        y, z = torch.empty_like(x), torch.empty_like(x)
        _call("pair_fwd", "halo_dropout_pair_fwd", x.device, (x, scale, shift, noise, y, z), B, C, H * W)
        ctx.save_for_backward(y, scale, noise)
        ctx.set_materialize_grads(False)                   # an output nobody used arrives as None and is not read
        return y, z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y, g_z):
        y, scale, noise = ctx.saved_tensors
        B, C, H, W = y.shape
        gx = None
        if ctx.needs_input_grad[0] and (g_y is not None or g_z is not None):
            g_y, g_z = (None if g is None else g.to(device=y.device, dtype=torch.float32).contiguous() for g in (g_y, g_z))
            gx = torch.empty_like(y)
            _call("pair_bwd", "halo_dropout_pair_bwd", y.device, (g_y, g_z, y, scale, noise, gx), B, C, H * W)
        return gx, None, None, None


def norm_relu_dropout2d_pair(x, bn, drop):
    """(y, z) = (relu(bn(x)), drop(y)) of a frozen norm and an nn.Dropout2d, x (B, C, H, W): the stock chain's bits in both, and its
    use of the random generator (one bernoulli_ over (B, C, 1, 1) in training mode with 0 < p < 1, nothing otherwise; then z is y,
    as nn.Dropout2d returns its input).  Differentiable w.r.t. x through either output or both; x is not modified; the backward is
    one pass that keeps y, scale and the noise tensor, reads only the gradients that arrived, and gates on y, the ReLU's own
    output.  One deviation, in the backward alone: g_z is not read in a dropped plane, so a non-finite g_z there contributes 0
    where autograd has a NaN; for finite gradients the bits are autograd's.  Outside the served envelope (pair_fallback_reason) it
    returns pair_statement(x, bn, drop)."""
    if pair_fallback_reason(x, bn, drop) is not None:
        return pair_statement(x, bn, drop)
    if not drop.training or drop.p == 0:
        y = fused_norm_relu(x, bn)
        return y, y
    return _NormReluDropPairFn.apply(x, *cached_scale_shift(bn), _noise(x, drop))


# ---------------------------------------------------------------- norm + ReLU + MaxPool2d(3, 2, 1): the stem
# The stem of the backbone behind conv1 (core/models/resnet.py:191-195), on the largest activation of the network:
#
#     pool(F.relu(bn(x), inplace=True))                      pool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
#
# norm_relu_maxpool reads x once and writes the pooled tensor and one byte per pooled element: the place of the recorded tap in
# its window, or "blocked" when the ReLU let nothing through there.  The backward is a gather over those bytes and the incoming
# gradient; neither the rectified tensor nor the pool's int64 indices exist.  The scan order, the tie and NaN rule and the
# order of the backward's sums are ATen's (halo_maxpool.hip; tests/stem_pool_ref.py is the restatement).

# norm_relu_maxpool's own speed rule, of the same kind as AUTOGRAD_MIN_ELEMENTS (a constant of its own: that dict is replaced
# wholesale by its users): below this many elements an x that needs a gradient runs norm_relu and the stock pool.  Under autograd
# all three chains sit on the host's cost of a pair of autograd nodes up to this size (at 2 x 64 x 160 x 320
# the fused pair is ahead of norm_relu + pool in both runs, x1.05 and x2.00, and level with or ahead of the stock statements, x1.00
# and x1.98; at 2 x 64 x 80 x 160 x1.03 and x1.54, x1.00 and x1.42, with the stock statements ahead in an earlier run), so the
# threshold is the larger of the two small shapes timed; the stem's real shapes, 26 M elements and more, win x2.5 to x5.6.
# Without a gradient every size is served.  Set it to 0 to serve every size.
POOL_AUTOGRAD_MIN_ELEMENTS = 2 * 64 * 160 * 320


def pool_statement(x, bn, pool):
    """the stock statements: the stem's norm and in-place ReLU, then the pool module"""
    return pool(F.relu(bn(x), inplace=True))


def _pair_of(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _pool_reason(pool):
    """why a pool module is not the stem's nn.MaxPool2d(3, 2, 1) (None: it is)"""
    if type(pool) is not nn.MaxPool2d:
        return "pool is not an nn.MaxPool2d"
    for name, want in (("kernel_size", 3), ("stride", 2), ("padding", 1), ("dilation", 1)):
        try:
            got = _pair_of(getattr(pool, name))
        except TypeError:
            got = None
        if got != (want, want):
            return "the pool's %s is %r, not %d" % (name, getattr(pool, name), want)
    if pool.ceil_mode:
        return "the pool rounds its output size up (ceil_mode)"
    if pool.return_indices:
        return "the pool returns its indices"
    return None


def pool_fallback_reason(x, bn, pool):
    """why norm_relu_maxpool(x, bn, pool) runs the torch statements (None: the fused pass serves it).  Reads no device memory."""
    return _speed_reason(_pool_reason(pool) or _envelope_reason(x, bn, None, None), POOL_AUTOGRAD_MIN_ELEMENTS, x)


class _NormReluPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift, keep):
        B, C, H, W = x.shape
        shape = (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
        out = x.new_empty(shape)
        tap = torch.empty(shape, dtype=torch.uint8, device=x.device) if keep else None      # no backward will come: no codes
        launches["pool_taps"] += keep
        _call("pool_fwd", "halo_maxpool_affine_relu_fwd", x.device, (x, scale, shift, out, tap), B, C, H, W)
        if keep:
            ctx.save_for_backward(tap, scale)
        ctx.x_shape = (B, C, H, W)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gx = None
        if ctx.needs_input_grad[0]:
            tap, scale = ctx.saved_tensors
            B, C, H, W = ctx.x_shape
            g = g.to(device=tap.device, dtype=torch.float32).contiguous()
            gx = torch.empty(ctx.x_shape, dtype=torch.float32, device=tap.device)
            _call("pool_bwd", "halo_maxpool_affine_relu_bwd", tap.device, (g, tap, scale, gx), B, C, H, W)
        return gx, None, None, None


def norm_relu_maxpool(x, bn, pool):
    """pool(relu(bn(x))) of a frozen norm and an nn.MaxPool2d(3, 2, 1), x (B, C, H, W): the stock chain's bits, forward and
    backward.  Differentiable w.r.t. x; x is not modified; the backward keeps one byte per output element and scale, and the
    forward writes those bytes only when a gradient for x will be asked for.  Outside the served envelope (pool_fallback_reason)
    it returns pool_statement(x, bn, pool) -- except that an x the speed rule alone turns away runs norm_relu and the pool."""
    if pool_fallback_reason(x, bn, pool) is not None:
        if _pool_reason(pool) is None and fallback_reason(x, bn) is None:
            return pool(fused_norm_relu(x, bn))
        return pool_statement(x, bn, pool)
    return fused_norm_relu_maxpool(x, bn)


def fused_norm_relu_maxpool(x, bn):
    """norm_relu_maxpool for arguments that pool_fallback_reason has accepted"""
    scale, shift = cached_scale_shift(bn)
    return _NormReluPoolFn.apply(x, scale, shift, bool(torch.is_grad_enabled() and x.requires_grad))


# ---------------------------------------------------------------- the block tail under torch.autocast
# Under autocast the convolution in front returns half (float16 or bfloat16), FrozenBatchNorm2d's `x * scale + bias` over float32
# buffers promotes to float32, the in-place ReLU and `out += identity` stay float32, and the next convolution has autocast round
# that float32 tensor to half with a kernel of its own.  norm_relu_autocast runs the chain in one pass with every operand in its own
# element type (halo_norm_autocast.hip): half -> float is exact, the statements are norm_relu's, and the half output is the
# round-to-nearest-even half of the float32 result -- what autocast's cast hands the next convolution.  The backward is autograd's
# for the chain plus the casts: g = g32, float(g16) or fl(g32 + float(g16)), gp = s <= 0 ? 0 : g, g_x = half(fl(gp * scale)),
# g_r = gp for a float32 identity or half(fl(gp * r_scale)) for a downsample convolution's half output.

OUTPUTS = ("float", "half", "both")
_HALF_CODES = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
# norm_relu_autocast's own speed rule, of the same kind as AUTOGRAD_MIN_ELEMENTS (constants of its own, not copies of the float32
# thresholds: the stock chain under autocast moves 28 to 42 bytes per element where the float32 chain moves 20 to 32): below these
# element counts an x that needs a gradient runs the stock statements; without a gradient every size is served.  Keyed by
# `outputs`, or "affine" with a residual_bn.  Each is the smallest size timed at which forward + backward won in every process
# (profiles/r29_time_autocast_norm.txt: two processes over all shapes, four more over "both"): "half" from
# 2 x 128 x 80 x 160 (x1.3 to x1.4), "float" and the half residual from 2 x 512 x 80 x 160 (x1.9 to x3.2; nothing smaller was timed),
# "both" from 2 x 1024 x 80 x 160 -- at 2 x 512 x 80 x 160 it won x2.3 and x2.4 in the two processes and lost x0.96 in one of the four
# further ones, on a host that took 0.2 ms for the pair of autograd nodes.  Set every value to 0 to serve every size.
AUTOCAST_AUTOGRAD_MIN_ELEMENTS = {"half": 2 * 128 * 80 * 160, "float": 2 * 512 * 80 * 160, "both": 2 * 1024 * 80 * 160, "affine": 2 * 512 * 80 * 160}


def _autocast_dtype():
    """the device's autocast dtype when autocast is on there, else None"""
    try:
        return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    except TypeError:                                      # torch without the device-type argument
        return torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else None


def autocast_statement(x, bn, residual=None, residual_bn=None, outputs="float"):
    """torch_statement under the current autocast state, plus `.to(x.dtype)` for the half output: y32, y16 or (y32, y16).  The
    fallback of norm_relu_autocast and the oracle of its tests."""
    if outputs not in OUTPUTS:
        raise ValueError("outputs is %r, not one of %s" % (outputs, ", ".join(OUTPUTS)))
    y = torch_statement(x, bn, residual, residual_bn)
    if outputs == "float":
        return y
    return y.to(x.dtype) if outputs == "half" else (y, y.to(x.dtype))


def _autocast_envelope_reason(x, bn, residual, residual_bn, outputs):
    if outputs not in OUTPUTS:
        return "outputs is %r, not one of %s" % (outputs, ", ".join(OUTPUTS))
    if not torch.is_tensor(x) or x.dim() != 4:
        return "x is not a (B, C, H, W) tensor"
    dt = _autocast_dtype()
    if dt is None:
        return "autocast is not enabled on the device"
    if x.dtype not in _HALF_CODES:
        return "x is %s, not float16 or bfloat16" % x.dtype
    if dt != x.dtype:
        return "the autocast dtype is %s, x is %s" % (dt, x.dtype)
    if not x.is_cuda:
        return "x is not on a ROCm device"
    if x.numel() == 0:
        return "empty input"
    if not x.is_contiguous():
        return "x is not contiguous NCHW"
    C = x.shape[1]
    if x.shape[2] * x.shape[3] > 2 ** 31 - 1025:
        return "plane of %d x %d" % (x.shape[2], x.shape[3])
    r = _norm_reason(bn, C, x.device, "bn")
    if r is not None:
        return r
    if residual is None:
        if residual_bn is not None:
            return "residual_bn without a residual"
        return None
    if outputs == "half":
        return "the half output alone is served without a residual"
    if not torch.is_tensor(residual) or residual.shape != x.shape:
        return "residual does not have x's shape"
    if residual.device != x.device:
        return "residual is not on %s" % (x.device,)
    if residual_bn is None:
        if residual.dtype != torch.float32:
            return "residual is %s without a residual_bn: an identity is float32" % residual.dtype
    elif residual.dtype != x.dtype:
        return "residual is %s with a residual_bn: a downsample convolution's output is %s" % (residual.dtype, x.dtype)
    if not residual.is_contiguous():
        return "residual is not contiguous NCHW"
    if residual_bn is not None:
        return _norm_reason(residual_bn, C, x.device, "residual_bn")
    return None


def autocast_fallback_reason(x, bn, residual=None, residual_bn=None, outputs="float"):
    """why norm_relu_autocast(x, bn, residual, residual_bn, outputs) runs autocast_statement (None: the fused pass serves it).
    Reads no device memory."""
    least = AUTOCAST_AUTOGRAD_MIN_ELEMENTS.get("affine" if residual_bn is not None else outputs, 0)
    return _speed_reason(_autocast_envelope_reason(x, bn, residual, residual_bn, outputs), least, x, residual)


class _AutocastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift, r, r_scale, r_shift, outputs):
        B, C, H, W = x.shape
        y32 = torch.empty(x.shape, dtype=torch.float32, device=x.device) if outputs != "half" else None
        y16 = torch.empty_like(x) if outputs != "float" else None
        _call("ac_fwd", "halo_autocast_norm_relu_fwd", x.device, (x, scale, shift, r, r_scale, r_shift, y32, y16), _HALF_CODES[x.dtype], B, C, H * W)
        if y32 is None:
            ctx.save_for_backward(x, scale, shift)         # no y32 to read the gate off: pre is recomputed from x
        else:
            ctx.save_for_backward(y32, scale, r_scale)
        ctx.outputs, ctx.half = outputs, x.dtype
        ctx.set_materialize_grads(False)                   # an output nobody used arrives as None and is not read
        return (y32, y16) if outputs == "both" else y32 if outputs == "float" else y16

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        g32, g16 = grads if ctx.outputs == "both" else (grads[0], None) if ctx.outputs == "float" else (None, grads[0])
        want_x, want_r = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        if not (want_x or want_r) or (g32 is None and g16 is None):
            return None, None, None, None, None, None, None
        y32 = x = shift = r_scale = None
        if ctx.outputs == "half":
            x, scale, shift = ctx.saved_tensors
            like = x
        else:
            y32, scale, r_scale = ctx.saved_tensors
            like = y32
        B, C, H, W = like.shape
        g32 = None if g32 is None else g32.to(device=like.device, dtype=torch.float32).contiguous()
        g16 = None if g16 is None else g16.to(device=like.device, dtype=ctx.half).contiguous()
        gx = torch.empty(like.shape, dtype=ctx.half, device=like.device) if want_x else None
        gr = torch.empty(like.shape, dtype=ctx.half if r_scale is not None else torch.float32, device=like.device) if want_r else None
        _call("ac_bwd", "halo_autocast_norm_relu_bwd", like.device, (g32, g16, y32, x, scale, shift, r_scale if want_r else None, gx, gr),
              _HALF_CODES[ctx.half], B, C, H * W)
        return gx, None, None, gr, None, None, None


def norm_relu_autocast(x, bn, residual=None, residual_bn=None, outputs="float"):
    """norm_relu under torch.autocast, for the half x a convolution returns there: the stock chain's bits, and those of the cast
    with which autocast would hand its result to the next convolution.

        outputs="float" -> y32         relu(bn(x) [+ residual | + residual_bn(residual)]), float32 as the stock chain returns it
        outputs="half"  -> y16         y32.to(x.dtype), for a result whose only reader is a convolution (a block's bn1 / bn2
                                       positions); y32 is never written.  Without a residual only
        outputs="both"  -> (y32, y16)  one autograd node with two outputs: a block output that a convolution reads (y16) and an
                                       identity or anything else (y32)

    residual is float32 of x's shape without a residual_bn (a block's identity), or of x's half dtype with one (the downsample
    convolution's output).  Differentiable w.r.t. x and residual; x is not modified; the gradient of x is x's half dtype, that of
    a float32 residual float32.  The backward is one pass: it reads the gradients that arrived (at y32, at y16 or at both, which
    it adds as the engine would: one float32 add), computes only the gradients asked for, and launches nothing when none is.  It
    keeps y32 and the scales.  outputs="half" has no y32, and y16 cannot stand in for the ReLU's gate -- a small positive y32 rounds
    to a half zero, where the chain's gradient passes --, so that node keeps x, which the convolution behind it keeps anyway,
    and its backward recomputes pre = fl(fl(float(x) * scale) + shift) from it.  Outside the served envelope
    (autocast_fallback_reason) it returns autocast_statement(x, bn, residual, residual_bn, outputs)."""
    if autocast_fallback_reason(x, bn, residual, residual_bn, outputs) is not None:
        return autocast_statement(x, bn, residual, residual_bn, outputs)
    return _AutocastFn.apply(*_tail_operands(x, bn, residual, residual_bn), outputs)


__all__ = ["norm_relu", "norm_relu_fork", "fork_fallback_reason", "torch_statement", "fallback_reason", "cached_scale_shift", "forget", "norm_relu_dropout2d",
           "dropout_statement", "dropout_fallback_reason", "norm_relu_dropout2d_pair", "pair_statement", "pair_fallback_reason",
           "norm_relu_maxpool", "pool_statement", "pool_fallback_reason", "norm_relu_autocast", "autocast_statement", "autocast_fallback_reason"]
