"""The training criterion from the head's low-resolution logits (core/train_learners.py:224-243, 328-368, 404-463, 505-563).

Every learner step asks the head for logits at the input size, which upsamples its (B, K, h, w) output with
F.interpolate(align_corners=True), then takes torch.softmax, nn.CrossEntropyLoss(ignore_index=255) and NegativeLearningLoss
on the full-resolution maps and lets autograd take all of it back through the resize.  Here both losses and their joint
gradient come from the low-resolution logits and the label map (halo_train_loss.hip); the full-resolution maps never exist:

    upsampled_losses(logits, label)     -> (ce, nl, n_labelled), ce and nl differentiable w.r.t. logits

This is the training-side counterpart of halo_amd.metrics.  There is no CPU route and no fallback: inputs outside the
served envelope raise.
"""
import collections

import torch

from . import _lib

UpsampledLosses = collections.namedtuple("UpsampledLosses", ["ce", "nl", "n_labelled"])

CE_SUM, CE_COUNT, NL_SUM, NL_COUNT, BAD_LABELS = range(5)       # the kernels' float64 sums vector


class _UpsampledLossFn(torch.autograd.Function):
    """(ce, nl) of one forward launch; one backward launch serves both terms.  The third output, the float64 sums vector, is
    not differentiable (it carries the counts to the caller)."""

    @staticmethod
    def forward(ctx, logits, label, H, W, ignore_index, threshold, terms):
        B, K, h, w = logits.shape
        L = _lib.lib()
        dev = logits.device
        nws = L.halo_upsampled_loss_workspace_bytes(B, K, H, W)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        sums = torch.empty(5, dtype=torch.float64, device=dev)
        _lib.check(L.halo_upsampled_loss_fwd(_lib.ptr(logits), K * h * w, B, K, h, w, _lib.ptr(label), _lib.int_code(label), H, W,
                                             ignore_index, threshold, terms, _lib.ptr(sums), _lib.ptr(ws), nws, _lib.stream_ptr(dev)),
                   "halo_upsampled_loss_fwd")
        ce = (sums[CE_SUM] / sums[CE_COUNT]).to(torch.float32)
        nl = (sums[NL_SUM] / sums[NL_COUNT]).to(torch.float32)
        ctx.save_for_backward(logits, label, sums)
        ctx.args = (H, W, ignore_index, threshold, terms)
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)          # an unused output's gradient stays None: NULL to the kernel, no zero tensor
        return ce, nl, sums

    @staticmethod
    def backward(ctx, g_ce, g_nl, _g_sums):
        logits, label, sums = ctx.saved_tensors
        H, W, ignore_index, threshold, terms = ctx.args
        if g_ce is None and g_nl is None:
            return (None,) * 7
        B, K, h, w = logits.shape
        dev = logits.device
        g_ce = None if g_ce is None else g_ce.to(device=dev, dtype=torch.float32).contiguous()
        g_nl = None if g_nl is None else g_nl.to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty((B, K, h, w), dtype=torch.float32, device=dev)
        L = _lib.lib()
        _lib.check(L.halo_upsampled_loss_bwd(_lib.ptr(logits), K * h * w, B, K, h, w, _lib.ptr(label), _lib.int_code(label), H, W,
                                             ignore_index, threshold, terms, _lib.ptr(sums), _lib.ptr(g_ce), _lib.ptr(g_nl), _lib.ptr(grad),
                                             _lib.stream_ptr(dev)),
                   "halo_upsampled_loss_bwd")
        return grad, None, None, None, None, None, None


def upsampled_losses(logits, label, *, size=None, ignore_index=255, negative_threshold=0.05, cross_entropy=True, negative=True,
                     check_labels=True):
    """nn.CrossEntropyLoss(ignore_index) and NegativeLearningLoss(negative_threshold) of softmax(F.interpolate(logits, size,
    mode='bilinear', align_corners=True)), from the low-resolution logits.

    logits: float32 (B, K, h, w) on the device; label: (B, H, W) int64 / int32 / uint8 on the same device; size defaults to
    label.shape[-2:] and must equal it, and must be at least (h, w) (this path upsamples only).  Returns UpsampledLosses:
    ce and nl float32 0-dim tensors, differentiable w.r.t. logits (None for a term switched off), and n_labelled, the device
    int64 count of labels in [0, K) other than ignore_index.  ce is NaN when nothing is labelled (torch's mean over nothing)
    and its gradient is then zero; nl is sum / count as NegativeLearningLoss.

    A label outside [0, K) that is not ignore_index raises IndexError, as torch's nll_loss does; that check reads one count
    back to the host (a device-to-host sync).  check_labels=False skips it: such labels are then counted and ignored."""
    if not torch.is_tensor(logits) or not torch.is_tensor(label):
        raise TypeError("halo_amd.training: logits and label must be tensors")
    if logits.dtype != torch.float32:
        raise TypeError("halo_amd.training: logits must be float32, got %s" % logits.dtype)
    if label.dtype not in (torch.int64, torch.int32, torch.uint8):
        raise TypeError("halo_amd.training: label must be int64, int32 or uint8, got %s" % label.dtype)
    if not logits.is_cuda or not label.is_cuda:
        raise ValueError("halo_amd.training: logits and label must be on a ROCm device (got %s and %s); there is no CPU route"
                         % (logits.device, label.device))
    if logits.device != label.device:
        raise ValueError("halo_amd.training: logits on %s, label on %s" % (logits.device, label.device))
    if logits.dim() != 4:
        raise ValueError("halo_amd.training: logits must be (B, K, h, w), got %s" % (tuple(logits.shape),))
    B, K, h, w = logits.shape
    if label.dim() != 3 or label.shape[0] != B:
        raise ValueError("halo_amd.training: label must be (%d, H, W) for logits %s, got %s" % (B, tuple(logits.shape), tuple(label.shape)))
    H, W = (int(s) for s in (label.shape[-2:] if size is None else size))
    if (H, W) != tuple(label.shape[-2:]):
        raise ValueError("halo_amd.training: size %s differs from the label's %s" % ((H, W), tuple(label.shape[-2:])))
    if H < h or W < w:
        raise ValueError("halo_amd.training: size %s is smaller than the logits' %s; this path upsamples only" % ((H, W), (h, w)))
    if not (cross_entropy or negative):
        raise ValueError("halo_amd.training: no term requested")
    terms = (_lib.LOSS_CE if cross_entropy else 0) | (_lib.LOSS_NL if negative else 0)
    ce, nl, sums = _UpsampledLossFn.apply(logits.contiguous(), label.contiguous(), H, W, int(ignore_index), float(negative_threshold), terms)
    if check_labels:
        bad = int(sums[BAD_LABELS].item())
        if bad:
            raise IndexError("Target out of bounds: %d label(s) outside [0, %d) that are not ignore_index %d" % (bad, K, int(ignore_index)))
    return UpsampledLosses(ce if cross_entropy else None, nl if negative else None, sums[CE_COUNT].to(torch.int64))


__all__ = ["upsampled_losses", "UpsampledLosses"]
