"""HFR, the weighted normalisation of the DeepLab-v3+ hyperbolic head (core/models/classifier.py:529-550), on the device.

With cfg.MODEL.HFR the head runs, between conv_reduce and mapper.expmap,

    weights = wn_mlp(x.permute(0, 2, 3, 1).reshape(-1, C)).view(B, P, C).mean(dim=1).clamp(min=1e-5)
    y = F.normalize(x.reshape(B, C, P), dim=-1).reshape(B, C, h, w) * weights[:, :, None, None]

with wn_mlp = Sequential(Linear(C, C), BatchNorm1d(C), ReLU(), Linear(C, C)).  `weighted_normalize(x, wn_mlp)` computes it and its
gradient for x and the six parameters with halo_hfr.hip: passes over x that recompute the per-pixel MLP and never build the
permuted copy or the (B * P, C) activations.  The BatchNorm follows the module: batch statistics in training (and when no
running statistics are tracked), the running statistics otherwise, the running-stat update with `momentum` (None: the
cumulative average) and `num_batches_tracked`, `eps`, `affine`.

A torch.nn.SyncBatchNorm in training mode, in an initialised process group of more than one rank, gathers every rank's
(count, mean, M2) rows over its process_group and merges them in rank order (merge_rank_stats), so every rank normalises with
the same bits; the backward gathers the two per-channel gradient sums and adds them in rank order, as SyncBatchNorm
all-reduces them.  Parameter gradients are this rank's own, as SyncBatchNorm's are.

Anything outside the served envelope runs the stock torch statement (torch_statement), so torch's results and errors are kept
there: a dtype other than float32, autocast, CPU tensors, C > 256, a wn_mlp of any other structure, batch statistics over a
single row.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

MAX_C = 256


def torch_statement(x, wn_mlp):
    """the stock statement of the head's forward (classifier.py:529-550, as halo_amd.core.models.classifier states it)"""
    b, ch, h, w = x.shape
    weights = wn_mlp(x.permute(0, 2, 3, 1).reshape(-1, ch)).view(b, h * w, ch).mean(dim=1)
    weights = weights.clamp(min=1e-5).view(b, ch, 1, 1)
    return F.normalize(x.reshape(b, ch, h * w), dim=-1).reshape(b, ch, h, w) * weights


def _layers(wn_mlp):
    """(lin1, bn, lin2) of a served wn_mlp, else None"""
    if type(wn_mlp) is not nn.Sequential or len(wn_mlp) != 4:
        return None
    lin1, bn, act, lin2 = wn_mlp
    if type(lin1) is not nn.Linear or type(lin2) is not nn.Linear or type(act) is not nn.ReLU:
        return None
    if type(bn) not in (nn.BatchNorm1d, nn.SyncBatchNorm):
        return None
    if lin1.bias is None or lin2.bias is None:
        return None
    C = lin1.in_features
    if lin1.out_features != C or lin2.in_features != C or lin2.out_features != C or bn.num_features != C:
        return None
    return lin1, bn, lin2


def _uses_batch_stats(bn):
    return bn.training or bn.running_mean is None or bn.running_var is None


def _sync_group(bn):
    """the process group of a SyncBatchNorm that synchronises in this call, else None"""
    if type(bn) is not nn.SyncBatchNorm or not bn.training:
        return None
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) > 1 else None


def fallback_reason(x, wn_mlp):
    """why weighted_normalize(x, wn_mlp) runs the torch statement (None: the fused path serves it)"""
    layers = _layers(wn_mlp)
    if layers is None:
        return "wn_mlp is not Sequential(Linear(C, C), BatchNorm1d(C) / SyncBatchNorm(C), ReLU(), Linear(C, C))"
    lin1, bn, lin2 = layers
    if not torch.is_tensor(x) or x.dim() != 4:
        return "x is not a (B, C, h, w) tensor"
    if x.shape[1] != lin1.in_features:
        return "x has %d channels, wn_mlp %d" % (x.shape[1], lin1.in_features)
    if x.shape[1] > MAX_C:
        return "C = %d > %d" % (x.shape[1], MAX_C)
    if x.dtype != torch.float32:
        return "x is %s, not float32" % x.dtype
    if _autocast():
        return "autocast is enabled"
    if not x.is_cuda:
        return "x is not on a ROCm device"
    tensors = [lin1.weight, lin1.bias, lin2.weight, lin2.bias, bn.weight, bn.bias]
    if not _uses_batch_stats(bn) or (bn.training and bn.track_running_stats):
        tensors += [bn.running_mean, bn.running_var]
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or t.device != x.device):
            return "a wn_mlp tensor is not float32 on %s" % x.device
    if (bn.weight is None) != (bn.bias is None):
        return "BatchNorm with only one of weight and bias"
    B, C, h, w = x.shape
    if B * h * w == 0:
        return "empty input"
    if _uses_batch_stats(bn) and B * h * w * _world(bn) <= 1:
        return "batch statistics over a single row"
    return None


def _autocast():
    try:
        return torch.is_autocast_enabled() or torch.is_autocast_enabled("cpu")
    except TypeError:                       # torch without the device-type argument
        return torch.is_autocast_enabled() or torch.is_autocast_cpu_enabled()


def _world(bn):
    group = _sync_group(bn)
    if group is None:
        return 1
    import torch.distributed as dist
    return dist.get_world_size(group)


def merge_rank_stats(rows):
    """Chan's merge of per-rank (C, 3) float64 rows (count, mean, M2) in list order: the device's merge statements"""
    n, m, M2 = (v.clone() for v in rows[0].unbind(1))
    for r in rows[1:]:
        nb, mb, M2b = r.unbind(1)
        nn_ = n + nb
        d = mb - m
        m = m + d * (nb / nn_)
        M2 = M2 + M2b + d * d * (n * nb / nn_)
        n = nn_
    return torch.stack([n, m, M2], dim=1)


def sum_in_rank_order(rows):
    out = rows[0].clone()
    for r in rows[1:]:
        out = out + r
    return out


def _gather(t, group):
    import torch.distributed as dist
    rows = [torch.empty_like(t) for _ in range(dist.get_world_size(group))]
    dist.all_gather(rows, t.contiguous(), group=group)
    return rows


def _ptr(t):
    return _lib.ptr(t)


class _WeightedNormalizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W1, b1, gamma, beta, W2, b2, bn_state):
        use_batch, rmean, rvar, factor, eps, group = bn_state
        B, C, h, w = x.shape
        P = h * w
        L = _lib.lib()
        dev = x.device
        st = _lib.stream_ptr(dev)
        nws = L.halo_hfr_workspace_bytes(B, C, P)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        stats = None
        if use_batch:
            stats = torch.empty((C, 3), dtype=torch.float64, device=dev)
            _lib.check(L.halo_hfr_fwd_stats(_ptr(x), B, C, P, _ptr(W1), _ptr(b1), _ptr(stats), _ptr(ws), nws, st), "halo_hfr_fwd_stats")
            if group is not None:
                stats = merge_rank_stats(_gather(stats, group))
        y = torch.empty_like(x)
        _lib.check(L.halo_hfr_fwd_apply(_ptr(x), B, C, P, _ptr(W1), _ptr(b1), _ptr(stats), _ptr(rmean), _ptr(rvar), float(factor),
                                        float(eps), _ptr(gamma), _ptr(beta), _ptr(W2), _ptr(b2), _ptr(y), _ptr(ws), nws, st),
                   "halo_hfr_fwd_apply")
        ctx.save_for_backward(x, W1, b1, gamma, W2)
        ctx.ws, ctx.group, ctx.affine = ws, group, gamma is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, W1, b1, gamma, W2 = ctx.saved_tensors
        B, C, h, w = x.shape
        P = h * w
        dev = x.device
        L = _lib.lib()
        st = _lib.stream_ptr(dev)
        ws = ctx.ws
        nws = ws.numel()
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        gW2, gb2 = torch.empty((C, C), **f32), torch.empty(C, **f32)
        ggamma = torch.empty(C, **f32) if ctx.affine else None
        gbeta = torch.empty(C, **f32) if ctx.affine else None
        gsums = torch.empty((C, 2), dtype=torch.float64, device=dev)
        _lib.check(L.halo_hfr_bwd_reduce(_ptr(x), B, C, P, _ptr(W2), _ptr(g), _ptr(gW2), _ptr(gb2), _ptr(ggamma), _ptr(gbeta),
                                         _ptr(gsums), _ptr(ws), nws, st), "halo_hfr_bwd_reduce")
        if ctx.group is not None:
            gsums = sum_in_rank_order(_gather(gsums, ctx.group))
        gx = torch.empty_like(x)
        gW1, gb1 = torch.empty((C, C), **f32), torch.empty(C, **f32)
        _lib.check(L.halo_hfr_bwd_apply(_ptr(x), B, C, P, _ptr(W1), _ptr(b1), _ptr(gamma), _ptr(g), _ptr(gsums), _ptr(gx), _ptr(gW1),
                                        _ptr(gb1), _ptr(ws), nws, st), "halo_hfr_bwd_apply")
        return gx, gW1, gb1, ggamma, gbeta, gW2, gb2, None


def weighted_normalize(x, wn_mlp):
    """The head's HFR statement: F.normalize(x over pixels) * clamp(mean_p wn_mlp(x_p), min=1e-5), x (B, C, h, w).
    Differentiable w.r.t. x and the parameters of wn_mlp; updates the BatchNorm's running statistics as the module would.
    Outside the served envelope (fallback_reason) it returns torch_statement(x, wn_mlp)."""
    if fallback_reason(x, wn_mlp) is not None:
        return torch_statement(x, wn_mlp)
    lin1, bn, lin2 = _layers(wn_mlp)
    use_batch = _uses_batch_stats(bn)
    update = bn.training and bn.track_running_stats and bn.running_mean is not None
    factor = 0.0
    if update:
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        factor = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
    if use_batch:
        rmean, rvar = (bn.running_mean, bn.running_var) if update else (None, None)
    else:
        rmean, rvar = bn.running_mean, bn.running_var
    state = (use_batch, rmean, rvar, factor, bn.eps, _sync_group(bn) if use_batch else None)
    return _WeightedNormalizeFn.apply(x.contiguous(), lin1.weight.contiguous(), lin1.bias.contiguous(),
                                      None if bn.weight is None else bn.weight.contiguous(),
                                      None if bn.bias is None else bn.bias.contiguous(),
                                      lin2.weight.contiguous(), lin2.bias.contiguous(), state)


__all__ = ["weighted_normalize", "torch_statement", "fallback_reason", "merge_rank_stats"]
