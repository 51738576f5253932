"""The numeric contract of halo_amd.norm.norm_relu_maxpool (halo_maxpool.hip) restated in plain torch on the CPU, shared by
tests/test_stem_pool_host.py (which holds it to torch's CPU autograd of the stock statements) and tests/test_gpu_stem_pool.py
(which holds the kernels to it):

    z          = relu(fl(fl(x scale[c]) + shift[c]))                    NaN stays NaN
    out[oh,ow] = z at the recorded tap of the window rows 2oh-1 .. 2oh+1, columns 2ow-1 .. 2ow+1 (taps inside the map only),
                 scanned row-major from -inf; a tap is taken if v > max or v is NaN: the first of equal values, the last NaN
    tap[oh,ow] = 3 kh + kw of the recorded tap, or BLOCKED (9) when its z <= 0
    g_x[h,w]   = fl(S scale[c]);  S = the float32 sum of g[oh,ow] over the windows whose recorded tap is (h, w), added in
                 ascending oh, then ascending ow, from +0, and replaced by +0 where z <= 0 (a NaN z lets it through)
"""
import torch

BLOCKED = 9


def out_size(n):
    return (n - 1) // 2 + 1


def stem_pool_ref(x, scale, shift, g=None):
    """x (B, C, H, W), scale, shift (C), g (B, C, OH, OW) or None, float32 on the CPU.  Returns a dict: `out` (B, C, OH, OW)
    float32, `index` (B, C, OH, OW) int64, the recorded tap as h * W + w (nn.MaxPool2d's return_indices), `tap` (B, C, OH, OW) uint8,
    and with g also `g_x` (B, C, H, W) float32."""
    x, scale, shift = x.detach().cpu().float(), scale.detach().cpu().float(), shift.detach().cpu().float()
    B, C, H, W = x.shape
    OH, OW = out_size(H), out_size(W)
    pre = x * scale.view(1, C, 1, 1)
    pre = pre + shift.view(1, C, 1, 1)
    z = torch.where(pre <= 0, torch.zeros_like(pre), pre)
    flat = z.reshape(B, C, H * W)
    oh = torch.arange(OH).view(OH, 1).expand(OH, OW)
    ow = torch.arange(OW).view(1, OW).expand(OH, OW)
    best = torch.full((B, C, OH, OW), float("-inf"))
    index = ((2 * oh - 1).clamp(min=0) * W + (2 * ow - 1).clamp(min=0)).expand(B, C, OH, OW).clone()      # ATen: the window's first tap
    code = torch.zeros((B, C, OH, OW), dtype=torch.int64)
    for kh in range(3):
        for kw in range(3):
            h, w = 2 * oh - 1 + kh, 2 * ow - 1 + kw
            inside = (h >= 0) & (h < H) & (w >= 0) & (w < W)
            at = (h.clamp(0, H - 1) * W + w.clamp(0, W - 1)).reshape(1, 1, OH * OW).expand(B, C, OH * OW)
            v = flat.gather(2, at).view(B, C, OH, OW)
            take = inside & ((v > best) | v.isnan())
            best = torch.where(take, v, best)
            index = torch.where(take, at.view(B, C, OH, OW), index)
            code = torch.where(take, torch.full_like(code, 3 * kh + kw), code)
    res = {"out": best, "index": index, "tap": torch.where(best <= 0, torch.full_like(code, BLOCKED), code).to(torch.uint8)}
    if g is not None:
        g = g.detach().cpu().float()
        S = torch.zeros(B * C, H * W)
        rows = torch.arange(B * C)
        idx, gg = index.view(B * C, OH, OW), g.reshape(B * C, OH, OW)
        for i in range(OH):                                    # ascending oh, then ascending ow: the order of the sums
            for j in range(OW):
                S[rows, idx[:, i, j]] = S[rows, idx[:, i, j]] + gg[:, i, j]
        S = torch.where(z <= 0, torch.zeros_like(z), S.view(B, C, H, W))
        res["g_x"] = S * scale.view(1, C, 1, 1)
    return res


def make_norm(C, seed):
    """a stand-in FrozenBatchNorm2d: channel 0 has scale = -2, shift = +1, channel 1 scale = +2, shift = -1 (x = 0.5 gives pre == 0 in
    both), the rest random with both signs"""
    import norm_ref as N
    from dwconv_ref import FrozenBatchNorm2d
    bn = N.randomize_norms(FrozenBatchNorm2d(C), seed)
    with torch.no_grad():
        bn.weight[0], bn.running_var[0], bn.bias[0], bn.running_mean[0] = -2.0, 1.0, 1.0, 0.0
        if C > 1:
            bn.weight[1], bn.running_var[1], bn.bias[1], bn.running_mean[1] = 2.0, 1.0, -1.0, 0.0
    return bn


def make_case(shape, seed):
    """(x, g) on the CPU for make_norm's statistics.  x: half-integers in [-2, 2], so equal values meet in most windows; NaN, +-inf,
    -0.0 and 0.5 (pre == 0 in channels 0 and 1) sprinkled over it; and, where the map is large enough (planted(shape)):
    a window of channel 0 whose pre is negative everywhere; in channel 1 a window whose first tap and centre tie at the positive
    maximum; in the last plane a window with two NaNs.  g: normal with a fifth of its elements zero."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, shape, generator=gen).float() / 2
    n = x.numel()
    k = min(n // 3, 28)
    if k:
        x.view(-1)[torch.randperm(n, generator=gen)[:k]] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.5, 0.5, 0.5] * 4)[:k]
    if planted(shape):
        x[0, 0, 0:2, 0:2] = 1.0                                # window (0, 0) of channel 0: pre = -1 at its four taps
        x[0, 1, 1:4, 1:4] = 0.0                                # window (1, 1) of channel 1: first tap (1, 1) and centre (2, 2) at 2.0
        x[0, 1, 1, 1] = x[0, 1, 2, 2] = 2.0
        top = 2 * (out_size(H) - 1)
        x[B - 1, C - 1, top - 1:top + 2, 0:2] = 0.0            # window (OH - 1, 0) of the last plane: two NaNs in its middle row
        x[B - 1, C - 1, top, 0] = x[B - 1, C - 1, top, 1] = float("nan")
    g = torch.randn((B, C, out_size(H), out_size(W)), generator=gen)
    g[torch.rand(g.shape, generator=gen) < 0.2] = 0.0
    return x, g


def planted(shape):
    return shape[1] >= 2 and shape[2] >= 5 and shape[3] >= 5
