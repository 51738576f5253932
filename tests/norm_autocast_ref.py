"""The statements of halo_amd.norm.norm_relu_autocast (halo_norm_autocast.hip) as torch ops, one rounding each, on any device: the
restatement that tests/test_norm_autocast_host.py holds to torch.autocast + autograd on the CPU.  Built on tests/norm_ref.py, whose
stand-ins and comparisons the autocast tests share."""
import torch

from norm_ref import same_bits, stock_chain  # noqa: F401  (re-exported for the two test files)


def scale_shift(bn):
    """FrozenBatchNorm2d.forward's two statements: (scale, shift), float32 (C,)"""
    with torch.no_grad():
        scale = bn.weight * bn.running_var.rsqrt()
        return scale, bn.bias - bn.running_mean * scale


def _per_channel(v):
    return v.reshape(1, -1, 1, 1)


def forward(x, bn, residual=None, residual_bn=None):
    """(s, y32, y16) of a half x: pre = fl(fl(float(x) scale) + shift); id = r32 or fl(fl(float(r16) r_scale) + r_shift);
    s = pre or fl(pre + id); y32 = s <= 0 ? 0 : s (a NaN stays); y16 = rne_half(y32)"""
    scale, shift = scale_shift(bn)
    s = x.float() * _per_channel(scale)
    s = s + _per_channel(shift)
    if residual is not None:
        if residual_bn is None:
            ident = residual
        else:
            r_scale, r_shift = scale_shift(residual_bn)
            ident = residual.float() * _per_channel(r_scale)
            ident = ident + _per_channel(r_shift)
        s = s + ident
    y32 = torch.where(s <= 0, torch.zeros_like(s), s)
    return s, y32, y32.to(x.dtype)


def backward(s, bn, residual_bn, half, g32=None, g16=None):
    """(g_x, g_r): g = g32, float(g16) or fl(g32 + float(g16)); gp = s <= 0 ? 0 : g (a NaN s lets g through);
    g_x = rne_half(fl(gp scale)); g_r = gp, or rne_half(fl(gp r_scale)) with a residual_bn"""
    if g32 is None:
        g = g16.float()
    elif g16 is None:
        g = g32
    else:
        g = g32 + g16.float()
    gp = torch.where(s <= 0, torch.zeros_like(g), g)
    g_x = (gp * _per_channel(scale_shift(bn)[0])).to(half)
    if residual_bn is None:
        return g_x, gp
    return g_x, (gp * _per_channel(scale_shift(residual_bn)[0])).to(half)
