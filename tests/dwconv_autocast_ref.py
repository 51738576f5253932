"""The statements of the depthwise half under torch.autocast (halo_half_dwconv3x3_* of halo_dwconv.hip, include/halo_hip.h), in torch
on the CPU with the nine-term sums in float64, and the EXCUSE of every summed element.

h() = `.float().to(dtype)`, round to nearest even to the autocast dtype; u = 2^-24.

    xh = h(x);  wh = h(w);  c16 = h(sum_k wh[k] xh[tap k])
    pre = fl(fl(float(c16) scale) + shift);  y32 = relu(pre);  y16 = h(y32)
    gp = y16 > 0 ? fl(float(g16) scale) : 0;  gc16 = h(gp)
    g_x = h(sum_k wh[k] gc16[p - k d])  in x's dtype;  g_w = float(h(fl32(sum_{b,p} float(gc16) float(xh[p + k d]))))

The device adds the nine terms in float32 (eight fmas), so its sum lies within 9u sum|wh||operand| of the float64 sum, and its half
can differ from h(float64 sum) only where that sum lies as close to the midpoint between two neighbouring halves: there an element
is excused and has two candidates, the rest of the chain applied exactly to either neighbour.  g_w's float64 partials are rounded
to float32 once: 8u sum|gc16||xh| (tests/dwconv_ref.py's bound) covers that rounding and the order of the float64 adds.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

U = 2.0 ** -24
HALVES = [torch.float16, torch.bfloat16]
_TOP = {torch.float16: (0x7c00, 2.0 ** 16), torch.bfloat16: (0x7f80, 2.0 ** 128)}    # the bits of inf, and the value one step past the largest finite


def h(t, dt):
    return t.float().to(dt)


def _neighbour(r, up):
    """the next half above (up) or below r; r itself where there is none (past an infinity, a NaN)"""
    inf_bits, _ = _TOP[r.dtype]
    b = r.view(torch.int16).to(torch.int32) & 0xffff
    mag = b & 0x7fff
    order = torch.where(b >= 0x8000, -mag, mag) + (1 if up else -1)
    nmag = order.abs()
    nb = torch.where(order < 0, nmag | 0x8000, nmag)
    nb = torch.where((mag > inf_bits) | (nmag > inf_bits), b, nb)
    return ((nb ^ 0x8000) - 0x8000).to(torch.int16).view(r.dtype)


def _value(r):
    """a half's float64 value, +-inf standing one step past the largest finite half (the rounding boundary of the overflow)"""
    v = r.double()
    return torch.where(torch.isinf(v), torch.sign(v) * _TOP[r.dtype][1], v)


def round_with_excuse(s, tol, dt):
    """(r, alt, excused): r = h(s); excused where s lies within tol of the midpoint between r and a neighbouring half, alt that
    neighbour there (r elsewhere).  Where the sum cancels so far that both midpoints lie within tol, the nearer one counts: the two
    candidates are always the two halves that s lies between"""
    r = h(s, dt)
    up, down = _neighbour(r, True), _neighbour(r, False)
    to_up, to_down = (s - (_value(r) + _value(up)) / 2).abs(), (s - (_value(r) + _value(down)) / 2).abs()
    near_up, near_down = (to_up <= tol) & (up != r), (to_down <= tol) & (down != r)
    alt = torch.where(near_up & ~(near_down & (to_down < to_up)), up, torch.where(near_down, down, r))
    return r, alt, near_up | near_down


def _v(t):
    return t.reshape(1, -1, 1, 1)


def _tail(c16, scale, shift, dt):
    pre = c16.float() * _v(scale) + _v(shift)
    y32 = torch.where(pre <= 0, torch.zeros((), dtype=torch.float32), pre)          # a NaN stays a NaN
    return y32, y32.to(dt)


def forward(x, w, scale, shift, d, dt):
    """x (B, C, H, W) float32 or dt, w (C, 1, 3, 3), scale, shift (C) float32 -> c16, y32, y16, and for the excused elements
    (`excused`) the other candidate `y16_alt` (y16 elsewhere)"""
    C = x.shape[1]
    xh, wh = h(x, dt).double(), h(w, dt).double()
    s = F.conv2d(xh, wh, None, 1, d, d, C)
    mag = F.conv2d(xh.abs(), wh.abs(), None, 1, d, d, C)
    c16, c_alt, excused = round_with_excuse(s, 9 * U * mag, dt)
    y32, y16 = _tail(c16, scale, shift, dt)
    return SimpleNamespace(c16=c16, y32=y32, y16=y16, y16_alt=_tail(c_alt, scale, shift, dt)[1], excused=excused, sum=s, mag=mag)


def gated(g16, gate16, scale, dt):
    """gc16 = h(gate16 > 0 ? fl(float(g16) scale) : 0)"""
    gp = torch.where(gate16.float() > 0, g16.float() * _v(scale), torch.zeros((), dtype=torch.float32))
    return gp.to(dt)


def backward(g16, gate16, x, w, scale, d, dt):
    """the gradients for the gate tensor given (the restatement's y16, or the device's own): g_x in x's dtype and g_w float32,
    each with its other candidate and its excuse"""
    C = x.shape[1]
    xh, wh = h(x, dt).double(), h(w, dt).double()
    gc = gated(g16, gate16, scale, dt).double()
    s = torch.nn.grad.conv2d_input(x.shape, wh, gc, 1, d, d, C)
    mag = torch.nn.grad.conv2d_input(x.shape, wh.abs(), gc.abs(), 1, d, d, C)
    gx, gx_alt, gx_exc = round_with_excuse(s, 9 * U * mag, dt)
    sw = torch.nn.grad.conv2d_weight(xh, w.shape, gc, 1, d, d, C)
    magw = torch.nn.grad.conv2d_weight(xh.abs(), w.shape, gc.abs(), 1, d, d, C)
    gw, gw_alt, gw_exc = round_with_excuse(sw, 8 * U * magw, dt)
    return SimpleNamespace(g_x=gx.to(x.dtype), g_x_alt=gx_alt.to(x.dtype), gx_excused=gx_exc, g_w=gw.float(), g_w_alt=gw_alt.float(),
                           gw_excused=gw_exc, gc16=gc.float().to(dt))


def same(a, b):
    """elementwise equality that takes two NaNs for equal (and -0 for 0, as torch.equal does)"""
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def matches(got, want, alt, excused):
    """every element equals the restatement, an excused one either candidate"""
    return bool((same(got, want) | (excused & same(got, alt))).all())


# ---------------------------------------------------------------- operands
def modules(w, scale, shift, d, device="cpu"):
    """(conv, bn): a depthwise conv with weight w and a FrozenBatchNorm2d whose statements give exactly scale and shift (variance 1,
    mean 0)"""
    import torch.nn as nn
    from dwconv_ref import FrozenBatchNorm2d
    C = w.shape[0]
    conv = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False)
    bn = FrozenBatchNorm2d(C)
    with torch.no_grad():
        conv.weight.copy_(w)
        bn.weight.copy_(scale)
        bn.bias.copy_(shift)
    return conv.to(device), bn.to(device)


def exact_case(seed, B, C, H, W, d):
    """small integers, power-of-two scales, integer shifts: every sum is exact in float32 and below 256, bfloat16's exact-integer
    range (|c16| <= 9 * 2 * 4 = 72, |y32| <= 146, |g_x| <= 9 * 2 * 6)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, C, H, W), generator=gen).float()
    w = torch.randint(-2, 3, (C, 1, 3, 3), generator=gen).float()
    g = torch.randint(-3, 4, (B, C, H, W), generator=gen).float()
    scale = torch.tensor([0.5, 1.0, 2.0, 0.25])[torch.arange(C) % 4]
    shift = torch.tensor([1.0, -2.0, 0.0, 3.0])[torch.arange(C) % 4]
    return x, w, g, scale, shift


def random_case(seed, B, C, H, W, d):
    """normal x, w, g around positive means, so that the nine-term sums cancel little and few of them fall into the rounding band
    of a half (tests/test_dwconv_autocast_host.py counts them); the shift centres pre on the ReLU's edge: both sides of the gate
    in every channel but the last, which is dead; channel 0 has a negative scale"""
    gen = torch.Generator().manual_seed(seed)
    x = 1.0 + 0.5 * torch.randn(B, C, H, W, generator=gen)
    w = 0.25 + 0.3 * torch.randn(C, 1, 3, 3, generator=gen)
    g = 1.0 + 0.5 * torch.randn(B, C, H, W, generator=gen)
    scale = 0.5 + torch.rand(C, generator=gen)
    scale[0] = -0.75
    shift = -scale * w.sum((1, 2, 3)) + 0.1 * torch.randn(C, generator=gen)
    shift[C - 1] = -1e4
    return x, w, g, scale, shift


# the random tier of tests/test_gpu_dwconv_autocast.py: names of tests/dwconv_cases.PLAIN and the seed of each (chosen so that at most
# 1 % of a case's elements are excused, for both dtypes: test_dwconv_autocast_host.py asserts it from the float64 evaluation alone)
RANDOM_TIER = {"vec_d3_two_blocks": 1, "scalar_d4_two_blocks": 1, "vec_d1_five_lane_block": 2, "d6_two_segments": 1, "d_beyond_plane": 1,
               "one_pixel": 1}
