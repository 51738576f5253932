"""Cases for the multi-dilation depthwise passes (halo_multi_dwconv3x3_* of halo_dwconv.hip, halo_amd.dwconv.multi_depthwise_bn_relu):
N dilations over one input, a plane held in LDS.  Operands come from tests/dwconv_cases.py's recipe (quarter steps, a negative norm
weight in channel 0, a dead last channel); x is shared, the gradient, the weights and the norm are drawn per dilation.  numpy only.
tests/test_dwmulti_host.py and tests/test_gpu_dwmulti.py use them."""
import numpy as np

from dwconv_cases import synthetic

# name: ((B, C, H, W, dilations), what the shape reaches)
CASES = {
    "head_dilations": ((2, 3, 40, 44, (6, 12, 18)), "the head's dilations, B > 1 and C > 1 with B != C, 16-byte route"),
    "odd_plane": ((2, 3, 13, 79, (1, 2, 5)), "HW = 1027: ragged last trip of the staging loop and of the item loop"),
    "two_segments": ((1, 3, 100, 12, (6, 1, 3)), "two 16-row segments in a chain; d = 1 mixed with d > 1"),
    "one_pixel": ((1, 3, 1, 1, (1, 2, 3)), "one pixel"),
    "one_row": ((2, 3, 1, 5, (1, 2, 3)), "one row"),
    "one_column": ((2, 3, 5, 1, (3, 1, 2)), "one column"),
    "d_beyond_plane": ((1, 3, 2, 8, (7, 9, 1)), "d beyond H and W: centre tap only"),
    "two_dilations": ((2, 3, 17, 4, (1, 3)), "N = 2"),
    "four_dilations": ((1, 3, 33, 20, (1, 6, 12, 18)), "N = 4"),
    "unsorted_repeated": ((1, 3, 20, 24, (12, 6, 12)), "list order is not sorted order; a repeated d with different weights"),
    "target_plane": ((1, 2, 80, 160, (6, 12, 18)), "the head's plane at the target crop, two channels"),
    "source_plane": ((1, 2, 90, 160, (6, 12, 18)), "the head's plane at the source crop, two channels"),
}
# the same planes through operands 4 bytes off a 16-byte boundary: the one-element route at a W % 4 == 0 shape
OFFSET = ("head_dilations",)
FLOAT64 = ("head_dilations", "two_segments")       # the first and third cases: an independent float64 check of g_x


def case(name):
    """a list of dwconv_ref case dicts, one per dilation, that share x"""
    return build(100 + list(CASES).index(name), *CASES[name][0])


def build(seed, B, C, H, W, dilations):
    out = []
    for i, d in enumerate(dilations):
        c = synthetic(1000 * seed + i, B, C, H, W, d)
        if out:
            c["x"] = out[0]["x"]
        out.append(c)
    return out


def edge_shapes(max_plane):
    """((1, 2, H, W) with H * W == max_plane, the same with one row more): the widest W <= 256 that divides the limit"""
    W = max(w for w in range(1, 257) if max_plane % w == 0)
    H = max_plane // W
    return (1, 2, H, W), (1, 2, H + 1, W)


def f32_sum_bound(gx64, bounds):
    """the bound of a float32 sum of N float32 terms in any order against the float64 sum of their exact values: each term's own
    bound, plus (N - 1) u times the magnitudes that pass through the adds"""
    U = 2.0 ** -24
    n = len(gx64)
    return sum(bounds) + (n - 1) * U * sum(np.abs(g) + b for g, b in zip(gx64, bounds))
