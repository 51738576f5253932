"""Synthetic cases for the work split of halo_dwconv.hip (dw_geom / dw_item: column groups x row chains x 16-row chain segments x
256-thread blocks), the operand recipe they share, and a pure-Python restatement of that split.  numpy only: the same operands on
any machine.  tests/test_dwconv_geometry_host.py proves under the model what each case reaches and that the operands keep the ReLU
mask away from the rounding band; tests/test_gpu_dwconv_geometry.py and tests/test_gpu_decoder_front.py run them on the device.
"""
import numpy as np

from dwconv_ref import FROZEN

DW_TPB, DW_L = 256, 16            # halo_dwconv.hip's constants (the host test reads them from the source and compares)

# name: ((B, C, H, W, d), what the split is at that shape on aligned operands:
#        gw (columns per thread: 4 = the 16-byte route, W % 4 == 0), nseg (segments per chain), items (threads with work per plane),
#        bpp (blocks per plane), empty (items whose segment starts at or below row H), last (lanes of a plane's last block that have an
#        item), work (those of them whose segment is not empty))
PLAIN = {
    "vec_d3_two_blocks": ((2, 3, 50, 176, 3), dict(gw=4, nseg=2, items=264, bpp=2, empty=44, last=8, work=0)),
    "scalar_d3_two_blocks": ((2, 3, 50, 45, 3), dict(gw=1, nseg=2, items=270, bpp=2, empty=45, last=14, work=0)),
    "scalar_d4_two_blocks": ((2, 3, 67, 41, 4), dict(gw=1, nseg=2, items=328, bpp=2, empty=41, last=72, work=31)),
    # W = 260 is a multiple of 4: aligned operands take <4, true> with one block; the one-column route at this shape (780 items,
    # 4 blocks) is reached through 4-byte-offset operands (test_gpu_dwconv_geometry.py), and by shape alone in scalar_d1_w261_four_blocks
    "scalar_d1_four_blocks": ((1, 3, 40, 260, 1), dict(gw=4, nseg=3, items=195, bpp=1, empty=0, last=195, work=195)),
    "vec_d1_five_lane_block": ((2, 3, 33, 348, 1), dict(gw=4, nseg=3, items=261, bpp=2, empty=0, last=5, work=5)),
    "vec_d1_single_group": ((2, 3, 17, 4, 1), dict(gw=4, nseg=2, items=2, bpp=1, empty=0, last=2, work=2)),
    "d6_two_segments": ((1, 3, 100, 12, 6), dict(gw=4, nseg=2, items=36, bpp=1, empty=6, last=36, work=30)),
    "one_row": ((2, 3, 1, 5, 1), dict(gw=1, nseg=1, items=5, bpp=1, empty=0, last=5, work=5)),
    "one_column": ((2, 3, 5, 1, 3), dict(gw=1, nseg=1, items=3, bpp=1, empty=0, last=3, work=3)),
    "d_beyond_plane": ((1, 3, 2, 8, 7), dict(gw=4, nseg=1, items=4, bpp=1, empty=0, last=4, work=4)),
    "one_pixel": ((1, 3, 1, 1, 1), dict(gw=1, nseg=1, items=1, bpp=1, empty=0, last=1, work=1)),
    "three_by_three": ((2, 3, 3, 3, 1), dict(gw=1, nseg=1, items=3, bpp=1, empty=0, last=3, work=3)),
    "scalar_d1_w261_four_blocks": ((1, 3, 40, 261, 1), dict(gw=1, nseg=3, items=783, bpp=4, empty=0, last=15, work=15)),
    # the second blocks of vec_d3_two_blocks and scalar_d3_two_blocks hold empty items only (the chain that is one row short comes
    # last): here <4, false> has a second block with work
    "vec_d2_working_second_block": ((1, 3, 40, 260, 2), dict(gw=4, nseg=2, items=260, bpp=2, empty=0, last=4, work=4)),
}
# the same planes through operands 4 bytes off a 16-byte boundary: the one-column route whatever W
PLAIN_OFFSET = {
    "vec_d3_two_blocks": dict(gw=1, nseg=2, items=1056, bpp=5, empty=176, last=32, work=0),
    "vec_d1_five_lane_block": dict(gw=1, nseg=3, items=1044, bpp=5, empty=0, last=20, work=20),
    "scalar_d1_four_blocks": dict(gw=1, nseg=3, items=780, bpp=4, empty=0, last=12, work=12),
}
# name: ((a's shape, s's shape), the split of the (Ca + Cs, H, W) planes at d = 1)
DECODER = {
    "vector_two_blocks": (((2, 2, 10, 70), (2, 2, 33, 348)), dict(gw=4, nseg=3, items=261, bpp=2, empty=0, last=5, work=5)),
    "scalar_four_blocks": (((1, 2, 7, 50), (1, 2, 40, 261)), dict(gw=1, nseg=3, items=783, bpp=4, empty=0, last=15, work=15)),
    "near_identity": (((1, 2, 36, 10), (1, 2, 37, 12)), dict(gw=4, nseg=3, items=9, bpp=1, empty=0, last=9, work=9)),
    "one_source_row": (((2, 2, 1, 3), (2, 2, 20, 8)), dict(gw=4, nseg=2, items=4, bpp=1, empty=0, last=4, work=4)),
    "two_source_rows": (((1, 2, 2, 2), (1, 2, 40, 4)), dict(gw=4, nseg=3, items=3, bpp=1, empty=0, last=3, work=3)),
    "single_row_plane": (((1, 2, 1, 4), (1, 2, 1, 9)), dict(gw=1, nseg=1, items=9, bpp=1, empty=0, last=9, work=9)),
}


def _quarters(rng, shape):
    return (rng.integers(-8, 9, shape) / 4).astype(np.float32)


def _norm(rng, C, dead):
    """the frozen norm's four vectors, drawn in this order: a negative weight in channel 0, a shift that leaves `dead` all-zero"""
    f32 = lambda v: v.astype(np.float32)
    weight = 0.25 + 1.5 * rng.random(C)
    weight[0] = -0.75
    bias = 0.4 * rng.standard_normal(C) + 0.1
    for c in dead:
        bias[c] = -1e4
    running_mean = 0.5 * rng.standard_normal(C) + 0.2
    running_var = 0.3 + 1.5 * rng.random(C)
    return dict(weight=f32(weight), bias=f32(bias), running_mean=f32(running_mean), running_var=f32(running_var), kind=FROZEN)


def synthetic(seed, B, C, H, W, d):
    """a case dict with the keys tests/dwconv_ref.py reads: x and g in quarter steps, the last channel dead behind the ReLU"""
    rng = np.random.default_rng(seed)
    c = dict(B=B, C=C, H=H, W=W, d=d, x=_quarters(rng, (B, C, H, W)), g=_quarters(rng, (B, C, H, W)))
    c["w"] = rng.standard_normal((C, 1, 3, 3)).astype(np.float32)
    c.update(_norm(rng, C, [C - 1]))
    return c


def plain(name):
    return synthetic(100 + list(PLAIN).index(name), *PLAIN[name][0])


def decoder(name):
    """the decoder front's operands a, s, g and a case dict without x (x = cat(resize(a), s) is the caller's: which resize is the
    point); channels Ca - 1 and C - 1 are dead"""
    (B, Ca, h, w), (_, Cs, H, W) = DECODER[name][0]
    C = Ca + Cs
    rng = np.random.default_rng(200 + list(DECODER).index(name))
    c = dict(B=B, C=C, H=H, W=W, d=1, Ca=Ca, a=_quarters(rng, (B, Ca, h, w)), s=_quarters(rng, (B, Cs, H, W)), g=_quarters(rng, (B, C, H, W)))
    c["w"] = rng.standard_normal((C, 1, 3, 3)).astype(np.float32)
    c.update(_norm(rng, C, [Ca - 1, C - 1]))
    return c


# ---------------------------------------------------------------- dw_geom / dw_item restated
def dw_geom(H, W, d, gw, L=DW_L, tpb=DW_TPB):
    cdiv = lambda a, b: -(-a // b)
    G = dict(H=H, W=W, d=d, gw=gw, L=L, tpb=tpb, ngroups=W // gw, nres=min(d, H), nseg=cdiv(cdiv(H, d), L))
    G["items"] = G["nseg"] * G["nres"] * G["ngroups"]
    G["bpp"] = cdiv(G["items"], tpb)
    return G


def dw_item(G, blk, lane):
    """(c0, i0, iend) of lane `lane` of block `blk` of a plane, or None when it has no item: its outputs are rows i0, i0 + d, ...
    below iend, columns c0 .. c0 + gw - 1"""
    item = blk * G["tpb"] + lane
    if item >= G["items"]:
        return None
    g, t = item % G["ngroups"], item // G["ngroups"]
    r, k0 = t % G["nres"], (t // G["nres"]) * G["L"]
    i0 = r + k0 * G["d"]
    return g * G["gw"], min(i0, G["H"]), min(i0 + G["L"] * G["d"], G["H"])


def split_facts(H, W, d, gw, L=DW_L, tpb=DW_TPB):
    """(the claims of the tables above, cover): cover[i, j] counts the items that write output (i, j)"""
    G = dw_geom(H, W, d, gw, L, tpb)
    cover = np.zeros((H, W), dtype=np.int64)
    empty = work = 0
    for blk in range(G["bpp"]):
        for lane in range(tpb):
            it = dw_item(G, blk, lane)
            if it is None:
                continue
            c0, i0, iend = it
            empty += i0 >= iend
            work += blk == G["bpp"] - 1 and i0 < iend
            cover[i0:iend:d, c0:c0 + gw] += 1
    facts = dict(gw=gw, nseg=G["nseg"], items=G["items"], bpp=G["bpp"], empty=int(empty), last=G["items"] - (G["bpp"] - 1) * tpb, work=int(work))
    return facts, cover
