"""CPU checks behind tests/test_gpu_dwconv_geometry.py and the synthetic cases of tests/test_gpu_decoder_front.py:

  * under a Python restatement of dw_geom / dw_item (tests/dwconv_cases.py) every output element of every case belongs to exactly
    one item, and the case has the block, segment, empty-item and last-block lane counts its table entry claims -- with DW_L and
    DW_TPB read from halo_dwconv.hip, so a change to either fails here;
  * the yardstick tests/dwconv_ref.py holds a correct float32 chain (torch's CPU conv -> FrozenBatchNorm2d -> relu and its
    autograd) inside its bounds 15u / 15u / 8u at every synthetic case;
  * the operands keep the ReLU's argument out of 4 x the forward bound for all but 1e-4 of the elements, so the device tests' cap
    on the band |pre64| <= bound is a property of the inputs;
  * adjoint64 (the resize backward with the float32 taps in exact arithmetic, tests/resize_ref.py), which the decoder-front test
    uses for g_a, agrees with the float32 numpy statement of the adjoint within 2 (n + 8) u adjoint64(|g|).
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import dwconv_cases as K
import dwconv_ref as R
import resize_ref as Z

U = R.U
BAND_CAP = 1e-4


def test_model_constants_are_the_kernel_files():
    text = open(os.path.join(ROOT, "halo_amd", "csrc", "halo_dwconv.hip")).read()
    assert int(re.search(r"constexpr int DW_TPB = (\d+);", text).group(1)) == K.DW_TPB
    assert int(re.search(r"constexpr int DW_L = (\d+);", text).group(1)) == K.DW_L


def _splits():
    for name, ((B, C, H, W, d), claim) in K.PLAIN.items():
        yield "plain-" + name, H, W, d, claim
        assert claim["gw"] == (4 if W % 4 == 0 else 1), name                 # aligned operands: the route is W's alone
    for name, claim in K.PLAIN_OFFSET.items():
        _, _, H, W, d = K.PLAIN[name][0]
        yield "offset-" + name, H, W, d, claim
    for name, ((_, (_, _, H, W)), claim) in K.DECODER.items():
        yield "decoder-" + name, H, W, 1, claim
        assert claim["gw"] == (4 if W % 4 == 0 else 1), name


@pytest.mark.parametrize("tag,H,W,d,claim", list(_splits()), ids=[s[0] for s in _splits()])
def test_every_output_belongs_to_one_item_and_the_case_reaches_what_it_claims(tag, H, W, d, claim):
    facts, cover = K.split_facts(H, W, d, claim["gw"])
    assert (cover == 1).all(), (tag, int(cover.min()), int(cover.max()))
    assert facts == claim, (tag, facts)


def test_the_table_reaches_every_property_it_is_there_for():
    """the properties of the work split that no small case reached before, each by at least one case, by route"""
    rows = [(s[4], c) for s, c in K.PLAIN.values()] + [(K.PLAIN[n][0][4], c) for n, c in K.PLAIN_OFFSET.items()]
    for gw, d1 in ((4, True), (4, False), (1, True), (1, False)):                     # <4,true>, <4,false>, <1,false> at d = 1 and d > 1
        assert any(c["gw"] == gw and (d == 1) == d1 and c["bpp"] > 1 and c["work"] > 0 for d, c in rows), (gw, d1)   # a last block with work
    for gw in (4, 1):
        assert any(c["gw"] == gw and d > 1 and c["nseg"] > 1 and c["empty"] > 0 for d, c in rows), gw
        assert any(c["gw"] == gw and c["bpp"] > 1 and 0 < c["work"] <= c["last"] < 64 for d, c in rows), gw      # ... of less than a wave
        assert any(c["gw"] == gw and c["bpp"] > 1 for _, c in K.DECODER.values()), gw
    shapes = [s[2:] for s, _ in K.PLAIN.values()]
    assert any(H == 1 and W > 1 for H, W, _ in shapes) and any(W == 1 and H > 1 for H, W, _ in shapes) and (1, 1, 1) in shapes
    assert any(W == 4 and d == 1 for _, W, d in shapes) and any(d > H for H, _, d in shapes) and any(d > W for _, W, d in shapes)
    hs = [(a[2], s[2]) for (a, s), _ in K.DECODER.values()]
    assert any(h == 1 and H > K.DW_L for h, H in hs) and any(h == 2 and H > 2 * K.DW_L for h, H in hs) and any(h == H - 1 for h, H in hs)
    assert any(H == 1 for _, H in hs)


def test_workspace_covers_the_route_with_more_blocks():
    """halo_dwconv_workspace_bytes is sized for whichever route the pointers select: b1 > b4 >= 1 at the offset cases"""
    from halo_amd import _lib
    L = _lib.lib()
    for name, off in K.PLAIN_OFFSET.items():
        (B, C, H, W, d), claim = K.PLAIN[name]
        assert off["bpp"] > claim["bpp"]
        assert L.halo_dwconv_workspace_bytes(B, C, H, W, d) == B * C * off["bpp"] * 9 * 8
    for (B, C, H, W, d), claim in K.PLAIN.values():
        assert L.halo_dwconv_workspace_bytes(B, C, H, W, d) == B * C * K.dw_geom(H, W, d, 1)["bpp"] * 9 * 8 >= B * C * claim["bpp"] * 72


def test_the_recipe_is_seeded_and_in_quarter_steps():
    a, b = K.plain("scalar_d3_two_blocks"), K.plain("scalar_d3_two_blocks")
    assert all(np.array_equal(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))
    for k in ("x", "g"):
        assert a[k].dtype == np.float32 and np.array_equal(a[k] * 4, np.round(a[k] * 4)) and np.abs(a[k]).max() == 2.0
    assert a["weight"][0] == np.float32(-0.75) and a["bias"][-1] == np.float32(-1e4) and a["kind"] == R.FROZEN
    c = K.decoder("vector_two_blocks")
    assert c["bias"][c["Ca"] - 1] == np.float32(-1e4) and c["bias"][-1] == np.float32(-1e4) and c["a"].shape == (2, 2, 10, 70)


def _ratio(err, bound):
    assert (err[bound == 0] == 0).all()                                         # exactly 0 where the bound is 0
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("name", list(K.PLAIN))
def test_yardstick_holds_torch_cpu_float32(name):
    """a correct float32 evaluation in another order of summation sits inside the three bounds, with its own mask"""
    c = K.plain(name)
    conv, bn = R.modules(c)
    x = torch.from_numpy(c["x"]).requires_grad_(True)
    y = torch.relu(bn(conv(x)))
    gx, gw = torch.autograd.grad(y, [x, conv.weight], torch.from_numpy(c["g"]))
    y, gx, gw = (t.detach().numpy().astype(np.float64) for t in (y, gx, gw))
    pre, bound = R.forward(c)
    rf = _ratio(np.abs(y - np.maximum(pre, 0)), bound)
    mask = y > 0
    band = np.abs(pre) <= bound
    assert (mask == (pre > 0))[~band].all()
    rx, bx = R.grad_x(c, mask)
    rw, bw = R.grad_w(c, mask)
    rgx, rgw = _ratio(np.abs(gx - rx), bx), _ratio(np.abs(gw - rw), bw)
    print("%s: max err / bound forward %.3f, g_x %.3f, g_w %.3f" % (name, rf, rgx, rgw))
    assert rf <= 1 and rgx <= 1 and rgw <= 1
    dead = c["C"] - 1
    assert (bx[:, dead] == 0).all() and (bw[dead] == 0).all() and (y[:, dead] == 0).all()


def _band_counts(tag, pre, bound):
    n1, n4 = int((np.abs(pre) <= bound).sum()), int((np.abs(pre) <= 4 * bound).sum())
    print("%s: %d of %d elements within the bound of zero, %d within 4 x" % (tag, n1, pre.size, n4))
    assert n4 <= BAND_CAP * pre.size, (tag, n4, pre.size)
    return n1, n4


@pytest.mark.parametrize("name", list(K.PLAIN))
def test_plain_operands_stay_out_of_the_band(name):
    c = K.plain(name)
    pre, bound = R.forward(c)
    _band_counts(name, pre, bound)
    assert (pre[:, c["C"] - 1] < -4 * bound[:, c["C"] - 1]).all()                # the dead channel is dead on any correct device


def decoder_case64(name):
    """the decoder case with x = cat(Ay a Ax^T, s) in float64 (the float32 taps, exact products and sums)"""
    c = K.decoder(name)
    c["x"] = np.concatenate([Z.resize64(c["a"], c["H"], c["W"]), c["s"].astype(np.float64)], 1)
    return c


@pytest.mark.parametrize("name", list(K.DECODER))
def test_decoder_operands_stay_out_of_the_band(name):
    """the device's x differs from this one by the three roundings of a bilerp, 3u |x| <= 6u: a shift of pre far inside the 4 x
    margin (the forward bound is 15u (|scale| sum |w||x| + ...)).  Channels 0 and Ca fire somewhere, Ca - 1 and C - 1 nowhere:
    what test_bits_of_the_composition asserts of y."""
    c = decoder_case64(name)
    pre, bound = R.forward(c)
    _band_counts(name, pre, bound)
    Ca, C = c["Ca"], c["C"]
    for dead in (Ca - 1, C - 1):
        assert (pre[:, dead] < -4 * bound[:, dead]).all()
    for live in (0, Ca):
        assert (pre[:, live] > 4 * bound[:, live]).any()


@pytest.mark.parametrize("name", list(K.DECODER))
def test_adjoint64_against_the_float32_adjoint(name):
    (_, _, h, w), (_, _, H, W) = K.DECODER[name][0]
    rng = np.random.default_rng(300 + list(K.DECODER).index(name))
    g = rng.standard_normal((2, H, W)).astype(np.float32)
    got = Z.numpy_adjoint(g, h, w).astype(np.float64)
    want = Z.adjoint64(g, h, w)
    bound = 2 * (Z.terms_bound(h, w, H, W) + 8) * U * Z.adjoint64(np.abs(g), h, w)
    r = _ratio(np.abs(got - want), bound)
    print("%s: %dx%d <- %dx%d, max err / bound %.3g" % (name, h, w, H, W, r))
    assert r <= 1
    assert abs(float(Z.adjoint64(np.ones((1, H, W)), h, w).sum()) - H * W) <= 1e-6 * H * W       # the weights of an output sum to 1
