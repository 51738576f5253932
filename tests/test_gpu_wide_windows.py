"""The LDS-tiled wide-window kernels (k_box_unc_tiled, k_region_impurity_tiled: odd windows from 5 x 5 to the module's default
33 x 33) on a real MI355X, bit for bit against the CPU oracle.  Every test first asserts that its configuration is on the tiled
route (floating_region.window_route, which asks the function the launchers branch on), then compares.

Shapes: 70 x 130 has several tiles each way for both kernels' tile shapes (64 x 32 pixels for the box sum, 256 x 16 for the
histogram), ragged in both directions, and a 33 x 33 window there spans three tiles; the small maps are narrower or lower than
the window; 40 x 72 is the smallest map on which reflect (pad < n) and circular (pad <= n) padding are defined at 33 x 33.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PADS = ("reflect", "replicate", "circular")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a == b) | both_nan))


def tiled(what, k, pad="zeros", bins=19, shape=None):
    from halo_amd.core.active.floating_region import window_route
    return window_route(what, k, pad, bins, shape) == "tiled"


def inputs(B, O, H, W, C, seed):
    """logits with smooth regions (a few classes per window) plus noise, a small embedding, labels with ignore pixels"""
    rng = np.random.default_rng(seed)
    coarse = rng.standard_normal((B, O, -(-H // 8), -(-W // 8))).astype(np.float32) * 3
    logit = np.kron(coarse, np.ones((1, 1, 8, 8), np.float32))[:, :, :H, :W] + rng.standard_normal((B, O, H, W)).astype(np.float32) * 0.7
    emb = rng.standard_normal((B, C, H, W)) * rng.uniform(0.01, 0.5, (B, 1, H, W))
    gt = rng.integers(0, O, (B, H, W)).astype(np.int64)
    gt[rng.random((B, H, W)) < 0.05] = 255
    return np.ascontiguousarray(logit), emb, gt


def check_score(dev, logit, emb, gt, unc, pur, norm, k, pad="zeros"):
    from halo_amd.core.active.floating_region import score_maps
    from oracle import halo_oracle as ho
    with torch.no_grad():
        s, i, u = score_maps(t(logit, dev), t(emb, dev), unc, pur, norm, t(gt, dev), size=k, padding_mode=pad)
    for b in range(logit.shape[0]):
        so, io, uo = ho.floating_region_score(logit[b], emb[b], unc, pur, norm, gt[b], size=k, purity_type=pur, padding_mode=pad)
        tag = (unc, pur, norm, k, pad, b)
        assert bits_equal(u[b].cpu().numpy(), uo), ("uncertainty",) + tag
        assert bits_equal(i[b].cpu().numpy(), io), ("impurity",) + tag
        assert bits_equal(s[b].cpu().numpy(), so), ("score",) + tag


@pytest.fixture(scope="module")
def maps70():
    return inputs(2, 19, 70, 130, 6, 70)


@pytest.mark.parametrize("k", [5, 9, 17, 33])
def test_full_score_zero_padding(dev, maps70, k):
    logit, emb, gt = maps70
    assert tiled("box", k, shape=(70, 130)) and tiled("hist", k, shape=(70, 130))
    for unc, pur in (("entropy", "ripu"), ("oracle_acc", "oracle_ripu"), ("entropy", "radius")):
        for norm in (True, False):
            check_score(dev, logit, emb, gt, unc, pur, norm, k)


@pytest.mark.parametrize("H,W,k", [(20, 150, 33), (150, 20, 33), (9, 9, 17), (1, 40, 5)])
def test_image_smaller_than_the_window(dev, H, W, k):
    assert tiled("box", k, shape=(H, W)) and tiled("hist", k, shape=(H, W))
    logit, emb, gt = inputs(1, 19, H, W, 4, H * 1000 + W)
    for norm in (True, False):
        check_score(dev, logit, emb, gt, "entropy", "ripu", norm, k)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("k", [5, 33])
def test_nonzero_padding_modes(dev, pad, k):
    from halo_amd.core.active.floating_region import FloatingRegionScore
    from oracle import halo_oracle as ho
    H, W, O = 40, 72, 19
    assert tiled("box", k, pad, shape=(H, W)) and tiled("hist", k, pad, O, (H, W))
    logit, emb, gt = inputs(2, O, H, W, 4, k)
    for unc, pur in (("entropy", "ripu"), ("entropy", "radius")):
        for norm in (True, False):
            check_score(dev, logit, emb, gt, unc, pur, norm, k, pad)
    frs = FloatingRegionScore(in_channels=O, padding_mode=pad, size=k, purity_type="ripu")
    p = ho.softmax(logit[0])
    u = frs.compute_region_uncertainty("entropy", t(logit[0], dev), t(p, dev))
    assert bits_equal(u.cpu().numpy(), ho.uncertainty_from_probs(p, "entropy", size=k, padding_mode=pad))
    pred = p.argmax(axis=0).astype(np.int64)
    imp, cnt = frs.compute_region_impurity(t(pred, dev), O)
    io, co = ho.region_impurity(pred, O, k, pad)
    assert bits_equal(imp.cpu().numpy(), io) and bits_equal(cnt.cpu().numpy(), co)


@pytest.mark.parametrize("O", [2, 16, 32, 33])
def test_bin_counts_and_label_types(dev, O):
    """Bin counts on both sides of the word boundaries of the packed counters (8 classes per 16-byte element) and of the kernel's
    limit of 32 (33: the generic kernel, same bits); the int16 labels of the pipeline and the int64 labels of the helper entry."""
    from halo_amd.core.active.floating_region import FloatingRegionScore, window_route
    from oracle import halo_oracle as ho
    H, W, k = 70, 130, 9
    assert window_route("hist", k, "zeros", O, (H, W)) == ("tiled" if O <= 32 else "generic")
    logit, emb, gt = inputs(1, O, H, W, 4, O)
    check_score(dev, logit, emb, gt, "entropy", "ripu", True, k)
    check_score(dev, logit, emb, gt, "oracle_acc", "oracle_ripu", False, k)
    frs = FloatingRegionScore(in_channels=O, size=k, purity_type="ripu")
    pred = np.random.default_rng(O).integers(0, O, (H, W)).astype(np.int64)
    imp, cnt = frs.compute_region_impurity(t(pred, dev), O)
    io, co = ho.region_impurity(pred, O, k)
    assert bits_equal(imp.cpu().numpy(), io) and bits_equal(cnt.cpu().numpy(), co)


def logits_of(labels, O, seed):
    """logits whose arg-max is the given label map"""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((1, O) + labels.shape).astype(np.float32) * 0.3
    lg[0] += 6.0 * (np.arange(O)[:, None, None] == labels[None]).astype(np.float32)
    return lg


@pytest.mark.parametrize("kind", ["uniform", "one_odd_pixel", "blocky", "noise"])
@pytest.mark.parametrize("k", [5, 33])
def test_degenerate_and_realistic_label_maps(dev, kind, k):
    """A uniform label map has a constant impurity: normalize_map divides 0 by 0 and the score is NaN everywhere, as in the oracle;
    one odd pixel makes the range positive again.  Blocky maps (2 to 6 classes per window) are the realistic case, pure noise puts
    every class into every window."""
    H, W, O = 70, 130, 19
    assert tiled("hist", k, shape=(H, W))
    rng = np.random.default_rng(k)
    if kind == "uniform":
        lab = np.full((H, W), 7)
    elif kind == "one_odd_pixel":
        lab = np.full((H, W), 7)
        lab[33, 101] = 18
    elif kind == "blocky":
        lab = np.kron(rng.integers(0, O, (-(-H // 12), -(-W // 12))), np.ones((12, 12), np.int64))[:H, :W]
    else:
        lab = rng.integers(0, O, (H, W))
    logit = logits_of(lab, O, k)
    assert np.array_equal(logit[0].argmax(axis=0), lab)
    emb = np.zeros((1, 2, H, W))
    gt = lab[None].astype(np.int64)
    for norm in (True, False):
        check_score(dev, logit, emb, gt, "entropy", "ripu", norm, k)


def generic_walk(pred, K, k):
    """NumPy statement of the generic window walk of halo_region_impurity with zero padding for ARBITRARY labels: classes below 0
    are never counted (but their pixels count in the window size), every other label is its own class, the classes' terms
    (-d) log(d + 1e-6), d = n / count, are summed in ascending class order in torch.sum's cascade over the class index."""
    from oracle import halo_oracle as ho
    H, W = pred.shape
    r = k // 2

    def box(m):
        c = np.zeros((H + 1, W + 1), np.int64)
        c[1:, 1:] = np.cumsum(np.cumsum(m.astype(np.int64), axis=0), axis=1)
        y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
        x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
        return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]
    cnt = box(np.ones((H, W))).astype(np.float32)
    terms = np.zeros((int(pred.max()) + 1, H, W), np.float32)
    for c in np.unique(pred[pred >= 0]):
        n = box(pred == c)
        d = n.astype(np.float32) / cnt
        terms[c] = np.where(n > 0, (-d) * ho.logf(d + np.float32(1e-6)), np.float32(0.0))
    return ho.sum_dim0(terms) / np.float32(math.log(K)), cnt


def test_labels_outside_the_bins_take_the_generic_walk(dev):
    """halo_region_impurity takes any int64 labels.  A tile of the tiled kernel that stages a label outside [0, K) walks its pixels
    as the generic kernel does; the other tiles count in LDS.  K sets both the bin count and log K, so the two routes cannot be
    asked for the same map through the ABI: both are compared with the NumPy statement of the generic walk."""
    from halo_amd import _lib
    from halo_amd.core.active.floating_region import window_route
    H, W, k = 40, 72, 9
    rng = np.random.default_rng(4)
    pred = rng.integers(0, 19, (H, W)).astype(np.int64)
    pred[3, 5], pred[20, 70], pred[39, 0] = 19, 40, 25          # >= bins
    pred[17, 33] = -3                                           # negative: never counted
    L = _lib.lib()
    for K in (19, 100):
        assert window_route("hist", k, "zeros", K, (H, W)) == ("tiled" if K == 19 else "generic")
        pd = t(pred, dev)
        imp = torch.empty((H, W), dtype=torch.float32, device=dev)
        cnt = torch.empty((H, W), dtype=torch.float32, device=dev)
        rc = L.halo_region_impurity(_lib.ptr(pd), 1, H, W, k, K, _lib.ptr(imp), _lib.ptr(cnt), _lib.PAD["zeros"], _lib.stream_ptr(dev))
        _lib.check(rc, "halo_region_impurity")
        torch.cuda.synchronize()
        want, wcnt = generic_walk(pred, K, k)
        assert bits_equal(cnt.cpu().numpy(), wcnt), K
        assert bits_equal(imp.cpu().numpy(), want), K
    # a wide map: tiles with and without such a label side by side (the histogram tile is 256 columns wide)
    H, W = 24, 600
    pred = rng.integers(0, 19, (H, W)).astype(np.int64)
    pred[5, 300] = 77
    pd = t(pred, dev)
    imp = torch.empty((H, W), dtype=torch.float32, device=dev)
    rc = L.halo_region_impurity(_lib.ptr(pd), 1, H, W, k, 19, _lib.ptr(imp), None, _lib.PAD["zeros"], _lib.stream_ptr(dev))
    _lib.check(rc, "halo_region_impurity")
    torch.cuda.synchronize()
    assert bits_equal(imp.cpu().numpy(), generic_walk(pred, 19, k)[0])


@pytest.mark.parametrize("k", [5, 33])
def test_entropy_with_nan_and_inf(dev, k):
    """A NaN and an infinite entropy: the box sums carry them into every window that holds the pixel, and the min / max of
    normalize_map propagate the NaN as torch's do (the oracle states both)."""
    from halo_amd.core.active.floating_region import FloatingRegionScore
    from oracle import halo_oracle as ho
    H, W, O = 70, 130, 19
    assert tiled("box", k, shape=(H, W))
    logit, emb, gt = inputs(1, O, H, W, 4, 5)
    p = ho.softmax(logit[0])
    p[:, 10, 100] = np.nan
    p[3, 60, 7] = np.inf                                        # -inf * log(inf) = -inf
    frs = FloatingRegionScore(in_channels=O, size=k, purity_type="ripu")
    u = frs.compute_region_uncertainty("entropy", t(logit[0], dev), t(p, dev)).cpu().numpy()
    uo = ho.uncertainty_from_probs(p, "entropy", size=k)
    assert np.isnan(uo).any() and np.isinf(uo).any() and np.isfinite(uo).any()
    assert bits_equal(u, uo)
    bad = logit.copy()
    bad[0, :, 10, 100] = np.nan
    for norm in (True, False):
        check_score(dev, bad, emb, gt, "entropy", "ripu", norm, k)
        check_score(dev, bad, emb, gt, "entropy", "radius", norm, k)


def test_module_defaults_are_on_the_tiled_route(dev):
    from halo_amd.core.active.floating_region import FloatingRegionScore
    from oracle import halo_oracle as ho
    H, W, O = 64, 96, 19
    frs = FloatingRegionScore(in_channels=O, purity_type="ripu")
    assert frs.size == 33 and frs.purity_size == 33
    assert tiled("box", frs.size, frs.padding_mode, O, (H, W)) and tiled("hist", frs.purity_size, frs.padding_mode, O, (H, W))
    logit, emb, gt = inputs(1, O, H, W, 4, 33)
    for norm in (True, False):
        s, i, u = frs(t(logit, dev), None, unc_type="entropy", pur_type="ripu", normalize=norm)
        so, io, uo = ho.floating_region_score(logit, None, "entropy", "ripu", norm, None, size=33, purity_type="ripu")
        assert bits_equal(s.cpu().numpy(), so) and bits_equal(i.cpu().numpy(), io) and bits_equal(u.cpu().numpy(), uo)
