"""CPU checks of tests/loss_ref.py, the float64 yardstick of tests/test_gpu_losses.py: it reproduces tests/golden/losses.npz (the
reference's own LocalConsistentLoss / NegativeLearningLoss under autograd), its integer boundary rule is the reference's float
convolution rule, the data of every LocalConsistentLoss case keeps clear of the band where a float32 sign(p - mean) is not
determined, and the float32 torch CPU chain stays within the stored K_REF of it."""
import functools

import numpy as np
import pytest
import torch

import loss_ref as R

U = R.U
CASE_IDS = ["x".join(str(v) for v in c) for c in R.LCL_CASES]


@functools.lru_cache(maxsize=None)
def data(case):
    return R.lcl_case(*case)


def chain_ratio(x, label, kl):
    """max |g32 - g64| / (2^-24 A) of the float32 chain over the elements with A > 0, and max |g32| over the others"""
    ref = R.local_consistent(x, label, kl)
    l32, m32, g32 = R.chain32(x, label, kl)
    assert np.array_equal(m32, ref.mask) and int(m32.sum()) == ref.count
    assert abs(l32 - ref.loss) <= 8 * U * abs(ref.loss)
    pos = ref.A > 0
    k = float((np.abs(g32.astype(np.float64) - ref.gx)[pos] / (U * ref.A[pos])).max())
    return k, (float(np.abs(g32[~pos]).max()) if (~pos).any() else 0.0), ref


@pytest.mark.parametrize("lt", ["l1", "kl"])
def test_evaluator_reproduces_the_reference_fixture_local_consistent(golden, lt):
    """value within 4 float32 ulps of the stored float32 loss; gradient within 2e-6 max|g| of the stored float32 gradient (34
    ulps of the largest element: the fixture IS a float32 chain; test_gpu_parity.py allows the kernels 2e-5 against it); mask and
    count equal the reference's float-convolution rule; gx and A vanish exactly where no masked pixel is in the 3x3 window.
    (The per-element ratio to 2^-24 A is printed, not asserted: K_REF belongs to the data of LCL_CASES, the fixture's logits are
    smooth and showed 29.9 for 'kl'.)"""
    d = golden("losses")
    ref = R.local_consistent(d["x"], d["label"], lt == "kl")
    want = float(d[f"lcl_{lt}__loss"][0])
    assert abs(ref.loss - want) <= 4 * U * abs(want), (ref.loss, want)
    _, m32, _ = R.chain32(d["x"], d["label"], lt == "kl")
    assert np.array_equal(ref.mask, m32) and ref.count == int(m32.sum()) and ref.count > 0
    g = d[f"lcl_{lt}__gx"].astype(np.float64)
    pos = ref.A > 0
    print("fixture", lt, "k = %.2f" % float((np.abs(g - ref.gx)[pos] / (U * ref.A[pos])).max()),
          "band ratio %.2e" % R.band_ratio(d["x"], d["label"]))
    assert np.abs(g - ref.gx).max() <= 2e-6 * np.abs(ref.gx).max()
    reach = torch.nn.functional.max_pool2d(torch.from_numpy(ref.mask).float()[:, None], 3, 1, 1)[:, 0].bool().numpy()
    assert not ref.gx[~np.broadcast_to(reach[:, None], ref.gx.shape)].any()     # no masked pixel in the 3x3 window: gx = 0 exactly
    assert np.array_equal(ref.A > 0, np.broadcast_to(reach[:, None], ref.A.shape))


def test_evaluator_reproduces_the_reference_fixture_negative_learning(golden):
    d = golden("losses")
    p, gp = d["neg__p"], d["neg__gp"]
    ref = R.negative_learning(p, 0.05)
    assert np.array_equal(ref.mask, gp != 0) and ref.count == int((gp != 0).sum()) and ref.count > 0
    want = float(d["neg__loss"][0])
    assert abs(ref.loss - want) <= 4 * U * abs(want), (ref.loss, want)
    assert not ref.gp[~ref.mask].any()
    assert np.all(np.abs(gp.astype(np.float64) - ref.gp)[ref.mask] <= 6 * U * ref.gp[ref.mask])


def test_negative_learning_mask_is_the_float32_comparison():
    t = np.float32(0.05)
    p = np.array([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), 0.0, 0.2], np.float32)
    ref = R.negative_learning(p, 0.05)
    assert ref.mask.tolist() == [False, True, False, True, False] and ref.count == 2
    q0 = float(np.float32(1.0) + np.float32(1e-6))                  # p = 0: the operand is float32(1 + 1e-6f), not 1 + 1e-6
    assert ref.gp[3] == 1.0 / (q0 * 2) and ref.gp[0] == 0.0
    none = R.negative_learning(np.full(4, 0.5, np.float32), 0.05)
    assert np.isnan(none.loss) and none.count == 0 and not none.gp.any()


def test_empty_selection_is_nan_with_a_zero_gradient(golden):
    d = golden("losses")
    ref = R.local_consistent(d["empty__x"], np.zeros((1, 8, 8), np.int64), False)
    assert np.isnan(ref.loss) and bool(d["empty__loss_isnan"][0]) and ref.count == 0 and not ref.mask.any()
    assert not ref.gx.any() and not ref.A.any() and not d["empty__gx"].any()


def test_boundary_rule_on_integers_is_the_reference_float_convolution():
    g = torch.Generator().manual_seed(5)
    label = torch.randint(0, 256, (3, 13, 17), generator=g)            # every label value, 255 included, at borders and corners
    label[0, :, 0] = 255
    label[1, 0, :] = 254
    _, m32, _ = R.chain32(torch.zeros((3, 2, 13, 17)), label, False)
    assert np.array_equal(R.boundary_mask(label).numpy(), m32)
    assert np.array_equal(R.boundary_mask(label.to(torch.uint8)).numpy(), m32)
    flat = torch.full((1, 6, 7), 9)
    m = R.boundary_mask(flat).numpy()
    assert m[0, 0].all() and m[0, :, 0].all() and not m[0, 1:-1, 1:-1].any()      # zero padding: the image border is a boundary


@pytest.mark.parametrize("case", R.LCL_CASES, ids=CASE_IDS)
def test_no_masked_pair_lies_in_the_float32_sign_band(case):
    """the share of (pixel, class) pairs left out of the GPU comparison is zero: the band is empty, nothing is filtered"""
    x, label = data(case)
    r = R.band_ratio(x, label)
    print(case, "smallest |p - mean| / max(p, mean) = %.3e = %.2f bands" % (r, r / R.BAND))
    assert r >= R.BAND, (case, r)
    assert int(R.boundary_mask(label).sum()) > 0 and bool((label == 255).any())


def test_float32_cpu_chain_stays_within_k_ref():
    worst = 0.0
    for case in R.LCL_CASES:
        x, label = data(case)
        ks = []
        for kl in (False, True):
            k, stray, ref = chain_ratio(x, label, kl)
            ks.append(k)
            # (where A == 0 the float32 chain itself is NOT exactly zero everywhere: its convolution backward leaves residues of
            #  1e-12 at pixels no masked pixel reaches, which is why the kernels are held to this evaluator and not to the chain)
            assert stray <= 1e-9 * np.abs(ref.gx).max()
        print(case, "k_l1 = %.2f  k_kl = %.2f  (stored %s)" % (ks[0], ks[1], R.K_REF_MEASURED[case]))
        worst = max(worst, *ks)
    assert worst <= R.K_REF, worst
    assert worst >= 0.5 * R.K_REF, worst                               # the stored constant is the measurement, not a loose cap
