"""CPU checks of tests/head_ref.py, the float64 yardstick of tests/test_gpu_head_backward.py: it reproduces the reference's own autograd
of the head tail (tests/golden/grads.npz), its own noise stays below the FLOOR the device bars are built from, and the inputs of the
device tests keep clear of the places where a last-bit difference could flip a where() between reference and device."""
import numpy as np
import pytest
import torch

import head_ref as R


@pytest.mark.parametrize("tag", ["c8_o19", "c16_o16_k07", "c64_o19"])
def test_reference_reproduces_the_recorded_autograd(golden, tag):
    """loss = <HyperMLR(embed).float(), Wt> + <embed, Ve>, embed = expmap(z, dim=1), as tests/golden/make_fixtures.py ran it through the
    reference: embed within 1e-14; d embed, d P, d A within 1e-12 of the tensor's maximum, d embed also within 1e-12 of every pixel's
    own maximum; d z (float32) bit for bit."""
    d = golden("grads")
    c = float(d[tag + "__c"][0])
    z = torch.from_numpy(d[tag + "__z"]).requires_grad_(True)
    P = torch.from_numpy(d[tag + "__P"]).requires_grad_(True)
    A = torch.from_numpy(d[tag + "__A"]).requires_grad_(True)
    embed = R.expmap_ref(z, c, 1)
    embed.retain_grad()
    logits = R.hyper_logits_ref(embed, P, A, c).float()
    ((logits * torch.from_numpy(d[tag + "__Wt"])).sum() + (embed * torch.from_numpy(d[tag + "__Ve"])).sum()).backward()
    assert np.abs(embed.detach().numpy() - d[tag + "__embed"]).max() <= 1e-14

    def rel(got, want):
        return float(np.abs(got - want).max() / np.abs(want).max())
    g_embed, want = embed.grad.numpy(), d[tag + "__g_embed"]
    per_pixel = float((np.abs(g_embed - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    figures = (rel(g_embed, want), per_pixel, rel(P.grad.numpy(), d[tag + "__g_P"]), rel(A.grad.numpy(), d[tag + "__g_A"]))
    print(tag, "d embed %.2e (per pixel %.2e)  d P %.2e  d A %.2e" % figures)
    assert max(figures) <= 1e-12, figures
    assert z.grad.dtype == torch.float32 and np.array_equal(z.grad.numpy(), d[tag + "__g_z"])
    # the fixture's two far-out pixels and its origin pixel are where the names say
    a, projected, gprime = R.expmap_pixel_classes(z.detach(), c, 1)
    assert projected[0, 0, 0] and gprime[0, 0, 0] == 0.0 and projected[1, 2, 3] and a[0, 1, 1] == 0.0 and not projected[0, 1, 1]
    assert np.array_equal(R.grads_ref(embed.detach(), P.detach(), A.detach(), d[tag + "__Wt"], c, float_logits=True)[1],
                          R.grads_ref(embed.detach(), P.detach(), A.detach(), d[tag + "__Wt"], c)[1])


def _shuffled(case):
    """the same problem with the channels permuted and the pixel grid reversed: every sum in another order"""
    x, P, A, Wt = R.mlr_case(case)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(x.shape[1]))
    return perm, (x[:, perm].flip(2, 3).contiguous(), P[:, perm].contiguous(), A[:, perm].contiguous(), Wt.flip(2, 3).contiguous())


def test_noise_floor_of_the_reference():
    """grads_ref against itself in another summation order, in the device tests' own measure (slice_ratio with bar = 1: per pixel
    for d x, per class row for d P and d A).  Printed per case; the largest must stay below FLOOR, and FLOOR below 1e-12."""
    worst = 0.0
    for case, name in zip(R.MLR_CASES, R.MLR_IDS):
        gx, gP, gA = R.mlr_ref(case)
        perm, (x2, P2, A2, W2) = _shuffled(case)
        hx, hP, hA = R.grads_ref(x2, P2, A2, W2, case[5])
        inv = np.argsort(perm.numpy())
        f = (R.slice_ratio(hx[:, inv][:, :, ::-1, ::-1], gx, 1, 1.0), R.slice_ratio(hP[:, inv], gP, 1, 1.0), R.slice_ratio(hA[:, inv], gA, 1, 1.0))
        print("floor %-22s d x %.2e  d P %.2e  d A %.2e" % ((name,) + f))
        worst = max(worst, *f)
    print("floor f = %.2e (FLOOR %.1e)" % (worst, R.FLOOR))
    assert worst <= R.FLOOR <= 1e-12


def test_expmap_noise_floor_and_planted_classes():
    """the expmap reference against itself with the channels permuted, per pixel, in every pixel class; and every planted class lies
    where its name says (projection active or not, 1 - tanh^2 zero or not)"""
    worst = 0.0
    for shape, dim in (((2, 7, 3, 5), 1), ((2, 64, 3, 5), 1), ((2, 256, 3, 5), 1), ((300, 7), -1), ((300, 64), -1), ((300, 256), -1)):
        for c in (1.0, 0.7):
            for f64 in (False, True):
                z, gy, planted = R.expmap_case(shape, dim, c, f64)
                R.check_planted_classes(z, c, dim, planted, f64)
                g = R.expmap_grad_ref(z, gy, c, dim)
                perm = torch.from_numpy(np.random.default_rng(6).permutation(shape[dim]))
                g2 = R.expmap_grad_ref(z.index_select(dim, perm), gy.index_select(dim, perm), c, dim)
                g2 = np.take(g2, np.argsort(perm.numpy()), axis=dim % len(shape))
                assert np.isfinite(g).all()
                worst = max(worst, R.slice_ratio(g2, g, dim % len(shape), 1.0))
    print("expmap floor %.2e" % worst)
    assert worst <= R.FLOOR


@pytest.mark.parametrize("case", R.MLR_CASES, ids=R.MLR_IDS)
def test_input_builder_conditions(case):
    """every case reaches the `over` arm of the sweep (its three planted x40 / x300 pixels, every class of them), keeps sqrt(mob)
    at least 1e-9 (relative) from the projection limit and D0 at least 1e-3 from its clamp; so no element is ever masked out of
    a comparison.  The fused cases lie on the fused side of the dispatch rule, the term cases on the other."""
    B, C, O, h, w, c, _, fused = case
    x, P, A, Wt = R.mlr_case(case)
    n_over, margin, d0 = R.margins(x, P, A, c)
    print("margins %-22s over %d of %d (%.2f %%)  sqrt(mob) margin %.2e  D0 >= %.3f" % ("x".join(map(str, case[:6])), n_over, B * O * h * w,
                                                                                        100.0 * n_over / (B * O * h * w), margin, d0))
    assert n_over >= 3 * O and margin >= 1e-9 and d0 >= 1e-3
    assert n_over >= (0.05 if case[6] > 0.15 else 0.0) * B * O * h * w      # the C = 256 case: a large share beyond the limit
    assert n_over < B * O * h * w // 2                                      # and most elements inside, in every case
    assert fused == (O <= 20 and C % 64 == 0 and 64 <= C <= 256)
    assert (B * h * w >= 400000) == (case == R.MLR_CASES[6])
    assert all(np.isfinite(g).all() for g in R.mlr_ref(case))
    assert float(x[0, :, 0, 0].abs().max()) == 0.0                          # the exact-origin pixel
    assert torch.equal(Wt.float().double(), Wt)
