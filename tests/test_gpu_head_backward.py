"""The training backward of the hyperbolic head tail against a float64 CPU restatement, per pixel, on every route.

halo_expmap0_project_bwd, halo_hypermlr_backward (k_mlr_prep, k_mlr_bwd_pixels in both weight arms, k_mlr_bwd_dxw, k_mlr_bwd_final) and
the term-map path (halo_hypermlr_bwd_terms + mlr_backward_terms) against tests/head_ref.py: torch CPU autograd over the same algebra
written out in plain float64 ops, which tests/test_head_ref_host.py ties to the reference's recorded autograd (grads.npz).  The other
tests of these calls compare one device path with another (shared k_mlr_prep, shared mlr_reverse) or hold a bar relative to the
tensor's global maximum; here nothing on the reference side is device code, and the rule is per slice:

    max_ch |got - ref| <= BAR * max_ch |ref|  at every pixel (d x, d z) and in every class row (d P, d A),
    plus BAR * 1e-3 * max |ref| as an absolute floor for slices whose gradient is exactly 0.

F is the reference's own noise in that measure (itself in another summation order: 4.2e-13 measured on the CPU over MLR_CASES, held
below head_ref.FLOOR = 5e-13 by the host test), BAR = 64 F = 3.2e-11, below the 1e-10 the project already holds globally.  x is
head_ref.expmap_ref(z) uploaded, so the device's forward is not in the loop, and the inputs keep sqrt(mob) >= 1e-9 (relative) from the
projection limit (host test), so no where() can flip between the two sides and no element is masked out.  Largest error / BAR seen
on an MI355X: 0.006 (d x of the C = 256 case, i.e. 2e-13 of the pixel's maximum: the reference's own noise there); 0.001 or less in
every other case; float32 d z of the expmap: 0 ulps from the rounded reference everywhere.

Not covered, and why: the D < 1e-12 arm of the sweep -- D0 >= (1 - c ||p|| ||x||)^2, so it is reached only at a near-exact
singularity, where the reference itself returns NaN or values near 1e24 --, and 1 - c * mobprojected < 1e-12, which cannot happen for
finite input (mobprojected <= (1 - 1e-3)^2 / c).  No forward kernels: they are held bit for bit against the oracle elsewhere."""
import functools

import numpy as np
import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu

F = R.FLOOR                      # 5e-13 >= the 4.2e-13 measured (tests/test_head_ref_host.py::test_noise_floor_of_the_reference)
BAR = 64 * F                     # 3.2e-11
assert BAR <= 1e-10

FUSED = [c for c in R.MLR_CASES if c[7]]
TERMS = [c for c in R.MLR_CASES if not c[7]]


def ids(cases):
    return ["x".join(str(v) for v in c[:6]) for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def served_by_fused(case):
    from halo_amd import _lib
    B, C, O, h, w = case[:5]
    return _lib.lib().halo_hypermlr_backward_workspace_bytes(B, C, O, h * w) != 0


def device_grads(x, P, A, Wt, c, dev, way):
    """d <HyperMLR(x), Wt> / d (x, P, A) through _HyperMLRFn's backward.  way: 'f64' (float64 gout), 'f32' (float32 logits and a
    float32 gout, the head's `.float()`), 'offset' (x one element into a larger buffer: 8- but not 16-byte aligned)"""
    from halo_amd.core.utils.hyperbolic import _HyperMLRFn
    if way == "offset":
        buf = torch.empty(x.numel() + 1, dtype=torch.float64, device=dev)
        buf[1:].copy_(x.reshape(-1))
        xd = buf[1:].view(x.shape)
        assert xd.data_ptr() % 16 == 8 and xd.is_contiguous()
    else:
        xd = x.to(dev)
    xd = xd.detach().requires_grad_(True)
    Pd, Ad = P.to(dev).requires_grad_(True), A.to(dev).requires_grad_(True)
    if way == "f32":
        out = _HyperMLRFn.apply(xd, Pd, Ad, c, torch.float32)
        assert out.dtype == torch.float32
        (out * Wt.float().to(dev)).sum().backward()
    else:
        (_HyperMLRFn.apply(xd, Pd, Ad, c) * Wt.to(dev)).sum().backward()
    got = [g.grad.cpu().numpy() for g in (xd, Pd, Ad)]
    assert all(g.dtype == np.float64 for g in got)
    return got


def check(got, ref, tag):
    ratios = (R.slice_ratio(got[0], ref[0], 1, BAR), R.slice_ratio(got[1], ref[1], 1, BAR), R.slice_ratio(got[2], ref[2], 1, BAR))
    print(tag, "error / bar: d x %.2e  d P %.2e  d A %.2e  (bar %.1e)" % (ratios + (BAR,)))
    assert max(ratios) <= 1.0, (tag, ratios)


@pytest.mark.parametrize("way", ["f64", "f32", "offset"])
@pytest.mark.parametrize("case", FUSED, ids=ids(FUSED))
def test_fused_backward_matches_float64_per_pixel(dev, case, way):
    assert served_by_fused(case)
    x, P, A, Wt = R.mlr_case(case)
    check(device_grads(x, P, A, Wt, case[5], dev, way), R.mlr_ref(case), (case[:6], way))


@pytest.mark.parametrize("case", TERMS, ids=ids(TERMS))
def test_term_path_matches_float64_per_pixel(dev, case):
    assert not served_by_fused(case)
    x, P, A, Wt = R.mlr_case(case)
    check(device_grads(x, P, A, Wt, case[5], dev, "f64"), R.mlr_ref(case), (case[:6], "terms"))


def test_term_path_at_a_fused_shape_matches_float64_per_pixel(dev):
    """mlr_backward_terms called directly at a shape the fused call serves: the sweep kernel's first full class block and C = 64"""
    from halo_amd.core.utils.hyperbolic import mlr_backward_terms
    case = R.MLR_CASES[0]
    x, P, A, Wt = R.mlr_case(case)
    got = [g.cpu().numpy() for g in mlr_backward_terms(x.to(dev), P.to(dev), A.to(dev), Wt.to(dev), case[5])]
    check(got, R.mlr_ref(case), (case[:6], "terms, direct"))


@functools.lru_cache(maxsize=None)
def nan_problem():
    x, P, A, Wt = R.mlr_case(R.NAN_CASE)
    x = x.clone()
    x[1, :, 8, 9] = float("nan")                                          # an interior pixel, inside the ball before
    return x, P, A, Wt, R.grads_ref(x, P, A, Wt, R.NAN_CASE[5])


@pytest.mark.parametrize("way", ["f64", "f32", "offset"])
def test_fused_backward_with_a_nan_pixel(dev, way):
    """the only input that reaches the fast sweep's `ok = false` arm without lying on the ball's edge: d x is NaN at that pixel and
    meets the bar at every other one; d P and d A are NaN wherever the reference's are (everywhere: every class sums over the pixel)"""
    x, P, A, Wt, ref = nan_problem()
    at = np.zeros(ref[0].shape, bool)
    at[1, :, 8, 9] = True
    assert np.array_equal(np.isnan(ref[0]), at) and np.isnan(ref[1]).all() and np.isnan(ref[2]).all()
    assert served_by_fused(R.NAN_CASE)
    check(device_grads(x, P, A, Wt, R.NAN_CASE[5], dev, way), ref, ("nan pixel", way))     # slice_ratio: NaNs must coincide


EXPMAP_SHAPES = [((2, 7, 3, 5), 1), ((2, 64, 3, 5), 1), ((2, 256, 3, 5), 1), ((300, 7), -1), ((300, 64), -1), ((300, 256), -1)]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("c", [1.0, 0.7])
@pytest.mark.parametrize("shape,dim", EXPMAP_SHAPES, ids=["x".join(map(str, s)) for s, _ in EXPMAP_SHAPES])
def test_expmap_backward_matches_float64_per_pixel(dev, shape, dim, c, f64):
    """halo_expmap0_project_bwd through HyperMapper.expmap under autograd: NCHW dim=1 and the inner = 1 route with more than one
    workgroup, with an exact-origin pixel, one below the norm clamp (float64 input), one inside, two projected with tanh live, one on
    either side of the tanh clamp and one far out (asserted from the reference side: each lies where its name says).  float64 d z: the
    per-pixel bar; float32 d z: within 1 float32 ulp of the float64 reference rounded to float32 -- the kernel rounds a float64 result once."""
    from halo_amd.core.utils.hyperbolic import HyperMapper
    z, gy, planted = R.expmap_case(shape, dim, c, f64)
    R.check_planted_classes(z, c, dim, planted, f64)
    ref = R.expmap_grad_ref(z, gy, c, dim)
    zd = z.to(dev).requires_grad_(True)
    y = HyperMapper(c=c).expmap(zd, dim=dim)
    assert y.dtype == torch.float64
    (y * gy.to(dev)).sum().backward()
    got = zd.grad.cpu().numpy()
    assert np.isfinite(got).all()
    if f64:
        assert got.dtype == np.float64
        ratio = R.slice_ratio(got, ref, dim % len(shape), BAR)
        print(shape, dim, c, "f64 error / bar %.2e" % ratio)
        assert ratio <= 1.0
    else:
        assert got.dtype == np.float32
        ref32 = ref.astype(np.float32)
        ulps = float((np.abs(got.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)).max())
        print(shape, dim, c, "f32 ulps from the rounded reference %.1f" % ulps)
        assert ulps <= 1.0
