"""Float64 CPU yardstick of the hyperbolic head tail's backward (tests/test_gpu_head_backward.py, anchored by
tests/test_head_ref_host.py): project(expmap0(z.double())) and HyperMLR's logit algebra restated statement by statement in plain
torch ops -- from the numeric contract the kernels' own comments state (halo_amd/csrc/halo_hyperbolic.hip) -- and differentiated by
torch's CPU autograd.  Nothing here touches the device library.

  expmap_ref        n = ||z||.clamp_min(1e-15), g = tanh(clamp(n ks, +-15)) / ks with ks = sqrt(c + 1e-15), y0 = g (z / n), and the
                    projection y0 / ||y0||.clamp_min(1e-15) * maxnorm where ||y0|| > maxnorm = (1 - 1e-5) / ks
  hyper_logits_ref  D = max(1 + 2K px + K^2 xx pp, 1e-12), the Moebius sum's norm from alpha = A / D and beta = B / D, both where()s of
                    the projection at (1 - 1e-3) / sqrt(K), F.normalize, max(1 - K mobprojected, 1e-12), asinh
  grads_ref         d <logits, Wt> / d (x, P, A)
  margins           how far an input keeps from the places where a last-bit difference could flip a where()
  mlr_case / expmap_case   the inputs of the device tests, built here so that the host test can check their conditions
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

# The reference's own noise: grads_ref against itself with the channels permuted and the pixels reversed (another summation order
# everywhere), per pixel relative to that pixel's largest |gradient| (d x) and per class row (d P, d A).  Largest value over
# MLR_CASES measured on the CPU: 4.2e-13 (d x of the C = 256 case, whose pixels lie closest to the projection limit; every other case stays
# below 4e-14, the expmap below 1e-15).  test_head_ref_host.py::test_noise_floor_of_the_reference prints the figures and asserts
# them below FLOOR.  The device bars are built from FLOOR.
FLOOR = 5e-13

PROJ_EPS_MLR = 1e-3
PROJ_EPS_MAP = 1e-5


# ------------------------------------------------------------------ expmap0 + project
def _expmap_parts(z, c, dim):
    z = z.double()
    ks = math.sqrt(c + 1e-15)
    maxnorm = (1.0 - PROJ_EPS_MAP) / ks
    n = z.norm(dim=dim, p=2, keepdim=True).clamp_min(1e-15)
    a = n * ks
    g = a.clamp(-15.0, 15.0).tanh() / ks
    y0 = g * (z / n)
    ny = y0.norm(dim=dim, p=2, keepdim=True).clamp_min(1e-15)
    return y0, ny, maxnorm, a


def expmap_ref(z, c, dim):
    """project(expmap0(z.double())) over `dim`, float64, differentiable"""
    y0, ny, maxnorm, _ = _expmap_parts(z, c, dim)
    return torch.where(ny > maxnorm, y0 / ny * maxnorm, y0)


def expmap_pixel_classes(z, c, dim):
    """per pixel (`dim` squeezed out), from the reference side: a = ks ||z|| before any clamp, whether the projection acts, and the
    factor d tanh / d a the backward sees (1 - tanh^2 inside the tanh clamp, 0.0 beyond it)"""
    with torch.no_grad():
        z = z.double()
        a = z.norm(dim=dim, p=2) * math.sqrt(c + 1e-15)
        _, ny, maxnorm, _ = _expmap_parts(z, c, dim)
        th = a.clamp(-15.0, 15.0).tanh()
        gprime = torch.where(a <= 15.0, 1.0 - th * th, torch.zeros_like(a))
    return a.numpy(), (ny.squeeze(dim) > maxnorm).numpy(), gprime.numpy()


def expmap_grad_ref(z, gy, c, dim):
    """d <expmap_ref(z), gy> / d z in float64 (z float32 or float64: the cast's backward is left to the caller)"""
    zz = z.detach().double().requires_grad_(True)
    (g,) = torch.autograd.grad((expmap_ref(zz, c, dim) * gy).sum(), zz)
    return g.numpy()


# ------------------------------------------------------------------ HyperMLR
def _mlr_scalars(x, P, A, c):
    """the per-(pixel, class) scalars up to the Moebius sum's squared norm; x (B, C, h, w), P and A (O, C), float64"""
    K = float(c)
    xx = (x.norm(dim=1, p=2) ** 2).unsqueeze(1)                            # (B, 1, h, w)
    pp = (P.norm(dim=1, p=2) ** 2)[None, :, None, None]                     # (1, O, 1, 1)
    px = torch.einsum("bchw,oc->bohw", x, -P)
    D0 = 1.0 + 2.0 * K * px + K * xx * K * pp
    D = torch.maximum(D0, torch.tensor(1e-12, dtype=torch.float64))
    alpha = (1.0 + 2.0 * K * px + K * xx) / D
    beta = (1.0 - K * pp) / D
    mob = alpha ** 2 * pp + beta ** 2 * xx + 2.0 * alpha * beta * px
    return K, xx, pp, px, D0, alpha, beta, mob


def hyper_logits_ref(x, P, A, c):
    """HyperMLR's logits (B, O, h, w), float64, differentiable in x, P and A"""
    K, xx, pp, px, D0, alpha, beta, mob = _mlr_scalars(x, P, A, c)
    tiny = torch.tensor(1e-12, dtype=torch.float64)
    maxnorm = (1.0 - PROJ_EPS_MLR) / math.sqrt(K)
    sq = torch.sqrt(mob)
    pn = torch.where(sq > maxnorm, maxnorm / torch.maximum(sq, tiny), torch.ones_like(mob))
    mobprojected = torch.where(sq < maxnorm, mob, torch.full_like(mob, maxnorm ** 2))
    a_norm = A.norm(dim=1, p=2)
    An = F.normalize(A, dim=1)
    xa = torch.einsum("bchw,oc->bohw", x, An)
    pa = (-P * An).sum(dim=1)[None, :, None, None]
    mobdota = (beta * xa + alpha * pa) * pn
    lam = 2.0 / torch.maximum(1.0 - K * mobprojected, tiny)
    sineterm = math.sqrt(K) * mobdota * lam
    return 2.0 / math.sqrt(K) * a_norm[None, :, None, None] * torch.asinh(sineterm)


def grads_ref(x, P, A, Wt, c, float_logits=False):
    """d <logits, Wt> / d (x, P, A) as float64 numpy arrays; float_logits: the head's `.float()` between the logits and the product"""
    x, P, A = (torch.as_tensor(v).detach().double().clone().requires_grad_(True) for v in (x, P, A))
    logits = hyper_logits_ref(x, P, A, c)
    Wt = torch.as_tensor(Wt)
    loss = (logits.float() * Wt.float()).sum() if float_logits else (logits * Wt.double()).sum()
    return tuple(g.numpy() for g in torch.autograd.grad(loss, (x, P, A)))


def margins(x, P, A, c):
    """(elements in the `over` arm, sqrt(mob) > maxnorm; smallest |sqrt(mob) - maxnorm| / maxnorm; smallest D0) over every finite
    (pixel, class) element"""
    with torch.no_grad():
        x, P, A = (torch.as_tensor(v).double() for v in (x, P, A))
        K, _, _, _, D0, _, _, mob = _mlr_scalars(x, P, A, c)
        maxnorm = (1.0 - PROJ_EPS_MLR) / math.sqrt(K)
        sq = torch.sqrt(mob)
        ok = torch.isfinite(sq)
        return int((sq[ok] > maxnorm).sum()), float(((sq[ok] - maxnorm).abs() / maxnorm).min()), float(D0[ok].min())


# ------------------------------------------------------------------ comparison rule
def slice_ratio(got, ref, axis, bar):
    """largest of  max_axis |got - ref| / (bar max_axis |ref| + bar 1e-3 max |ref|)  over the slices along `axis` (the channels of a
    pixel, the columns of a class row): <= 1 means every slice is within `bar` of its own largest element, with an absolute floor
    for slices whose gradient is exactly 0.  NaNs must coincide; they are then left out of both sides."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    nan = np.isnan(ref)
    if nan.all():
        return 0.0
    g, r = np.where(nan, 0.0, got), np.where(nan, 0.0, ref)
    err = np.abs(g - r).max(axis=axis)
    scale = np.abs(r).max(axis=axis)
    return float((err / (bar * scale + bar * 1e-3 * np.abs(r).max())).max())


# ------------------------------------------------------------------ inputs of the device tests
# (B, C, O, h, w, c, z's std times sqrt(C / 64), served by the fused call)
MLR_CASES = (
    (2, 64, 19, 17, 19, 1.0, 0.15, True),        # ragged last workgroup and last tile, odd O (a padding class)
    (1, 128, 7, 5, 13, 0.7, 0.15, True),         # 2 channel blocks, hw = 65
    (1, 192, 1, 4, 4, 2.0, 0.15, True),          # O = 1, hw = 16 exactly: one tile, 3 of 4 waves idle
    (1, 256, 20, 3, 11, 1.3, 0.30, True),        # 80 KiB LDS image, O = MLRB_OP, std 0.15 unscaled: 9 % of the elements beyond the limit
    (3, 64, 2, 1, 3, 1.0, 0.15, True),           # hw = 3 < 16 with B > 1
    (2, 64, 19, 90, 93, 1.0, 0.15, True),        # 1 048 tiles > 256 workgroups x 4 waves: second trip of k_mlr_bwd_dxw
    (1, 64, 3, 633, 633, 1.0, 0.15, True),       # 400 689 pixels: the scalar-weight arm of k_mlr_bwd_pixels
    (1, 8, 11, 7, 9, 1.0, 0.15, False),          # term path: a ragged second class block of the OB = 10 kernel
    (1, 48, 21, 6, 5, 0.7, 0.15, False),         # term path: 21 classes > MLRB_OP, C no multiple of 64
    (1, 320, 10, 4, 7, 1.0, 0.15, False),        # term path: C = 320 > 256
)
MLR_IDS = ["x".join(str(v) for v in case[:6]) for case in MLR_CASES]
NAN_CASE = MLR_CASES[0]


@functools.lru_cache(maxsize=None)
def mlr_case(case):
    """(x, P, A, Wt) as float64 torch CPU tensors.  z float32 normal with most pixels inside the ball, three planted pixels in image 0
    (exact origin, x40: projected, x300: tanh-clamped) and a x40 one at the very end, x = expmap_ref(z): the device's own forward is not in the loop.  Wt holds
    float32 values, so that a float32 and a float64 gout are the same numbers."""
    B, C, O, h, w, c, std, _ = case
    rng = np.random.default_rng(1000 * C + 10 * O + h)
    z = (rng.standard_normal((B, C, h * w)) * (std / math.sqrt(C / 64))).astype(np.float32)
    z[0, :, 0] = 0.0
    z[0, :, 1] *= 40.0
    z[0, :, 2] *= 300.0
    z[B - 1, :, h * w - 1] *= 40.0 if B * h * w > 3 else 1.0            # the last lane of the ragged last workgroup and tile
    with torch.no_grad():
        x = expmap_ref(torch.from_numpy(z.reshape(B, C, h, w)), c, 1).contiguous()
    bound = 1.0 / math.sqrt(C)
    P = torch.from_numpy(rng.uniform(-bound, bound, (O, C)))
    A = torch.from_numpy(rng.uniform(-bound, bound, (O, C)))
    Wt = torch.from_numpy(rng.standard_normal((B, O, h, w)).astype(np.float32).astype(np.float64))
    return x, P, A, Wt


@functools.lru_cache(maxsize=None)
def mlr_ref(case):
    """grads_ref of mlr_case(case): computed once, shared by every test of the case, never written to"""
    x, P, A, Wt = mlr_case(case)
    out = grads_ref(x, P, A, Wt, case[5])
    for g in out:
        g.setflags(write=False)
    return out


EXPMAP_CLASSES = (("origin", 0.0), ("tiny", None), ("inside", 5.0), ("projected_6.5", 6.5), ("projected_12", 12.0),
                  ("below_tanh_clamp", 14.9), ("above_tanh_clamp", 15.1), ("far", 300.0))


@functools.lru_cache(maxsize=None)
def expmap_case(shape, dim, c, f64):
    """(z, gy, {class name: pixel index along the flattened non-`dim` axes}).  Pixels 0.. of the flattened pixel axis are scaled to
    sqrt(c) ||z|| = the class's value; 'tiny' (norm 1e-16, below the 1e-15 clamp) only exists for float64 input."""
    dim = dim % len(shape)
    C = shape[dim]
    rng = np.random.default_rng(17 * C + len(shape) + (3 if f64 else 0) + int(10 * c))
    z = rng.standard_normal(shape) * (0.3 / math.sqrt(C / 8))
    zp = np.moveaxis(z, dim, -1).reshape(-1, C)                            # a copy: (pixels, C)
    planted = {}
    for k, (name, a) in enumerate(EXPMAP_CLASSES):
        if name == "tiny" and not f64:
            continue
        n = np.linalg.norm(zp[k])
        zp[k] *= 0.0 if name == "origin" else ((1e-16 if name == "tiny" else a / math.sqrt(c)) / n)
        planted[name] = k
    moved = [s for i, s in enumerate(shape) if i != dim] + [C]
    z = np.ascontiguousarray(np.moveaxis(zp.reshape(moved), -1, dim))
    z = torch.from_numpy(z if f64 else z.astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal(shape))
    return z, gy, planted


def check_planted_classes(z, c, dim, planted, f64):
    """from the reference side: every planted class of expmap_case lies where its name says (projection active or not, 1 - tanh^2
    zero or not), and every other pixel is inside the ball with every term live"""
    a, projected, gprime = expmap_pixel_classes(z, c, dim)
    a, projected, gprime = a.reshape(-1), projected.reshape(-1), gprime.reshape(-1)
    assert set(planted) == {n for n, _ in EXPMAP_CLASSES if f64 or n != "tiny"}
    for name, value in EXPMAP_CLASSES:
        if name not in planted:
            continue
        k = planted[name]
        if name == "origin":
            assert a[k] == 0.0
        elif name == "tiny":
            assert 0.0 < a[k] < 1e-15
        else:
            assert abs(a[k] - value) <= 1e-6 * value                       # float32 input: the scaling rounds
        assert projected[k] == (name not in ("origin", "tiny", "inside")), name
        assert (gprime[k] == 0.0) == (name in ("above_tanh_clamp", "far")), name
    others = np.ones(a.shape, bool)
    others[list(planted.values())] = False
    assert not projected[others].any() and (gprime[others] > 1e-3).all()   # the bulk of the pixels: inside, every term live
