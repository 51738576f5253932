"""k_feat_reduce's result stores (feat_store in halo_score.hip): the 16-byte radius store of the two- and four-pixel routes
leaves the chip under a cache policy of its own, through a buffer descriptor that covers the chunk's pixels inside the map.
Whatever the policy, every byte of the three maps is what the one-pixel route (plain stores, stand-alone entropy kernel)
and the CPU oracle compute, and it is there when the next kernel on the stream reads it.

Each shape is the smallest that reaches one edge of the store code: a block with 33 live lanes and hw % 4 == 2, one live
lane in a second block (float64: 256-pixel chunks, float32: 512), a chunk count that halves the granule and leaves one chunk
on the plain map, several granule groups with both entropy orders, the class counts with and without the fused entropy, the
Euclidean norm."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _offset_copy(x, off=1):
    """x's values one element past the start of a larger allocation: no longer 16-byte aligned, so the one-pixel route"""
    buf = torch.empty(x.numel() + off, dtype=x.dtype, device=x.device)
    v = buf[off:].view(x.shape)
    v.copy_(x)
    return v


def _batch_view(x, lead, pad):
    """x's values as a view of a larger allocation: `lead` elements in front, `pad` elements between two images"""
    B, per = x.shape[0], x[0].numel()
    buf = torch.full((lead + B * (per + pad),), float("nan"), dtype=x.dtype, device=x.device)
    v = torch.as_strided(buf, x.shape, (per + pad,) + tuple(x.stride()[1:]), lead)
    v.copy_(x)
    return v


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _inputs(H, W, dt, C, O, seed):
    rng = np.random.default_rng(seed)
    logit = rng.standard_normal((2, O, H, W)).astype(np.float32)
    emb = (rng.standard_normal((2, C, H, W)) * 0.05).astype(dt)
    return logit, emb


def _check(dev, H, W, dt, C, O=19, pur="radius", norm=True, seed=2600):
    from halo_amd.core.active.floating_region import score_maps
    from oracle import halo_oracle as ho
    logit, emb = _inputs(H, W, dt, C, O, seed)
    lg, em = t(logit, dev), t(emb, dev)
    assert em.data_ptr() % 16 == 0
    new = score_maps(lg, em, "entropy", pur, norm, None, size=3)
    old = score_maps(lg, _offset_copy(em), "entropy", pur, norm, None, size=3)
    for name, x, y in zip(("score", "impurity", "uncertainty"), new, old):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy()), (name, "one-pixel route", H, W, dt, C, O, pur)
    so, io, uo = ho.floating_region_score(logit[1:2], emb[1:2], "entropy", pur, norm, None, size=3, purity_type=pur)
    for name, x, y in zip(("score", "impurity", "uncertainty"), new, (so, io, uo)):
        assert bits_equal(x[1].cpu().numpy(), y), (name, "oracle", H, W, dt, C, O, pur)
    return new


@pytest.mark.parametrize("H,W,dt,C", [
    (6, 11, np.float64, 3),       # one block, 33 live lanes, hw % 4 == 2
    (1, 258, np.float64, 8),      # one full chunk plus one live lane in the second block
    (17, 256, np.float64, 11),    # 17 chunks: granule halved to 2, one chunk on the plain map, channel remainder after one unrolled trip
    (4, 129, np.float32, 9),      # hw = 516: one full 512-pixel chunk plus one live lane
    (40, 72, np.float64, 8),      # several granule groups, both entropy orders
    (40, 72, np.float32, 8),
], ids=["6x11-f64", "1x258-f64", "17x256-f64", "4x129-f32", "40x72-f64", "40x72-f32"])
def test_store_edges_match_the_one_pixel_route_and_the_oracle(dev, H, W, dt, C):
    _check(dev, H, W, dt, C)


@pytest.mark.parametrize("O", [16, 7], ids=["O16-fused-entropy", "O7-radius-store-alone"])
def test_class_counts_with_and_without_the_fused_entropy(dev, O):
    _check(dev, 24, 64, np.float64, 8, O=O)


def test_euclidean_norm_not_normalised(dev):
    _check(dev, 24, 64, np.float64, 8, pur="euc_norm", norm=False)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_batches_as_views_of_larger_allocations(dev, dt):
    """batch stride larger than C * hw, bases 16-byte but not 128-byte aligned"""
    from halo_amd.core.active.floating_region import score_maps
    H, W, C = 40, 72, 8
    logit, emb = _inputs(H, W, dt, C, 19, 2601)
    lg, em = t(logit, dev), t(emb, dev)
    want = score_maps(lg, em, "entropy", "radius", True, None, size=3)
    per16 = 16 // em.element_size()
    emv, lgv = _batch_view(em, per16, 3 * per16), _batch_view(lg, 4, 12)
    assert emv.data_ptr() % 16 == 0 and emv.data_ptr() % 128 != 0 and emv.stride(0) > C * H * W
    assert lgv.data_ptr() % 16 == 0 and lgv.data_ptr() % 128 != 0 and lgv.stride(0) > 19 * H * W
    got = score_maps(lgv, emv, "entropy", "radius", True, None, size=3)
    for x, y in zip(got, want):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
    assert bits_equal(got[0].cpu().numpy(), score_maps(lg, _offset_copy(em), "entropy", "radius", True, None, size=3)[0].cpu().numpy())


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_stores_are_complete_at_the_kernel_boundary(dev, dt):
    """three calls back to back on a side stream, each with its own outputs and workspace: the tail kernels of a call read
    the maps its feature pass has just stored"""
    from halo_amd.core.active.floating_region import score_maps, score_workspace
    H, W, C, B = 40, 72, 8, 2
    logit, emb = _inputs(H, W, dt, C, 19, 2602)
    lg, em = t(logit, dev), t(emb, dev)
    odt = em.dtype
    side = torch.cuda.Stream(dev)
    sets = [(torch.full((B, H, W), float("nan"), dtype=odt, device=dev), torch.full((B, H, W), float("nan"), dtype=odt, device=dev),
             torch.full((B, H, W), float("nan"), dtype=torch.float32, device=dev), score_workspace(B, H, W, dev)) for _ in range(3)]
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        got = [score_maps(lg, em, "entropy", "radius", True, None, size=3, out=o, maps=(i, u), workspace=ws) for o, i, u, ws in sets]
    side.synchronize()
    for k in (1, 2):
        for x, y in zip(got[k], got[0]):
            assert bits_equal(x.cpu().numpy(), y.cpu().numpy()), k
    ref = score_maps(lg, _offset_copy(em), "entropy", "radius", True, None, size=3)
    for x, y in zip(got[0], ref):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
