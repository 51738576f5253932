"""halo_select_first_tranche, the host query behind the selector's two tranches, and the workspace query, which the tranches must
not change: no device is touched."""
import pytest

GEOMS = [(1024, 2048, 2331, 5), (1024, 2048, 2331, 3), (512, 1024, 600, 5), (96, 128, 60, 2), (7, 300, 900, 1), (260, 420, 300, 14)]

# halo_select_workspace_bytes(B, H, W, n_regions, mask_radius) of the one-tranche selector this change started from: the bench
# geometry (16 images) and three small ones
WORKSPACE_BEFORE = {
    (16, 1024, 2048, 2331, 5): 270989568,
    (1, 96, 128, 60, 2): 3513344,
    (5, 98, 126, 40, 3): 17560576,
    (3, 7, 300, 900, 1): 9800192,
}


def L():
    from halo_amd import _lib
    return _lib.lib()


def kneed(H, W, n, r):
    return min(min(n, H * W) * (2 * r + 1) ** 2, H * W)


def test_first_tranche_is_a_pure_host_function():
    """same answer every time, for any sizes (no stream, no pointer in its signature), and nothing for an empty question"""
    from halo_amd import _lib
    assert _lib.SIGNATURES["halo_select_first_tranche"][1] == [_lib._i64] * 4
    for g in GEOMS:
        assert L().halo_select_first_tranche(*g) == L().halo_select_first_tranche(*g) > 0
    assert L().halo_select_first_tranche(0, 10, 5, 2) == 0 and L().halo_select_first_tranche(10, 10, 0, 2) == 0


@pytest.mark.parametrize("geom", GEOMS)
def test_first_tranche_never_exceeds_the_bound(geom):
    H, W, n, r = geom
    for k in (1, 2, n // 2 + 1, n, 4 * n, H * W, H * W + 7):
        assert 0 < L().halo_select_first_tranche(H, W, k, r) <= kneed(H, W, k, r)


@pytest.mark.parametrize("geom", GEOMS)
def test_first_tranche_is_monotone_in_n_regions(geom):
    H, W, n, r = geom
    prev = 0
    for k in list(range(1, 40)) + list(range(40, min(4 * n, H * W) + 2, max(1, n // 13))):
        cur = L().halo_select_first_tranche(H, W, k, r)
        assert cur >= prev, (k, cur, prev)
        prev = cur


@pytest.mark.parametrize("geom", GEOMS)
def test_first_tranche_is_the_bound_where_the_share_per_pick_covers_it(geom):
    """kfirst = min(kneed, n_regions x F): F is read off a question small enough not to be capped, and then predicts every other"""
    H, W, n, r = geom
    F = L().halo_select_first_tranche(4096, 4096, 1, 14)            # one pick, an 841-pixel window: min(841, F)
    assert 0 < F < 841
    for k in (1, 3, n, 2 * n, H * W):
        k = min(k, H * W)
        want = min(kneed(H, W, k, r), k * F)
        assert L().halo_select_first_tranche(H, W, k, r) == want
        if k * F >= kneed(H, W, k, r):
            assert L().halo_select_first_tranche(H, W, k, r) == kneed(H, W, k, r)


def test_workspace_query_is_unchanged():
    for args, want in WORKSPACE_BEFORE.items():
        assert L().halo_select_workspace_bytes(*args) == want, args
