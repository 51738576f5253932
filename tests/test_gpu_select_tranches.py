"""The value-binned selector's two tranches (halo_select_plan.hpp: TRANCHE_F) on the device.

Round A places and sweeps the top kfirst = halo_select_first_tranche(...) values; round B the rest of the proven bound, only for an
image whose first tranche ran out.  Every case compares picks, counts, the mutated score map and the three state maps with
oracle.halo_oracle.select_pixels_to_label bit for bit and with method="serial", and asserts through `stats` which round ran.  No F
is written down here: every input is built from halo_select_first_tranche, and the tranche a map's values fall into is worked out
on the host with the selector's own binning arithmetic (tranche_a_size)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NB1 = 2048          # coarse bins (halo_select_common.hpp)
BIN_CAP = 128       # slots of a fine bin (halo_select_binned.hip)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def kfirst_kneed(H, W, n, r):
    from halo_amd import _lib
    n = min(n, H * W)
    return int(_lib.lib().halo_select_first_tranche(H, W, n, r)), min(n * (2 * r + 1) ** 2, H * W)


def two_tranche_radius(H, W, n, r_min=2):
    """the smallest mask radius >= r_min at which this geometry has a second tranche: kfirst < kneed < H W"""
    for r in range(r_min, 15):
        kf, kn = kfirst_kneed(H, W, n, r)
        if kf < kn < H * W:
            return r
    pytest.fail("no mask radius gives %d x %d, n = %d a second tranche" % (H, W, n))


def coarse_bins(m, values):
    """coarse bin of each of `values` in map m's exact value range: k_sel_range / coarse_bin on the host, the same IEEE operations"""
    v = m[np.isfinite(m)].astype(np.float64)
    lo, hi = v.min(), v.max()
    scale = np.float64(NB1) / (hi - lo)
    return np.minimum(np.maximum((np.asarray(values, np.float64) - lo) * scale, 0.0).astype(np.int64), NB1 - 1), lo, scale


def tranche_a_size(m, kfirst):
    """(candidates of the first tranche of map m, its threshold bin t1a, about the lowest value of that bin): k_sel_scan1 on the
    host, for a map whose threshold bin is not dropped"""
    v = m[np.isfinite(m)].astype(np.float64)
    j, lo, scale = coarse_bins(m, v)
    S = np.cumsum(np.bincount(j, minlength=NB1)[::-1])[::-1]            # values in bins >= j
    ok = np.nonzero(S >= kfirst)[0]
    t1a = int(ok.max()) if len(ok) else 0
    return int(S[t1a]), t1a, float(lo + t1a / scale)


def rounds_by_the_rule(m, n, r, picks):
    """which rounds the rule of halo_select_plan.hpp runs for map m, given the reference's picks: round B iff a second tranche
    exists and the n-th pick does not lie in the first"""
    kf, kn = kfirst_kneed(m.shape[0], m.shape[1], n, r)
    t1a, t1 = tranche_a_size(m, kf)[1], tranche_a_size(m, kn)[1]
    if t1a == t1:
        return 1
    return 1 if len(picks) >= n and coarse_bins(m, picks[n - 1:n, 2])[0][0] >= t1a else 2


def staircase(ty, tx, r, dtype=np.float64, stretch=None, order=None):
    """(2r+1)^2 tiles ranked strictly; value = -(tile rank x (2r+1)^2 + rank in tile), rank 0 at the tile's centre: the greedy rule
    consumes exactly (2r+1)^2 candidates per pick -- the bound -- and pick i is the centre of the tile ranked i.  stretch: the value
    of the map's last pixel (widens the value range and with it the coarse bins)."""
    s = 2 * r + 1
    win = s * s
    inner = np.empty((s, s), np.int64)
    others = [(y, x) for y in range(s) for x in range(s) if (y, x) != (r, r)]
    inner[r, r] = 0
    for k, (y, x) in enumerate(others):
        inner[y, x] = k + 1
    rank = np.arange(ty * tx) if order is None else order
    m = -(np.kron(rank.reshape(ty, tx) * win, np.ones((s, s), np.int64)) + np.tile(inner, (ty, tx))).astype(np.float64)
    if stretch is not None:
        m.flat[np.argmin(m)] = -float(stretch)
    return m.astype(dtype)


def smooth(H, W, seed, dtype=np.float64):
    from oracle import halo_oracle as ho
    rng = np.random.default_rng(seed)
    return ho.bilinear(rng.standard_normal((1, max(2, H // 6), max(2, W // 6))), (H, W))[0].astype(dtype)


_oracle_cache = {}


def oracle(m, n, arad, r, prior, gt, key=None):
    """(picks, active, selected, active_mask, mutated map) of the reference; computed once per key"""
    from oracle import halo_oracle as ho
    if key is not None and key in _oracle_cache:
        return _oracle_cache[key]
    so, a_o = m.copy(), prior.copy()
    s_o, m_o = np.zeros(m.shape, bool), np.full(m.shape, 255, np.int64)
    po = ho.select_pixels_to_label(so, n, arad, r, a_o, s_o, m_o, gt, True)[-1]
    out = (np.ascontiguousarray(po), a_o, s_o, m_o, so)
    if key is not None:
        _oracle_cache[key] = out
    return out


def run(dev, maps, n, r, arad=1, method=None, stream=None, score_range=None, seed=5):
    """one call on a batch of maps -> per-image results + handover + stats (host arrays)"""
    from halo_amd.core.active.build import greedy_select
    maps = np.ascontiguousarray(np.stack(maps))
    B, H, W = maps.shape
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, 19, (B, H, W)).astype(np.int64)
    prior = rng.random((B, H, W)) < 0.02
    s = t(maps, dev).clone()
    act, sel = t(prior, dev).clone(), torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    am = torch.full((B, H, W), 255, dtype=torch.int64, device=dev)
    hov = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    st = torch.full((B, 3), -1, dtype=torch.int32, device=dev)
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
    with ctx:
        picks, npk = greedy_select(s, n, arad, r, act, sel, am, t(gt, dev), method=method, handover=hov, stats=st, score_range=score_range)
    return dict(maps=maps, gt=gt, prior=prior, s=s, act=act, sel=sel, am=am, hov=hov, st=st, picks=picks, npk=npk, n=n, r=r, arad=arad)


def same_as_oracle(res, keys=None):
    maps, B = res["maps"], res["maps"].shape[0]
    got = {k: res[k].cpu().numpy() for k in ("s", "act", "sel", "am", "picks", "npk")}
    for b in range(B):
        po, a_o, s_o, m_o, so = oracle(maps[b], res["n"], res["arad"], res["r"], res["prior"][b], res["gt"][b], None if keys is None else keys[b])
        k = int(got["npk"][b])
        assert k == len(po), (b, k, len(po))
        assert bits_equal(got["picks"][b, :k], po), (b, "picks")
        assert np.array_equal(got["act"][b], a_o) and np.array_equal(got["sel"][b], s_o) and np.array_equal(got["am"][b], m_o), (b, "maps")
        assert bits_equal(got["s"][b], so), (b, "score")


def same_as_serial(dev, res):
    ser = run(dev, list(res["maps"]), res["n"], res["r"], res["arad"], method="serial")
    assert torch.equal(ser["npk"], res["npk"])
    assert bits_equal(ser["picks"].cpu().numpy(), res["picks"].cpu().numpy())
    for k in ("act", "sel", "am"):
        assert torch.equal(ser[k], res[k]), k
    assert bits_equal(ser["s"].cpu().numpy(), res["s"].cpu().numpy())
    assert int(ser["st"].abs().sum()) == 0                       # the sweep did not run: zeros


def check(dev, maps, n, r, rounds, reasons=("done",), arad=1, keys=None):
    """rounds: what `stats` must report per image; None = what rounds_by_the_rule says for the reference's picks"""
    from halo_amd import _lib
    res = run(dev, maps, n, r, arad)
    same_as_oracle(res, keys)
    same_as_serial(dev, res)
    st, hov = res["st"].cpu().numpy(), res["hov"].cpu().numpy()
    if rounds is None:
        rounds = [rounds_by_the_rule(res["maps"][b], n, r, oracle(res["maps"][b], n, arad, r, res["prior"][b], res["gt"][b])[0])
                  for b in range(len(maps))]
    if isinstance(rounds, int):
        rounds = [rounds] * len(maps)
    if isinstance(reasons[0], str):
        reasons = [reasons] * len(maps)
    for b in range(len(maps)):
        print("image %d: placed %d consumed %d rounds %d reason %s sweep picks %d" % (b, st[b, 0], st[b, 1], st[b, 2],
                                                                                      _lib.SWEEP_REASONS[hov[b, 0]], hov[b, 1]))
        assert st[b, 2] == rounds[b], (b, st[b], rounds[b])
        assert _lib.SWEEP_REASONS[hov[b, 0]] in reasons[b], (b, _lib.SWEEP_REASONS[hov[b, 0]], reasons[b])
        assert 0 <= st[b, 1] <= st[b, 0]
    return res, st, hov


# ---------------------------------------------------------------- geometry of the staircase cases
TY, TX = 14, 18


def stair_geom(n):
    r = two_tranche_radius(TY * 7, TX * 7, n, 3)                 # the tile side follows the radius; 7 only sizes the search
    s = 2 * r + 1
    return r, s * s, TY * s, TX * s


def find_stair_case(want):
    """(n, stretch, size of tranche A) of a staircase in which round A ends `want`: 'exact' = the n-th pick is its last candidate,
    'short' = one pick short of n when it runs out.  Searched, so that it holds for whatever F the library was built with."""
    for n in range(2, TY * TX):
        r, win, H, W = stair_geom(n)
        kf, kn = kfirst_kneed(H, W, n, r)
        if not kf < kn < H * W:
            continue
        for stretch in (None, win * NB1, 2 * win * NB1, 3 * win * NB1, 5 * win * NB1, 8 * win * NB1):
            size = tranche_a_size(staircase(TY, TX, r, stretch=stretch), kf)[0]
            picks_a = -(-size // win)                            # pick i is candidate i * win
            if (want == "exact" and size == win * (n - 1) + 1) or (want == "short" and picks_a == n - 1 and size < kn):
                return n, stretch, size
    pytest.fail("no staircase case '%s' for the built first tranche" % want)


# ---------------------------------------------------------------- cases
def test_round_a_suffices(dev):
    H, W, n = 96, 128, 60
    r = two_tranche_radius(H, W, n, 2)
    kf, kn = kfirst_kneed(H, W, n, r)
    assert kf < kn < H * W
    _, st, _ = check(dev, [smooth(H, W, 1)], n, r, rounds=1)
    assert st[0, 0] == tranche_a_size(smooth(H, W, 1), kf)[0] >= kf          # only the first tranche was placed


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_round_b_forced_without_ties(dev, dtype):
    n = 40
    r, win, H, W = stair_geom(n)
    kf, kn = kfirst_kneed(H, W, n, r)
    assert kf < kn < H * W
    res, st, hov = check(dev, [staircase(TY, TX, r, dtype)], n, r, rounds=2)
    assert int(res["npk"][0]) == n and hov[0, 1] == n
    assert st[0, 1] >= kf                                         # all of tranche A was consumed, then some of B
    pk = res["picks"][0].cpu().numpy()
    s = 2 * r + 1
    assert np.array_equal(pk[:, 0], (np.arange(n) // TX) * s + r) and np.array_equal(pk[:, 1], (np.arange(n) % TX) * s + r)


def test_round_a_ends_exactly_at_its_last_candidate(dev):
    n, stretch, size = find_stair_case("exact")
    r, win, H, W = stair_geom(n)
    res, st, _ = check(dev, [staircase(TY, TX, r, stretch=stretch)], n, r, rounds=1)
    assert int(res["npk"][0]) == n and st[0, 0] == size


def test_round_a_ends_one_pick_short(dev):
    n, stretch, size = find_stair_case("short")
    r, win, H, W = stair_geom(n)
    res, st, hov = check(dev, [staircase(TY, TX, r, stretch=stretch)], n, r, rounds=2)
    assert int(res["npk"][0]) == n and st[0, 0] > size


def test_one_tranche_when_kfirst_is_kneed(dev):
    """a staircase whose windows are no larger than the first tranche's share per pick: kfirst == kneed, one tranche, and round B
    returns at once although the map is the worst case"""
    n = 40
    for r in range(14, 0, -1):
        s = 2 * r + 1
        kf, kn = kfirst_kneed(TY * s, TX * s, n, r)
        if kf == kn < TY * TX * s * s:
            break
    else:
        pytest.fail("no mask radius with kfirst == kneed")
    res, st, _ = check(dev, [staircase(TY, TX, r)], n, r, rounds=1)
    assert int(res["npk"][0]) == n and st[0, 1] >= (n - 1) * s * s + 1


def test_values_on_the_coarse_bin_edge_at_t1a(dev):
    """values equal to, just below and just above the edge of the first tranche's threshold bin, many of each: the candidates of
    one coarse bin are never split between the rounds"""
    n = 40
    r, win, H, W = stair_geom(n)
    kf, kn = kfirst_kneed(H, W, n, r)
    base = staircase(TY, TX, r)
    _, t1a, edge = tranche_a_size(base, kf)
    m = base.copy()
    rng = np.random.default_rng(3)
    lo, hi = base.min(), base.max()
    idx = rng.choice(H * W - 2, 90, replace=False) + 1            # keeps the extrema (first and last pixel of the ranking) in place
    vals = [edge, np.nextafter(edge, -np.inf), np.nextafter(edge, np.inf)]
    keep = (m.flat[idx] != lo) & (m.flat[idx] != hi)
    m.flat[idx[keep]] = np.resize(vals, int(keep.sum()))
    assert m.min() == lo and m.max() == hi
    assert kf < kn < H * W and int((m == edge).sum()) >= 20
    check(dev, [m, base], n, r, rounds=None)


def plateau_in_tranche_b(r, n):
    """a staircase whose tiles ranked n - 8 .. n - 3 all carry one value: a plateau of ties deep inside tranche B"""
    s = 2 * r + 1
    m = staircase(TY, TX, r)
    for k in range(n - 8, n - 2):
        y, x = (k // TX) * s, (k % TX) * s
        m[y:y + s, x:x + s] = -float((n - 8) * s * s)
    return m


def test_batch_mixing_rounds_and_hand_overs(dev):
    n = 60
    r, win, H, W = stair_geom(n)
    kf, kn = kfirst_kneed(H, W, n, r)
    assert kf < kn and 6 * win > BIN_CAP and (n - 8) * win > kf + win      # the plateau overflows a bin, and lies behind tranche A
    masked = np.full((H, W), -np.inf)
    nan = smooth(H, W, 4)
    nan[H // 2, W // 3] = np.nan
    maps = [smooth(H, W, 2), staircase(TY, TX, r), masked, nan, plateau_in_tranche_b(r, n)]
    res, st, hov = check(dev, maps, n, r, rounds=[1, 2, 1, 1, 2],
                         reasons=[("done",), ("done",), ("bad_values",), ("bad_values",), ("done", "bin_overflow", "survivors")])
    assert hov[2, 1] == 0 and hov[3, 1] == 0 and hov[4, 1] >= n - 8


def stale_histogram_case(dev):
    """(score maps, range records, n, r) of a batch whose maps the caller masked AFTER the scorer counted them"""
    from halo_amd.core.active.floating_region import new_score_range, score_maps
    from oracle import halo_oracle as ho
    rng = np.random.default_rng(13)
    B, C, O, H, W = 3, 8, 19, 96, 160
    emb = ho.bilinear(ho.expmap((rng.standard_normal((B, C, H // 4, W // 4)) * 0.2).astype(np.float32), 1.0, dim=1), (H, W))
    logit = ho.bilinear(rng.standard_normal((B, O, H // 4, W // 4)).astype(np.float32), (H, W))
    rec = new_score_range(B, dev)
    act = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    sc = score_maps(t(logit, dev), t(emb, dev), "entropy", "radius", True, None, size=3, active=act, want_maps=False, score_range=rec)[0]
    sc[:, : int(H * 0.6)] = -float("inf")
    return sc, rec, 120, 5                      # kneed = 14520 < H W: the threshold bin lies above bin 0, so the stale counts matter


# what the one-tranche selector (the parent of this change) reports for this batch: reason, and the picks its sweep made per image
STALE_PARENT = {"reasons": ["exhausted", "exhausted", "done"], "picks": [118, 118, 120]}


def test_round_b_then_exhausted(dev):
    """a stale scorer histogram: fewer candidates than the counts promise in BOTH tranches -> round B runs and, in two of the three
    images, runs out as well: they are handed over as `exhausted` from the pick at which the one-tranche sweep handed them over
    (the sweep's picks are the reference's picks among all the candidates above t1, however those are split into rounds); the third
    image reaches n_regions with its last candidates, in round B"""
    from halo_amd import _lib
    from halo_amd.core.active.build import greedy_select
    sc, rec, n, r = stale_histogram_case(dev)
    B, H, W = sc.shape
    kf, kn = kfirst_kneed(H, W, n, r)
    assert kf < kn < H * W
    maps = sc.cpu().numpy()
    gt = np.zeros((B, H, W), np.int64)
    act = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    sel, am = torch.zeros_like(act), torch.full((B, H, W), 255, dtype=torch.int64, device=dev)
    hov = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    st = torch.full((B, 3), -1, dtype=torch.int32, device=dev)
    picks, npk = greedy_select(sc, n, 1, r, act, sel, am, t(gt, dev), score_range=rec, handover=hov, stats=st)
    res = dict(maps=maps, gt=gt, prior=np.zeros((B, H, W), bool), s=sc, act=act, sel=sel, am=am, picks=picks, npk=npk, n=n, r=r, arad=1)
    same_as_oracle(res)
    # and the serial kernel alone on the same (masked) maps
    s2, a2 = t(maps, dev).clone(), torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    l2, m2 = torch.zeros_like(a2), torch.full((B, H, W), 255, dtype=torch.int64, device=dev)
    p2, n2 = greedy_select(s2, n, 1, r, a2, l2, m2, t(gt, dev), method="serial")
    assert torch.equal(n2, npk) and bits_equal(p2.cpu().numpy(), picks.cpu().numpy())
    assert torch.equal(a2, act) and torch.equal(l2, sel) and torch.equal(m2, am) and bits_equal(s2.cpu().numpy(), sc.cpu().numpy())
    hov, st = hov.cpu().numpy(), st.cpu().numpy()
    print("stale histogram: handover", hov.tolist(), "stats", st.tolist())
    for b in range(B):
        assert _lib.SWEEP_REASONS[hov[b, 0]] == STALE_PARENT["reasons"][b] and st[b, 2] == 2, (b, hov[b], st[b])
        assert int(npk[b]) >= hov[b, 1]
    assert hov[:, 1].tolist() == STALE_PARENT["picks"]


def test_late_round_blocks_and_more_regions_than_pixels(dev):
    """-inf blocks as earlier rounds leave them (whole tiles, so the staircase argument holds for the rest), and n_regions above
    what can be picked: the sweep runs out of candidates in both rounds and the count is the reference's"""
    n = 40
    r, win, H, W = stair_geom(n)
    s = 2 * r + 1
    m = staircase(TY, TX, r)
    rng = np.random.default_rng(8)
    for k in rng.choice(TY * TX, TY * TX // 2, replace=False):
        y, x = (k // TX) * s, (k % TX) * s
        m[y:y + s, x:x + s] = -np.inf
    res, st, _ = check(dev, [m], n, r, rounds=2)
    assert int(res["npk"][0]) == n
    big = TY * TX + 50                                            # more regions than tiles: every tile centre, then nothing
    kf, kn = kfirst_kneed(H, W, big, r)
    assert big * win > H * W and kf < kn == H * W
    order = np.random.default_rng(9).permutation(TY * TX)
    res, st, _ = check(dev, [staircase(TY, TX, r), staircase(TY, TX, r, order=order)], big, r, rounds=2)
    assert res["npk"].tolist() == [TY * TX, TY * TX]


def test_three_calls_back_to_back_share_one_workspace(dev):
    """round-B image, round-A image, round-B image on a side stream, no synchronisation between them, one workspace: what a call
    leaves in the header, the bin counters or the pick list must not show in the next"""
    n = 40
    r, win, H, W = stair_geom(n)
    order = np.random.default_rng(2).permutation(TY * TX)
    seq = [staircase(TY, TX, r), smooth(H, W, 6), staircase(TY, TX, r, order=order)]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    out = [run(dev, [m], n, r, stream=side) for m in seq]
    side.synchronize()
    for res, rounds in zip(out, (2, 1, 2)):
        same_as_oracle(res)
        same_as_serial(dev, res)
        assert int(res["st"][0, 2]) == rounds and int(res["hov"][0, 0]) == 0


def test_graph_replay_of_both_rounds(dev):
    from halo_amd.core.active.build import greedy_select
    n = 40
    r, win, H, W = stair_geom(n)
    maps = np.stack([smooth(H, W, 7), staircase(TY, TX, r)])
    eager = run(dev, list(maps), n, r)
    same_as_oracle(eager)
    same_as_serial(dev, eager)
    assert eager["st"][:, 2].tolist() == [1, 2]
    src, gt, prior = t(maps, dev), t(eager["gt"], dev), t(eager["prior"], dev)
    score, act, sel = src.clone(), prior.clone(), torch.zeros_like(prior)
    am = torch.full(maps.shape, 255, dtype=torch.int64, device=dev)
    picks, npk = torch.zeros((2, n, 3), dtype=torch.float64, device=dev), torch.zeros((2,), dtype=torch.int32, device=dev)
    hov, st = torch.zeros((2, 2), dtype=torch.int32, device=dev), torch.zeros((2, 3), dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        greedy_select(score, n, 1, r, act, sel, am, gt, out=(picks, npk), handover=hov, stats=st)      # warm-up: workspace, LDS limit
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            greedy_select(score, n, 1, r, act, sel, am, gt, out=(picks, npk), handover=hov, stats=st)
    for rep in range(3):
        score.copy_(src); act.copy_(prior); sel.zero_(); am.fill_(255); picks.zero_(); npk.zero_(); hov.fill_(-1); st.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(npk, eager["npk"]) and bits_equal(picks.cpu().numpy(), eager["picks"].cpu().numpy()), rep
        assert torch.equal(act, eager["act"]) and torch.equal(sel, eager["sel"]) and torch.equal(am, eager["am"]), rep
        assert bits_equal(score.cpu().numpy(), eager["s"].cpu().numpy()), rep
        assert torch.equal(st, eager["st"]) and torch.equal(hov, eager["hov"]), rep
