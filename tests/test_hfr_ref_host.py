"""CPU checks of what tests/test_gpu_hfr_routes.py stands on (no device): hfr_cases.py's constants are halo_hfr.hip's and each case
reaches the edge its row names; hfr_ref.py's float64 statement is halo_amd.hfr.torch_statement run in float64; every case is
admissible (zero knife edges, hfr_ref.py's three conditions) and the float32 stock chain agrees with float64 on every ReLU and clamp
bit; the yardstick rho* (the stock chain's worst group per tensor) is printed; the bars 2 rho* reject seven seeded errors; the
workspace query and the entry points' range checks accept every case."""
import os
import re

import numpy as np
import pytest
import torch

import hfr_cases as hc
import hfr_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1                                     # HALO_E_ARG of include/halo_hip.h
MARGIN = 2.0                                   # the device bar: rho_dev <= MARGIN * rho* (tests/test_gpu_hfr_routes.py says why)


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "halo_amd", "csrc", "halo_hfr.hip")).read()
    for name in ("HT", "HCW", "HSEG", "HDOT", "H_MAX_C"):
        (v,) = re.findall(r"constexpr int %s = (\d+);" % name, src)
        assert int(v) == getattr(hc, name), name
    assert "blockIdx.y * HT * 4" in src and "cdiv(P, HT * 4)" in src and hc.SCALE_CHUNK == 4 * hc.HT      # k_hfr_scale's chunk
    assert "C == 64" in src                                                                                # the register arm's width


@pytest.mark.parametrize("name", list(hc.CASES))
def test_case_reaches_its_edge(name):
    (B, C, h, w), modes, _, claim = hc.CASES[name]
    P = h * w
    f = hc.split_facts(B, C, P)
    assert {k: f[k] for k in claim} == claim
    assert f["arm"] == ("register" if name.startswith("c64_") else "generic")
    checks = {
        "c64_p257": f["nblk"] == 2 and f["tail"] == 1,
        "c64_p511": f["tail"] == hc.HT - 1,
        "c64_p768": P % hc.HT == 0 and f["nblk"] > 1,
        "c64_p1025": f["scale_blocks"] == 2 and f["last_chunk"] == 1 and 1 < f["nblk"] < hc.HSEG and f["empty_segments_fwd"] > 0,
        "c64_p4252_b1": B == 1 and f["nblk"] == hc.HSEG + 1 and 0 < f["tail"] < hc.HT,
        "c64_p7_b3": P < hc.HDOT and f["empty_splits"] > 0 and B > 2,
        "c64_p1_b3": P == 1 and B * P > 1,
        "c64_p2043_b33": f["R"] > hc.HT and f["R"] - B < hc.HT + 1 and B * C > hc.HT and B > hc.HSEG and 0 < f["tail"] < hc.HT,
        "c10_p257": C % hc.HCW != 0 and C > hc.HCW and f["tail"] == 1,
        "c3_p1025": C < hc.HCW and f["scale_blocks"] == 2,
        "c72_p511": C > 64 and C % hc.HCW == 0 and f["tail"] == hc.HT - 1,
        "c256_p300": C == hc.H_MAX_C and 0 < f["tail"] < hc.HT,
        "c10_p257_b4": B == 4 and C % hc.HCW != 0,
    }
    assert checks[name]
    assert set(modes) <= set(hr.MODES)
    if name in ("c64_p257", "c64_p1025", "c10_p257"):
        assert set(modes) == set(hr.MODES)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_case_marks(name):
    """two channels clamped by b2 = -10, none by luck, one all-zero plane of x in the last image; where the last tile is partial the
    zero plane and the clamped channel C - 1 have pixels in it (every image's last tile is the partial one)"""
    case = hc.build(name)
    (B, C, h, w), modes = hc.CASES[name][0], hc.CASES[name][1]
    clamped, (zb, zc) = case["clamped"], case["zero"]
    assert len(clamped) >= 2 and zb == B - 1 and all(case["b2"][c] == -10.0 for c in clamped)
    zero = np.abs(case["x"]).reshape(B, C, -1).max(-1) == 0
    assert zero.sum() == 1 and zero[zb, zc]
    for mode in modes:
        ref = hc.held(name, mode)[0]
        is_clamped = ref["w"] < hr.CLAMP
        assert is_clamped[:, list(clamped)].all() and is_clamped.sum() == B * len(clamped), mode
        assert (ref["wc"][:, list(clamped)] == hr.CLAMP).all()
    if C == 64:
        assert 40 not in clamped                                            # the rejection test zeroes row 40 of g_W2


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in hc.case_modes() if hc.CASES[n][0][0] < 33])
def test_reference_is_the_torch_statement_in_float64(name, mode):
    """hfr_ref.reference writes the statement out operator by operator; torch's own modules in float64 give the same numbers (every
    case but the 33-image one, which has no operator or mode of its own and costs as much as the others together)"""
    from halo_amd.hfr import torch_statement
    case = hc.build(name)
    ref = hc.held(name, mode)[0]
    got, mlp, _ = hr.run_statement(torch_statement, case, mode, dtype=torch.float64)
    for T in hr.TENSORS:
        if T not in ref:
            assert T not in got
            continue
        s = np.abs(ref["g_W1" if T == "g_b1" else T]).max()                      # g_b1 is rounding noise under batch statistics
        assert np.abs(got[T] - ref[T]).max() <= 1e-11 * s, T
    bn = mlp[1]
    if hr.updates(mode):
        assert int(bn.num_batches_tracked) == hc.NUM_BATCHES_TRACKED + 1
    elif bn.track_running_stats:
        assert int(bn.num_batches_tracked) == hc.NUM_BATCHES_TRACKED


@pytest.mark.parametrize("name,mode", hc.case_modes())
def test_admissible_and_the_stock_chain_agrees_on_every_bit(name, mode):
    _, adm, _, differ = hc.held(name, mode)
    print("%s %s: min |z| / tau %.2f, min |w - 1e-5| / dw %.3g, min w / Sw (unclamped) %.3f, nudged values %d"
          % (name, mode, adm["min_z_over_tau"], adm["min_clamp_over_dw"], adm["min_w_over_Sw"], hc.build(name)["nudged"]))
    assert len(adm["relu"]) == 0, adm["relu"][:5]
    assert len(adm["clamp"]) == 0, adm["clamp"][:5]
    assert len(adm["cond"]) == 0, adm["cond"][:5]
    assert differ == (0, 0)


def test_yardstick_table():
    """rho*_T, the float32 stock chain's worst group over every case and mode: printed (NOTES.md records it), finite, and below
    what no float32 chain of this length could exceed while still being one (C + 2 + log2 N roundings do not reach 1e-2)"""
    yard = hc.yardstick()
    print("\n| tensor | rho* (stock float32 chain, worst group) | where |\n|---|---|---|")
    for T in hr.TENSORS:
        print("| `%s` | %.3e | %s |" % (T, yard[T][0], yard[T][1]))
    assert set(yard) == set(hr.TENSORS)
    for T, (r, _) in yard.items():
        assert 0 < r < 1e-2 and np.isfinite(r), T


# the tensor that has to catch each slip (more may); for the last two also the group
CATCHES = {
    "stats_skip_last_pixel": ("running_mean", None),
    "mean_r_skip_last_pixel": ("y", None),
    "tail_counts_over_full_tile": ("g_beta", None),
    "coef_of_image0_for_image1": ("g_x", None),
    "g_W1_drops_last_part_row": ("g_W1", None),
    "clamped_y_times_2": ("y", "channel 1"),
    "g_W2_row40_zeroed": ("g_W2", "row 40"),
}


@pytest.mark.parametrize("fault", hr.FAULTS)
def test_seeded_error_is_rejected(fault):
    """the correct float64 results with one slip in them, against the device's bars: some group of some tensor exceeds 2 rho*"""
    name, mode = "c64_p257", "train"
    case = hc.build(name)
    ref = hc.held(name, mode)[0]
    yard = hc.yardstick()
    wrong = hr.reference(case, mode, fault=fault, tile=hc.HT)
    res = hr.rho(ref, {T: wrong[T] for T in hr.TENSORS})
    caught = {T: (r, where) for T, (r, where) in res.items() if r > MARGIN * yard[T][0]}
    print("%s: caught by %s" % (fault, ", ".join("%s (%s, %.2e = %.3g rho*)" % (T, w, r, r / yard[T][0]) for T, (r, w) in caught.items())))
    T, group = CATCHES[fault]
    assert T in caught, (fault, res)
    if group:
        assert group in caught[T][1] and set(caught) == {T}
    # and the unspoilt reference passes its own comparison exactly
    assert all(r == 0.0 for r, _ in hr.rho(ref, {T: ref[T] for T in hr.TENSORS if T in ref}).values())


@pytest.mark.parametrize("name", list(hc.CASES))
def test_workspace_and_ranges(name):
    from halo_amd import _lib
    L = _lib.lib()
    (B, C, h, w) = hc.CASES[name][0]
    P = h * w
    f = hc.split_facts(B, C, P)
    n = L.halo_hfr_workspace_bytes(B, C, P)
    assert n >= f["R"] * (C * C + C) * 4 + f["R"] * (2 + 4) * C * 8 + (0 if C == 64 else B * C * P * 4)
    # hfr_check's ranges, restated, and the entry points' own answer: with the shape accepted they go on to refuse the null operands
    assert -(-P // hc.SCALE_CHUNK) <= 65535 and B <= 65535 and B * C < 2 ** 31 and C <= hc.H_MAX_C
    assert L.halo_hfr_fwd_stats(None, B, C, P, None, None, None, None, n, None) == E_ARG
    assert "null argument" in L.halo_last_error().decode()
    assert L.halo_hfr_bwd_apply(None, B, C, P, None, None, None, None, None, None, None, None, None, n, None) == E_ARG
    assert "null argument" in L.halo_last_error().decode()
