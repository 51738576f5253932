"""CPU checks of the HFR weighted normalisation (halo_hfr.hip, halo_amd.hfr, halo_amd.hooks.use_fused_feature_reweighting): the
fixture's float32 reference meets the bars the device is held to against its own float64 evaluation, the entry points are
declared, listed and exported, the workspace query is host code, the argument checks refuse before any launch, and the
envelope, the fallback and the hook binding.  The kernels themselves are held to the fixture in tests/test_gpu_hfr.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "hfr.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("halo_hfr_workspace_bytes", "halo_hfr_fwd_stats", "halo_hfr_fwd_apply", "halo_hfr_bwd_reduce", "halo_hfr_bwd_apply")
PARAMS = ("W1", "b1", "gamma", "beta", "W2", "b2")


def case(name):
    z = np.load(FIX)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


def cases():
    z = np.load(FIX)
    return sorted({k.split("/")[0] for k in z.files})


def rel_err(got, want, scale=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), scale, 1e-300)


@pytest.mark.parametrize("name", cases())
def test_float32_reference_meets_the_device_bars(name):
    """the stock float32 chain of the reference head against its float64 evaluation: the bars of tests/test_gpu_hfr.py
    (y 2e-6 of max|y|, gradients 2e-5 of max|g|, an all-zero channel of d x to its own max, running stats 2e-6) are met"""
    d = case(name)
    assert rel_err(d["f32/y"], d["f64/y"]) <= 2e-6
    zero = np.abs(d["x"]).reshape(d["x"].shape[0], d["x"].shape[1], -1).max(-1) == 0
    for sel in (zero, ~zero):
        if sel.any():
            assert rel_err(d["f32/dx"][sel], d["f64/dx"][sel]) <= 2e-5
    for p in PARAMS:
        # under batch statistics d b1 is zero up to rounding: it is held to the scale of d W1 (as in tests/test_gpu_hfr.py)
        scale = np.abs(d["f64/dW1"]).max() if p == "b1" else 0.0
        assert rel_err(d["f32/d" + p], d["f64/d" + p], scale) <= 2e-5, p
    for s in ("running_mean", "running_var"):
        assert rel_err(d["f32/" + s], d["f64/" + s]) <= 2e-6, s


def test_fixture_covers_the_listed_cases():
    names = cases()
    metas = {n: case(n)["meta"] for n in names}
    widths = {int(m[0]) for m in metas.values()}
    assert {10, 64, 256} <= widths
    assert any(m[0] == 64 and m[4] == 1 for m in metas.values()) and any(m[0] == 64 and m[4] == 0 for m in metas.values())
    assert any(m[5] < 0 for m in metas.values())                             # momentum=None
    assert any((np.abs(case(n)["x"]).reshape(int(metas[n][1]), int(metas[n][0]), -1).max(-1) == 0).any() for n in names)
    # the clamp is active: some channel's weight is the clamp value, so y / u is 1e-5 there
    clamped = False
    for n in names:
        d = case(n)
        x = d["x"].astype(np.float64)
        nrm = np.sqrt((x.reshape(x.shape[0], x.shape[1], -1) ** 2).sum(-1))
        ratio = np.abs(d["f64/y"].reshape(x.shape[0], x.shape[1], -1)).max(-1) / np.maximum(
            np.abs(x.reshape(x.shape[0], x.shape[1], -1)).max(-1) / np.maximum(nrm, 1e-12), 1e-30)
        clamped |= bool((np.abs(ratio - 1e-5) < 1e-9).any())
    assert clamped


def _declared():
    text = open(os.path.join(ROOT, "include", "halo_hip.h")).read()
    return set(re.findall(r"\b(halo_hfr_\w+)\s*\(", text))


def test_header_signatures_and_library_agree():
    from halo_amd import _build, _lib
    assert _declared() == set(SYMBOLS)
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(h, s), s
    assert _lib.ABI_VERSION >= 10 and _lib.lib().halo_version() == _lib.ABI_VERSION


def test_workspace_query_is_host_code():
    """answered here, where no device exists"""
    from halo_amd import _lib
    q = _lib.lib().halo_hfr_workspace_bytes
    n = q(2, 64, 160 * 320)
    assert n >= 2 * 200 * (64 * 64 + 64) * 4                     # the per-block g_W1 / g_b1 partials of 256-pixel tiles
    assert q(2, 10, 160 * 320) >= 2 * 10 * 160 * 320 * 4           # the generic arm stages g_h (B, C, P)
    assert q(0, 64, 100) == 0 and q(2, 0, 100) == 0 and q(2, 64, 0) == 0 and q(2, 257, 100) == 0


def test_argument_checks_refuse_before_launching():
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.cast(buf, ctypes.c_void_p)
    n = L.halo_hfr_workspace_bytes(1, 64, 16)
    assert L.halo_hfr_fwd_stats(a, 1, 64, 16, a, a, None, a, n, None) != 0                       # no stats
    assert L.halo_hfr_fwd_stats(a, 1, 300, 16, a, a, a, a, n, None) == _lib.E_UNSUPPORTED       # C > 256
    assert L.halo_hfr_fwd_stats(a, 1, 64, 16, a, a, a, a, n - 1, None) != 0                     # short workspace
    assert L.halo_hfr_fwd_apply(a, 1, 64, 16, a, a, None, None, None, 0.1, 1e-5, a, a, a, a, a, a, n, None) != 0   # no statistics
    assert L.halo_hfr_bwd_reduce(a, 0, 64, 16, a, a, a, a, a, a, a, a, n, None) != 0             # empty shape
    assert L.halo_hfr_bwd_apply(a, 1, 64, 16, a, a, a, a, None, a, a, a, a, n, None) != 0        # no gradient sums
    assert "halo_hfr" in L.halo_last_error().decode()


def _mlp(C=64, norm=nn.BatchNorm1d):
    return nn.Sequential(nn.Linear(C, C), norm(C), nn.ReLU(), nn.Linear(C, C))


def test_envelope_and_fallback_decisions():
    from halo_amd.hfr import fallback_reason, weighted_normalize, torch_statement
    x = torch.randn(2, 64, 3, 5)
    mlp = _mlp()
    assert "device" in fallback_reason(x, mlp)                           # CPU tensors: the torch statement
    assert "float32" in fallback_reason(x.double(), mlp.double())
    assert "C = 300" in fallback_reason(torch.randn(1, 300, 2, 2), _mlp(300))
    assert "Sequential" in fallback_reason(x, nn.Sequential(nn.Linear(64, 64), nn.ReLU()))
    assert "Sequential" in fallback_reason(x, nn.Sequential(nn.Linear(64, 64), nn.BatchNorm1d(64), nn.GELU(), nn.Linear(64, 64)))
    assert "Sequential" in fallback_reason(x, nn.Sequential(nn.Linear(64, 64, bias=False), nn.BatchNorm1d(64), nn.ReLU(), nn.Linear(64, 64)))
    assert "channels" in fallback_reason(torch.randn(2, 32, 3, 5), mlp)
    assert fallback_reason(x, _mlp(norm=nn.SyncBatchNorm)) is not None  # served structure; here only the device is missing
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert fallback_reason(x, mlp) is not None
    torch.manual_seed(0)
    a, b = _mlp().train(), _mlp().train()
    b.load_state_dict(a.state_dict())
    assert torch.equal(weighted_normalize(x, a), torch_statement(x, b))   # the fallback IS the torch statement
    assert torch.equal(a[1].running_mean, b[1].running_mean) and int(a[1].num_batches_tracked) == 1
    one = torch.randn(1, 64, 1, 1)
    with pytest.raises(ValueError) as got:
        weighted_normalize(one, a)
    with pytest.raises(ValueError) as want:
        torch_statement(one, b)
    assert str(got.value) == str(want.value)


def test_merge_rank_stats_is_chan_in_rank_order():
    from halo_amd.hfr import merge_rank_stats
    rng = np.random.default_rng(4)
    parts = [rng.standard_normal((n, 3)) * 2 + 1 for n in (5, 7, 11)]
    rows = [torch.tensor(np.stack([np.full(3, len(p)), p.mean(0), ((p - p.mean(0)) ** 2).sum(0)], 1)) for p in parts]
    got = merge_rank_stats(rows).numpy()
    allp = np.concatenate(parts)
    assert np.allclose(got[:, 0], len(allp)) and np.allclose(got[:, 1], allp.mean(0), rtol=1e-13)
    assert np.allclose(got[:, 2], ((allp - allp.mean(0)) ** 2).sum(0), rtol=1e-12)
    assert torch.equal(merge_rank_stats(rows), merge_rank_stats([r.clone() for r in rows]))


class DepthwiseSeparableASPP_Hyper(nn.Module):
    """a stand-in with the reference's class and attribute names"""

    def forward(self, x, size=None):
        return "reference forward"


def test_hook_binds_an_opt_in_forward_and_keeps_the_previous_one():
    import halo_amd
    from halo_amd.core.models import classifier
    from halo_amd.hooks import use_fused_feature_reweighting, fused_v3plus_hyper_forward
    v3 = classifier.v3plus_hyper_forward
    Head = type("DepthwiseSeparableASPP_Hyper", (DepthwiseSeparableASPP_Hyper,), {})
    assert use_fused_feature_reweighting(Head) is Head
    assert Head.forward is fused_v3plus_hyper_forward
    assert Head._unfused_forward is DepthwiseSeparableASPP_Hyper.__dict__["forward"]
    assert use_fused_feature_reweighting(Head)._unfused_forward is DepthwiseSeparableASPP_Hyper.__dict__["forward"]   # idempotent
    assert classifier.v3plus_hyper_forward is v3 and DepthwiseSeparableASPP_Hyper.forward is not fused_v3plus_hyper_forward
    assert "fused_v3plus_hyper_forward" not in open(os.path.join(os.path.dirname(halo_amd.__file__), "__init__.py")).read()
