"""The loss kernels at the launch geometries of the training shapes, scaled down to the smallest sizes that still reach them.

halo_loss.hip (LocalConsistentLoss 'l1' / 'kl', NegativeLearningLoss) against tests/loss_ref.py, a float64 CPU evaluation: masks and
counts exact, values within the project's 3e-6, gradients PER ELEMENT -- |gx - g64| <= 4 K_REF 2^-24 A for LocalConsistentLoss
(K_REF: what the float32 torch CPU chain itself shows, tests/test_loss_ref_host.py) and exactly 0.0 where A == 0; zero where
unmasked and within 6 * 2^-24 relative where masked for NegativeLearningLoss.  halo_train_loss.hip (upsampled_losses) against the
live float32 CPU chain of tests/test_gpu_upsampled_loss.py, to which that path is pinned bit for bit in its taps and softmax.

Largest ratios to the bounds observed on an MI355X: see NOTES.md (round 12)."""
import functools

import numpy as np
import pytest
import torch

import loss_ref as R
from test_gpu_upsampled_loss import close, fused, grad_close, sums_of, torch_chain

pytestmark = pytest.mark.gpu

LCL_IDS = ["x".join(str(v) for v in c) for c in R.LCL_CASES]
SMALL = (1, 19, 9, 258)                                               # the wrapper paths: two strips, two row groups


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def lcl_data(case):
    return R.lcl_case(*case)


@functools.lru_cache(maxsize=None)
def lcl_ref(case, kl):
    return R.local_consistent(*lcl_data(case), kl)


def lcl_raw_forward(x, label, kl, dev):
    """one direct halo_local_consistent_fwd call with the backward's outputs requested: (sums, mask bytes)"""
    from halo_amd import _lib
    L = _lib.lib()
    B, O, h, w = x.shape
    p, ca, cb = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    mask = torch.full((B, h, w), 7, dtype=torch.uint8, device=dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    nws = L.halo_loss_workspace_bytes(B * h * w)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _lib.check(L.halo_local_consistent_fwd(_lib.ptr(x), _lib.ptr(label), B, O, h, w, 1 if kl else 0, _lib.ptr(p), _lib.ptr(sums), _lib.ptr(ca),
                                           _lib.ptr(cb), _lib.ptr(mask), _lib.ptr(ws), nws, _lib.stream_ptr(dev)), "halo_local_consistent_fwd")
    return sums.cpu().numpy(), mask.cpu().numpy()


def lcl_run(x, label, lt):
    from halo_amd.core.loss import LocalConsistentLoss
    loss = LocalConsistentLoss(x.shape[1], lt)(x, label)
    (gx,) = torch.autograd.grad(loss, x)
    return loss.detach(), gx


@pytest.mark.parametrize("lt", ["l1", "kl"])
@pytest.mark.parametrize("case", R.LCL_CASES, ids=LCL_IDS)
def test_local_consistent_matches_float64_per_element(dev, case, lt):
    x, label = lcl_data(case)
    ref = lcl_ref(case, lt == "kl")
    xd, lab = x.to(dev).requires_grad_(True), label.to(dev)
    loss, gx = lcl_run(xd, lab, lt)
    assert loss.dtype == torch.float32 and gx.dtype == torch.float32
    sums, mask = lcl_raw_forward(xd.detach(), lab, lt == "kl", dev)
    assert np.array_equal(mask, ref.mask.astype(np.uint8))                      # every byte written, 0 or 1
    assert sums[1] == ref.count
    assert abs(loss.item() - ref.loss) < 3e-6 * max(1.0, abs(ref.loss)), (loss.item(), ref.loss)
    g = gx.cpu().numpy().astype(np.float64)
    pos = ref.A > 0
    err = np.abs(g - ref.gx)
    ratio = float((err[pos] / (4 * R.K_REF * R.U * ref.A[pos])).max())
    print("lcl", case, lt, "count %d  max |gx - g64| / (4 K_REF 2^-24 A) = %.4f  global %.3e of max|g|"
          % (ref.count, ratio, err.max() / np.abs(ref.gx).max()))
    assert ratio <= 1.0, ratio
    assert not g[~pos].any()                                                    # no masked pixel in the window: the zeros are written
    assert err.max() < 3e-5 * np.abs(ref.gx).max() + 1e-9
    side = torch.cuda.Stream(dev)                                               # the same bits from a second call on another stream
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        x2 = x.to(dev).requires_grad_(True)
        loss2, gx2 = lcl_run(x2, lab, lt)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert torch.equal(loss2, loss) and torch.equal(gx2, gx)


@pytest.mark.parametrize("lt", ["l1", "kl"])
def test_local_consistent_wrapper_paths(dev, lt):
    """a strided channel slice, float16 / float64 logits (the gradient returns in the input's dtype and is the float32 run's after
    the cast), int32 / uint8 labels: the bits of the plain float32 / int64 call"""
    x, label = lcl_data(SMALL)
    lab = label.to(dev)
    loss, gx = lcl_run(x.to(dev).requires_grad_(True), lab, lt)
    big = torch.zeros((1, 38, 9, 258), device=dev)
    big[:, ::2] = x.to(dev)
    big.requires_grad_(True)
    xs = big[:, ::2]
    assert not xs.is_contiguous()
    from halo_amd.core.loss import LocalConsistentLoss
    ls = LocalConsistentLoss(19, lt)(xs, lab)
    (gb,) = torch.autograd.grad(ls, big)
    assert torch.equal(ls.detach(), loss) and torch.equal(gb[:, ::2], gx) and not bool(gb[:, 1::2].any())
    for dt in (torch.float16, torch.float64):
        xt = (x.double() * (1 + 2.0 ** -30)).to(dt).to(dev)                   # (float64: bits below float32's that the wrapper rounds away)
        l32, g32 = lcl_run(xt.float().requires_grad_(True), lab, lt)
        lt_, gt = lcl_run(xt.clone().requires_grad_(True), lab, lt)
        assert gt.dtype == dt and lt_.dtype == torch.float32
        assert torch.equal(lt_, l32) and torch.equal(gt, g32.to(dt))
    for dt in (torch.int32, torch.uint8):
        l2, g2 = lcl_run(x.to(dev).requires_grad_(True), label.to(dt).to(dev), lt)
        assert torch.equal(l2, loss) and torch.equal(g2, gx)


# ---------------------------------------------------------------- NegativeLearningLoss
NL_BIG = 4 * 2048 * 256 + 4 * 256 * 3 + 3              # blocks 0..2 take a second trip of the float4 loop; a three-element scalar tail
THR = np.float32(0.05)
BELOW = np.nextafter(THR, np.float32(0))


@functools.lru_cache(maxsize=None)
def nl_data(n):
    if n <= 3:
        return torch.from_numpy(np.array([BELOW, THR, 0.0][:n] if n < 3 else [THR, BELOW, 0.0], np.float32))
    g = torch.Generator().manual_seed(n)
    p = torch.rand(n, generator=g) * 0.2
    plant = torch.tensor([float(THR), float(BELOW), 0.0])
    for at in (5, 4 * 2048 * 256 + 9, n - 3):          # first trip, second trip of block 0, the scalar tail
        p[at:at + 3] = plant
    return p


@functools.lru_cache(maxsize=None)
def nl_ref(n):
    return R.negative_learning(nl_data(n).numpy(), 0.05)


def nl_sums(p, dev):
    from halo_amd import _lib
    L = _lib.lib()
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    nws = L.halo_loss_workspace_bytes(p.numel())
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _lib.check(L.halo_negative_learning_fwd(_lib.ptr(p), p.numel(), 0.05, _lib.ptr(sums), _lib.ptr(ws), nws, _lib.stream_ptr(dev)),
               "halo_negative_learning_fwd")
    return sums.cpu().numpy()


@pytest.mark.parametrize("n,off", [(NL_BIG, 0), (NL_BIG, 1), (1, 0), (2, 0), (3, 0)], ids=["big", "big_offset_1", "n1", "n2", "n3"])
def test_negative_learning_matches_float64_per_element(dev, n, off):
    from halo_amd.core.loss import NegativeLearningLoss
    ref = nl_ref(n)
    assert ref.count > 0
    buf = torch.zeros(n + off + 8, device=dev)
    buf[off:off + n] = nl_data(n).to(dev)
    p = buf[off:off + n].detach().requires_grad_(True)                           # off = 1: a view 4 bytes past a 16-byte boundary
    assert p.data_ptr() % 16 == 4 * off
    loss = NegativeLearningLoss(0.05)(p)
    (gp,) = torch.autograd.grad(loss, p)
    assert nl_sums(p.detach(), dev)[1] == ref.count
    assert abs(loss.item() - ref.loss) < 3e-6, (loss.item(), ref.loss)
    g = gp.cpu().numpy().astype(np.float64)
    assert not g[~ref.mask].any()
    rel = np.abs(g - ref.gp)[ref.mask] / ref.gp[ref.mask]
    print("nl", n, off, "count %d  max relative gradient error %.3f * 2^-24" % (ref.count, rel.max() / R.U))
    assert rel.max() <= 6 * R.U


# ---------------------------------------------------------------- upsampled_losses
UPL_CASES = [  # name, B, K, (h, w), (H, W), label dtype
    ("ragged_second_tile", 2, 19, (5, 40), (20, 160), torch.int64),             # 8 live cells in the second backward tile
    ("fractional_one_live_cell", 2, 16, (3, 33), (7, 70), torch.int32),
    ("x8_partial_row_trips", 1, 19, (3, 34), (24, 272), torch.uint8),           # two and more trips of the y0 loop, the last partial
    ("scale_one", 1, 19, (4, 70), (4, 70), torch.int64),
    ("scale_zero_both", 1, 19, (1, 1), (6, 9), torch.int32),
    ("scale_zero_columns", 1, 19, (6, 1), (24, 1), torch.uint8),
    ("scale_zero_rows", 1, 19, (1, 37), (1, 148), torch.int64),
    ("generic_two_tiles_wide", 1, 7, (2, 45), (9, 100), torch.int32),
]


@pytest.mark.parametrize("shape", UPL_CASES, ids=[s[0] for s in UPL_CASES])
def test_upsampled_losses_ragged_tiles_and_scales_match_the_cpu_chain(dev, shape):
    name, B, K, (h, w), (H, W), dt = shape
    g = torch.Generator().manual_seed(17 + h * 1000 + w)
    lg = torch.randn((B, K, h, w), generator=g) * 2.5
    label = torch.randint(0, K, (B, H, W), generator=g)
    label[torch.rand((B, H, W), generator=g) >= 0.3] = 255
    label = label.to(dt)
    ce, nl, counts, g_ce, g_nl = torch_chain(lg, label)
    assert counts[0] > 0 and counts[1] > 0
    x, y, r = fused(lg, label, dev)
    assert y.dtype == dt
    assert close(r.ce, ce) and close(r.nl, nl), (float(r.ce), ce, float(r.nl), nl)
    s = sums_of(x.detach(), y, dev)
    assert (int(s[1]), int(s[3])) == counts and s[4] == 0
    (gc,) = torch.autograd.grad(r.ce, x, retain_graph=True)
    assert grad_close(gc, g_ce)
    (gn,) = torch.autograd.grad(r.nl, x)
    assert grad_close(gn, g_nl)
