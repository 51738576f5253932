"""The validation metric on the device (halo_eval.hip through halo_amd.metrics / halo_amd.hooks) against the reference's own
arrays (tests/golden/eval.npz, tests/golden/make_eval_fixtures.py): counts exactly, arg-max maps bit for bit.  Sizes that are no
multiple of a block's 1024 pixels, other class counts, ignore_index values and strides are held to the contract chain of
tests/eval_inputs.py, equally exactly."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_inputs as ei  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = os.path.join(GOLDEN, "eval.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def small_cases():
    z = np.load(FIX)
    return sorted({k.split("/")[0] for k in z.files if not k.startswith("full_")})


def case(name):
    z = np.load(FIX)
    K, flip = (int(v) for v in z[name + "/meta"])
    return K, bool(flip), z[name + "/logits"], z[name + "/label"], z[name + "/pred"], z[name + "/ref"]


@pytest.mark.parametrize("name", small_cases())
def test_fused_counts_and_pred_equal_the_reference(dev, name):
    from halo_amd.metrics import flip_tta_confusion
    K, flip, lg, label, pred, ref = case(name)
    B, H, W = label.shape
    pred_out = torch.full((B, H, W), -7, dtype=torch.int64, device=dev)
    got = flip_tta_confusion(torch.from_numpy(lg).to(dev), torch.from_numpy(label).to(dev), K, 255, flip=flip, pred_out=pred_out)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and got.shape == (B, 3, K) and got.device == dev
    assert np.array_equal(pred_out.cpu().numpy(), pred)
    assert np.array_equal(got.cpu().numpy(), ref.astype(np.int64))


@pytest.mark.parametrize("name", small_cases())
def test_batch_equals_sum_of_single_image_calls_and_accumulates(dev, name):
    from halo_amd.metrics import ConfusionAccumulator, flip_tta_confusion
    K, flip, lg, label, _, ref = case(name)
    views = 2 if flip else 1
    lg_d, lab_d = torch.from_numpy(lg).to(dev), torch.from_numpy(label).to(dev)
    out = torch.zeros((1, 3, K), dtype=torch.int64, device=dev)
    for i in range(label.shape[0]):
        flip_tta_confusion(lg_d[views * i: views * (i + 1)], lab_d[i], K, flip=flip, out=out)
    acc = ConfusionAccumulator(K, dev).add_logits(lg_d, lab_d, flip=flip).add_logits(lg_d[:views], lab_d[0], flip=flip)
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), ref.sum(0).astype(np.int64))
    assert np.array_equal(acc.counts().cpu().numpy(), (ref.sum(0) + ref[0]).astype(np.int64))


@pytest.mark.parametrize("name", small_cases())
@pytest.mark.parametrize("pdt", [torch.int64, torch.int32, torch.uint8])
def test_counts_from_pred_equal_the_reference(dev, name, pdt):
    from halo_amd.metrics import confusion_from_pred
    K, _, _, label, pred, ref = case(name)
    got = confusion_from_pred(torch.from_numpy(pred).to(dev, pdt), torch.from_numpy(label).to(dev), K)
    assert np.array_equal(got.cpu().numpy(), ref.astype(np.int64))


@pytest.mark.parametrize("name", small_cases())
def test_intersection_and_union_gpu_is_the_reference_drop_in(dev, name):
    from halo_amd.metrics import intersection_and_union_gpu
    K, _, _, label, pred, ref = case(name)
    for i in range(label.shape[0]):
        output = torch.from_numpy(pred[i:i + 1]).to(dev)
        before = output.clone()
        got = intersection_and_union_gpu(output, torch.from_numpy(label[i:i + 1]).to(dev), K, 255)
        assert len(got) == 3
        for g, want in zip(got, ref[i]):
            assert g.dtype == torch.float32 and g.device == output.device and g.shape == (K,)
            assert np.array_equal(g.cpu().numpy(), want)
        assert torch.equal(output, before)                          # the one deviation: no in-place ignore write


@pytest.mark.parametrize("name", sorted(ei.FULLSIZE))
def test_fullsize_equals_stored_counts_digest_and_live_cpu_chain(dev, name):
    from halo_amd.metrics import flip_tta_confusion
    z = np.load(FIX)
    lg, label = ei.fullsize(name)
    H, W = label.shape
    pred_out = torch.empty((1, H, W), dtype=torch.int64, device=dev)
    got = flip_tta_confusion(torch.from_numpy(lg).to(dev), torch.from_numpy(label).to(dev), 19, pred_out=pred_out)
    pred = pred_out[0].cpu().numpy()
    assert ei.digest(pred) == str(z["full_" + name + "/pred_sha256"])
    assert np.array_equal(got[0].cpu().numpy(), z["full_" + name + "/ref"].astype(np.int64))
    live = ei.torch_chain_pred(torch.from_numpy(lg), (H, W), True)[0].numpy()
    assert np.array_equal(pred, live)
    assert np.array_equal(got[0].cpu().numpy(), ei.counts_from_pred(live, label, 19))


def test_unsupported_configurations_raise(dev):
    from halo_amd import _lib
    from halo_amd.metrics import confusion_from_pred, flip_tta_confusion
    lab = torch.zeros((1, 8, 16), dtype=torch.int16, device=dev)
    with pytest.raises(_lib.HaloUnsupported):
        confusion_from_pred(lab.to(torch.int64), lab, 19)
    with pytest.raises(_lib.HaloUnsupported):
        flip_tta_confusion(torch.zeros((2, 1025, 2, 4), device=dev), lab.to(torch.int64), 1025)
    with pytest.raises(TypeError):
        flip_tta_confusion(torch.zeros((2, 19, 2, 4), dtype=torch.float64, device=dev), lab.to(torch.int64), 19)


# ---------------------------------------------------------------- off the 1024 pixels of a block: tail lanes, any K, odd strides
# The reference here is eval_inputs.contract_pred (oracle/'s resize and softmax; tests/test_eval_metrics.py ties it to eval.npz):
# torch's CPU softmax has scalar tails at these sizes.  Every comparison is exact.
CANARY_PRED, CANARY_COUNT = -7, 2 ** 40 + 12345


def windows(n_pred, n_counts, dev, lead=5):
    """views of n elements inside larger canary-filled buffers, `lead` elements in (8-byte alignment only): (buffer, view) twice"""
    pb = torch.full((n_pred + 2 * lead,), CANARY_PRED, dtype=torch.int64, device=dev)
    cb = torch.full((n_counts + 2 * lead,), CANARY_COUNT, dtype=torch.int64, device=dev)
    return pb, pb[lead:lead + n_pred], cb, cb[lead:lead + n_counts]


def untouched(buf, n, canary, lead=5):
    b = buf.cpu().numpy()
    return bool((b[:lead] == canary).all() and (b[lead + n:] == canary).all())


def ragged_on(dev, name):
    K, views, lg, label, pred = ei.ragged_case(name)
    return K, views, torch.from_numpy(lg.copy()).to(dev), torch.from_numpy(label.copy()).to(dev), label, pred


def want_counts(pred, label, K, ignore_index=255):
    return np.stack([ei.counts_from_pred(pred[i], label[i], K, ignore_index) for i in range(label.shape[0])])


@pytest.mark.parametrize("name", sorted(ei.RAGGED))
def test_ragged_sizes_equal_the_contract_chain(dev, name):
    """Tail lanes count nothing and store nothing; the counts are added into values above 2^32."""
    from halo_amd.metrics import flip_tta_confusion
    K, views, lg_d, lab_d, label, pred = ragged_on(dev, name)
    B, H, W = label.shape
    pbuf, pwin, cbuf, cwin = windows(B * H * W, B * 3 * K, dev)
    got = flip_tta_confusion(lg_d, lab_d, K, 255, flip=views == 2, out=cwin.view(B, 3, K), pred_out=pwin.view(B, H, W))
    torch.cuda.synchronize()
    assert got.data_ptr() == cwin.data_ptr()
    assert np.array_equal(pwin.view(B, H, W).cpu().numpy(), pred)
    assert np.array_equal(cwin.view(B, 3, K).cpu().numpy() - CANARY_COUNT, want_counts(pred, label, K))
    assert untouched(pbuf, B * H * W, CANARY_PRED) and untouched(cbuf, B * 3 * K, CANARY_COUNT)


@pytest.mark.parametrize("name", sorted(n for n in ei.RAGGED if ei.RAGGED[n][5] > 1))
def test_ragged_batch_equals_single_image_calls(dev, name):
    """blockIdx.y's offsets into logits, labels, the prediction map and the slab, off every alignment"""
    from halo_amd.metrics import flip_tta_confusion
    K, views, lg_d, lab_d, label, pred = ragged_on(dev, name)
    B, H, W = label.shape
    batched = flip_tta_confusion(lg_d, lab_d, K, flip=views == 2)
    out = torch.zeros((1, 3, K), dtype=torch.int64, device=dev)
    singles = torch.full((B, H, W), CANARY_PRED, dtype=torch.int64, device=dev)
    for i in range(B):
        flip_tta_confusion(lg_d[views * i: views * (i + 1)], lab_d[i], K, flip=views == 2, out=out, pred_out=singles[i])
    torch.cuda.synchronize()
    assert np.array_equal(batched.sum(0).cpu().numpy(), out[0].cpu().numpy())
    assert np.array_equal(out[0].cpu().numpy(), want_counts(pred, label, K).sum(0))
    assert np.array_equal(singles.cpu().numpy(), pred)


def test_ignore_index_variants(dev):
    """ignore_index is taken literally, inside [0, K) (0, 7), negative (-1: the signed labels' -1s) or
    beyond every label (300: nothing is ignored)."""
    from halo_amd.metrics import confusion_from_pred, flip_tta_confusion
    K, views, lg_d, lab_d, label, pred = ragged_on(dev, "k19_37x53")
    lab_d, label = lab_d.to(torch.int64), label.astype(np.int64)
    pred_d = torch.from_numpy(pred.copy()).to(dev)
    seen = set()
    for ignore_index in (255, 0, 7, -1, 300):
        want = want_counts(pred, label, K, ignore_index)
        fused = flip_tta_confusion(lg_d, lab_d, K, ignore_index, flip=True)
        counted = confusion_from_pred(pred_d, lab_d, K, ignore_index)
        assert np.array_equal(fused.cpu().numpy(), want), ignore_index
        assert np.array_equal(counted.cpu().numpy(), want), ignore_index
        seen.add(want.tobytes())
    assert len(seen) == 5                                               # five different answers: none of them is 255's by accident


def pred_like(rng, label, K, dtype, ignore_index=255):
    """a prediction map for `label` (int64 values): agreeing at half of the pixels, else random classes, values outside
    [0, K) (negative ones for signed dtypes) and ignore_index at pixels whose label is not ignored"""
    p = rng.integers(0, K, label.shape)
    agree = (rng.random(label.shape) < 0.5) & (label >= 0) & (label < K)
    p[agree] = label[agree]
    r = rng.random(label.shape)
    p[r < 0.05] = rng.integers(K, K + 40, int((r < 0.05).sum()))
    p[(r >= 0.05) & (r < 0.10) & (label != ignore_index)] = ignore_index
    p[(r >= 0.10) & (r < 0.15)] = -3
    p[:, 0, :3] = (-3, K + 3, ignore_index)                              # over labels of class 0
    return p.astype(dtype)                                              # uint8 wraps: whatever it holds is the map that is counted


@pytest.mark.parametrize("K", [19, 86, 1024])
def test_from_pred_ragged_sizes_dtypes_and_key_patterns(dev, K):
    from halo_amd.metrics import confusion_from_pred
    rng = np.random.default_rng(300 + K)
    dts = [(np.int64, torch.int64), (np.int32, torch.int32), (np.uint8, torch.uint8)]
    for H, W in ((5, 7), (33, 31), (25, 41), (37, 53)):                 # 35, 1023, 1025, 1961 pixels
        for ldt, _ in dts:
            lab = rng.integers(0, K, (2, H, W))
            r = rng.random(lab.shape)
            lab[r < 0.1] = 255
            lab[(r >= 0.1) & (r < 0.14)] = K + 7
            lab[(r >= 0.14) & (r < 0.17)] = -1
            lab[:, 0, :6] = (0, 0, 0, 255, -1, K + 7)                   # the 35-pixel image holds one of each as well
            label = lab.astype(ldt)
            for pdt, _ in dts:
                pred = pred_like(rng, label.astype(np.int64), K, pdt)
                if pdt != np.uint8:
                    assert (pred < 0).any() and (pred >= K).any()
                assert ((pred == 255) & (label.astype(np.int64) != 255)).any()
                got = confusion_from_pred(torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev), K)
                assert np.array_equal(got.cpu().numpy(), want_counts(pred, label, K)), (H, W, ldt, pdt)


@pytest.mark.parametrize("pattern", ["64_pairs_per_wave", "one_pair"])
def test_from_pred_wave_key_patterns(dev, pattern):
    """The ballot loop's extremes at K = 86 on 1961 pixels: 64 distinct (prediction, label) pairs in every wave (64 trips,
    every leader lane in turn), and one pair for all pixels (one trip; class 85: the last word of the histogram)."""
    from halo_amd.metrics import confusion_from_pred
    K, B, H, W = 86, 2, 37, 53
    idx = np.arange(H * W)
    if pattern == "64_pairs_per_wave":
        label = np.stack([idx % 64, (idx + 5) % 64]).reshape(B, H, W)   # blocks start at multiples of 64: a wave sees each label once
        pred = np.stack([(idx // 64) % K, (idx % 64 + idx // 64) % K]).reshape(B, H, W)
    else:
        label = np.full((B, H, W), K - 1)
        pred = np.full((B, H, W), K - 1)
    got = confusion_from_pred(torch.from_numpy(pred).to(dev, torch.int32), torch.from_numpy(label).to(dev, torch.uint8), K)
    want = want_counts(pred, label, K)
    assert want[:, 0].sum() > 0
    assert np.array_equal(got.cpu().numpy(), want)


def test_finalize_with_more_than_256_blocks_and_two_images(dev):
    """513 x 512 pixels are 257 blocks: k_confusion_finalize's strided loop takes a second trip, on top of image 1's slab offset."""
    from halo_amd.metrics import confusion_from_pred
    K, B, H, W = 19, 2, 513, 512
    assert -(-H * W // 1024) == 257
    rng = np.random.default_rng(41)
    label = rng.integers(0, K, (B, H, W)).astype(np.uint8)
    label[rng.random((B, H, W)) < 0.1] = 255
    pred = rng.integers(0, K, (B, H, W)).astype(np.uint8)
    pred[1, : H // 2] = 4                                               # the two images differ, and so do their halves
    label[0, -1] = 11                                                   # the 257th block's only row: seen by the second trip alone
    pred[0, -1] = 11
    got = confusion_from_pred(torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev), K)
    want = want_counts(pred, label, K)
    assert not np.array_equal(want[0], want[1])
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("K", [19, 7])
def test_padded_batch_stride_through_the_entry_point(dev, K):
    """halo_eval_confusion accepts logit_bstride > K h w (a (B views, K + 2, h, w) buffer whose first K planes are the
    logits).  The two spare planes hold values that would win every arg-max."""
    from halo_amd import _lib
    from halo_amd.metrics import flip_tta_confusion
    _, views, lg_d, lab_d, label, pred = ragged_on(dev, "k19_37x53" if K == 19 else "k7_37x53")
    B, H, W = label.shape
    h, w = lg_d.shape[2:]
    padded = torch.full((B * views, K + 2, h, w), 1.0e4, dtype=torch.float32, device=dev)
    padded[:, :K] = lg_d
    L = _lib.lib()
    nws = L.halo_eval_workspace_bytes(B, K, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    counts = torch.zeros((B, 3, K), dtype=torch.int64, device=dev)
    pred_out = torch.full((B, H, W), CANARY_PRED, dtype=torch.int64, device=dev)
    _lib.check(L.halo_eval_confusion(_lib.ptr(padded), (K + 2) * h * w, views, K, h, w, _lib.ptr(lab_d), _lib.int_code(lab_d), H, W, B,
                                     255, _lib.ptr(counts), _lib.ptr(pred_out), _lib.ptr(ws), nws, _lib.stream_ptr(dev)),
               "halo_eval_confusion")
    plain_pred = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    plain = flip_tta_confusion(padded[:, :K].contiguous(), lab_d, K, flip=views == 2, pred_out=plain_pred)
    torch.cuda.synchronize()
    assert torch.equal(pred_out, plain_pred) and torch.equal(counts, plain)
    assert np.array_equal(pred_out.cpu().numpy(), pred)


class TinyBackbone(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, C, kernel_size=8, stride=8)

    def forward(self, x):
        return {"out": self.conv(x)}


class StandIn(object):
    """The attributes BaseLearner's validation methods use, with a tiny real head.  Its own (unhooked) methods are the
    reference's chain written out on the CPU (tests/eval_inputs.py) and the reference's epoch-end formula."""

    def __init__(self, dev, K=19, C=8):
        from halo_amd.core.models.classifier import ASPP_Classifier_V2_Hyper
        torch.manual_seed(0)
        self.cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=K), INPUT=types.SimpleNamespace(IGNORE_LABEL=255))
        self.device = dev
        self.feature_extractor = TinyBackbone(C).to(dev).eval()
        self.classifier = ASPP_Classifier_V2_Hyper(C, [1, 2], [1, 2], K, C).to(dev).eval()
        for m in self.classifier.conv2d_list:
            m.weight.data.normal_(0, 0.3)
        self.intersections = self.unions = self.targets = np.array([])
        self.logged = {}

    def validation_step(self, batch, batch_idx):
        x, y = batch["img"], batch["label"]
        with torch.no_grad():
            output, _ = self.classifier(self.feature_extractor(torch.cat([x, torch.flip(x, [3])], 0)))
        pred = ei.torch_chain_pred(output.cpu(), y.shape[-2:], True)[0].numpy()
        c = ei.counts_from_pred(pred, y[0].cpu().numpy(), self.cfg.MODEL.NUM_CLASSES).astype(np.float32)[:, None]
        for attr, row in zip(("intersections", "unions", "targets"), c):
            have = getattr(self, attr)
            setattr(self, attr, row if have.size == 0 else np.concatenate((have, row), axis=0))

    def on_validation_epoch_end(self):
        inter, union, target = (getattr(self, n).sum(axis=0) for n in ("intersections", "unions", "targets"))
        iou_class, accuracy_class = inter / (union + 1e-10), inter / (target + 1e-10)
        for k, v in (("mIoU", iou_class.mean() * 100), ("mAcc", accuracy_class.mean() * 100),
                     ("aAcc", inter.sum() / (target.sum() + 1e-10) * 100)):
            self.log(k, v, on_step=False, on_epoch=True, sync_dist=True, prog_bar=True)
        self.intersections = self.unions = self.targets = np.array([])

    def all_gather(self, t):
        return t

    def log(self, name, value, **kw):
        self.logged[name] = (float(value), kw)


def test_hooked_learner_logs_the_unhooked_metrics(dev):
    from halo_amd.hooks import use_device_metrics

    class Hooked(StandIn):
        pass

    use_device_metrics(Hooked)
    rng = np.random.default_rng(5)
    H, W = 128, 256
    batches = []
    for i in range(3):
        x = torch.from_numpy(rng.standard_normal((1, 3, H, W), dtype=np.float32)).to(dev)
        y = rng.integers(0, 19, (1, H, W))
        y[:, rng.random((H, W)) < 0.1] = 255
        batches.append({"img": x, "label": torch.from_numpy(y).to(dev), "name": ["img%d" % i]})
    plain, hooked = StandIn(dev), Hooked(dev)
    for i, b in enumerate(batches):
        plain.validation_step(b, i)
        hooked.validation_step(b, i)
    assert hooked.intersections.size == 0                         # every step took the device path
    plain.on_validation_epoch_end()
    hooked.on_validation_epoch_end()
    for k in ("mIoU", "mAcc", "aAcc"):
        want, kw = plain.logged[k]
        got, kw2 = hooked.logged[k]
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want)) and kw == kw2
    assert 0.0 < plain.logged["aAcc"][0] < 100.0
