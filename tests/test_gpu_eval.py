"""The validation metric on the device (halo_eval.hip through halo_amd.metrics / halo_amd.hooks) against the reference's own
arrays (tests/golden/eval.npz, tests/golden/make_eval_fixtures.py): counts exactly, arg-max maps bit for bit."""
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
