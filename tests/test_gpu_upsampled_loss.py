"""The training criterion from low-resolution logits on the device (halo_train_loss.hip through halo_amd.training / halo_amd.hooks)
against the reference's own loss modules (tests/golden/upsampled_loss.npz, tests/golden/make_upsampled_loss_fixtures.py) and a
live torch CPU chain: losses within 2e-6 relative, logit gradients within 2e-5 * max|g|, both counts exact."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIX = os.path.join(GOLDEN, "upsampled_loss.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def fixture_cases():
    z = np.load(FIX)
    return sorted({k.split("/")[0] for k in z.files if k.endswith("/values")})


def case(name):
    z = np.load(FIX)
    return {k.split("/")[1]: z[k] for k in z.files if k.startswith(name + "/")}


def close(got, want, rel=2e-6):
    got, want = float(got.detach() if torch.is_tensor(got) else got), float(want)
    if np.isnan(want):
        return np.isnan(got)
    return abs(got - want) <= rel * max(abs(want), 1e-30)


def grad_close(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return np.abs(got - want).max() <= 2e-5 * np.abs(want).max() + 1e-12


def torch_chain(lg, label, threshold=0.05):
    """the reference's chain on the CPU: F.interpolate (align_corners=True) -> CrossEntropyLoss(ignore_index=255) and
    NegativeLearningLoss of torch.softmax; returns values, counts and both logit gradients"""
    x = lg.detach().cpu().clone().requires_grad_(True)
    y = label.cpu().to(torch.int64)
    up = F.interpolate(x, size=y.shape[-2:], mode="bilinear", align_corners=True)
    ce = nn.CrossEntropyLoss(ignore_index=255)(up, y)
    p = torch.softmax(up, dim=1)
    mask = (p < threshold).detach()
    nl = torch.sum(-1 * mask * torch.log(1 - p + 1e-6)) / torch.sum(mask)
    (g_ce,) = torch.autograd.grad(ce, x, retain_graph=True)
    (g_nl,) = torch.autograd.grad(nl, x)
    return ce.item(), nl.item(), (int((y != 255).sum()), int(mask.sum())), g_ce.numpy(), g_nl.numpy()


def fused(lg, label, dev, **kw):
    from halo_amd.training import upsampled_losses
    x = torch.from_numpy(lg).to(dev).requires_grad_(True) if isinstance(lg, np.ndarray) else lg.to(dev).detach().requires_grad_(True)
    y = torch.from_numpy(label).to(dev) if isinstance(label, np.ndarray) else label.to(dev)
    return x, y, upsampled_losses(x, y, **kw)


def sums_of(x, y, dev, terms=3):
    """the kernel's raw sums vector (ce_sum, ce_count, nl_sum, nl_count, bad)"""
    from halo_amd import _lib
    L = _lib.lib()
    B, K, h, w = x.shape
    H, W = y.shape[-2:]
    n = L.halo_upsampled_loss_workspace_bytes(B, K, H, W)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    sums = torch.empty(5, dtype=torch.float64, device=dev)
    _lib.check(L.halo_upsampled_loss_fwd(_lib.ptr(x), K * h * w, B, K, h, w, _lib.ptr(y), _lib.int_code(y), H, W, 255, 0.05, terms,
                                         _lib.ptr(sums), _lib.ptr(ws), n, _lib.stream_ptr(dev)), "fwd")
    return sums.cpu().numpy()


@pytest.mark.parametrize("name", fixture_cases())
def test_golden_values_gradients_and_exact_counts(dev, name):
    c = case(name)
    x, y, r = fused(c["logits"], c["label"], dev)
    assert r.ce.dtype == torch.float32 and r.ce.dim() == 0 and r.nl.dim() == 0 and r.n_labelled.dtype == torch.int64
    assert close(r.ce, c["values"][0]) and close(r.nl, c["values"][1]), (float(r.ce), float(r.nl), c["values"])
    assert int(r.n_labelled) == int(c["counts"][0])
    s = sums_of(x.detach(), y, dev)
    assert int(s[1]) == int(c["counts"][0]) and int(s[3]) == int(c["counts"][1]) and s[4] == 0
    (g_ce,) = torch.autograd.grad(r.ce, x, retain_graph=True)
    (g_nl,) = torch.autograd.grad(r.nl, x)
    if int(c["counts"][0]) == 0:
        assert np.isnan(float(r.ce.detach())) and float(g_ce.abs().max()) == 0.0
    else:
        assert grad_close(g_ce, c["g_ce"])
    assert grad_close(g_nl, c["g_nl"])


TRAINING_SHAPES = [  # name, B, K, (h, w), (H, W), labelled fraction
    ("target", 2, 19, (160, 320), (640, 1280), 0.05),
    ("source", 2, 19, (180, 320), (720, 1280), 1.0),
    ("k16", 2, 16, (160, 320), (640, 1280), 0.9),
]


@pytest.mark.parametrize("shape", TRAINING_SHAPES, ids=[s[0] for s in TRAINING_SHAPES])
def test_training_shapes_match_a_live_cpu_chain(dev, shape):
    name, B, K, (h, w), (H, W), frac = shape
    g = torch.Generator().manual_seed(11)
    lg = torch.randn((B, K, h, w), generator=g) * 2.5
    label = torch.randint(0, K, (B, H, W), generator=g)
    label[torch.rand((B, H, W), generator=g) >= frac] = 255
    ce, nl, counts, g_ce, g_nl = torch_chain(lg, label)
    x, y, r = fused(lg, label, dev)
    assert close(r.ce, ce) and close(r.nl, nl), (float(r.ce), ce, float(r.nl), nl)
    s = sums_of(x.detach(), y, dev)
    assert (int(s[1]), int(s[3])) == counts                      # the NL mask is torch's, pair for pair
    (gc,) = torch.autograd.grad(r.ce, x, retain_graph=True)
    assert grad_close(gc, g_ce)
    (gn,) = torch.autograd.grad(r.nl, x)
    assert grad_close(gn, g_nl)


def test_backward_is_bit_reproducible(dev):
    g = torch.Generator().manual_seed(3)
    lg = torch.randn((2, 19, 160, 320), generator=g) * 2.5
    label = torch.randint(0, 19, (2, 640, 1280), generator=g)
    label[torch.rand((2, 640, 1280), generator=g) >= 0.3] = 255
    x, y, r = fused(lg, label, dev)
    a = torch.autograd.grad(r.ce + 0.5 * r.nl, x, retain_graph=True)[0].clone()
    b = torch.autograd.grad(r.ce + 0.5 * r.nl, x)[0]
    assert torch.equal(a, b)
    r2 = fused(lg, label, dev)[2]
    assert torch.equal(r2.ce, r.ce) and torch.equal(r2.nl, r.nl)


@pytest.mark.parametrize("name", ["k19_i64_x4_active", "k16_i32_x4_dense", "k7_u8_frac_active"])
def test_mixed_upstream_gradients_match_autograd_of_the_weighted_sum(dev, name):
    c = case(name)
    for wc, wn in ((1.0, None), (None, 1.0), (0.3, 1.7), (-2.0, 0.25)):
        x, y, r = fused(c["logits"], c["label"], dev)
        loss = (r.ce * wc if wc is not None else 0) + (r.nl * wn if wn is not None else 0)
        (gx,) = torch.autograd.grad(loss, x)
        want = (wc or 0.0) * c["g_ce"] + (wn or 0.0) * c["g_nl"]
        assert grad_close(gx, want), (wc, wn)
    x, y, r = fused(c["logits"], c["label"], dev, negative=False)     # one term off: its output is None, the other unchanged
    assert r.nl is None and close(r.ce, c["values"][0])
    assert grad_close(torch.autograd.grad(r.ce, x)[0], c["g_ce"])
    x, y, r = fused(c["logits"], c["label"], dev, cross_entropy=False)
    assert r.ce is None and close(r.nl, c["values"][1]) and int(r.n_labelled) == int(c["counts"][0])
    assert grad_close(torch.autograd.grad(r.nl, x)[0], c["g_nl"])


def test_out_of_range_label_raises_index_error_and_the_stream_stays_usable(dev):
    c = case("k7_i64_bad_label")
    assert "out of bounds" in str(c["torch_error"])
    with pytest.raises(IndexError, match="out of bounds"):
        fused(c["logits"], c["label"], dev)
    x, y, r = fused(c["logits"], c["label"], dev, check_labels=False)        # counted, never used as an index
    assert np.isfinite(float(r.ce))
    assert sums_of(x.detach(), y, dev)[4] == 1
    good = case("k7_i64_x4_dense")
    _, _, r = fused(good["logits"], good["label"], dev)
    torch.cuda.synchronize()
    assert close(r.ce, good["values"][0]) and close(r.nl, good["values"][1])


def test_unsupported_inputs_raise(dev):
    from halo_amd import _lib
    from halo_amd.training import upsampled_losses
    lg = torch.zeros((1, 19, 4, 8), device=dev)
    lab = torch.zeros((1, 16, 32), dtype=torch.int64, device=dev)
    with pytest.raises(TypeError):
        upsampled_losses(lg.double(), lab)
    with pytest.raises(TypeError):
        upsampled_losses(lg, lab.to(torch.int16))
    with pytest.raises(ValueError):
        upsampled_losses(lg.cpu(), lab)
    with pytest.raises(ValueError):
        upsampled_losses(lg[0], lab)
    with pytest.raises(ValueError):
        upsampled_losses(lg, torch.zeros((2, 16, 32), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        upsampled_losses(lg, lab, size=(16, 30))
    with pytest.raises(ValueError):
        upsampled_losses(lg, torch.zeros((1, 3, 32), dtype=torch.int64, device=dev))     # downsampling
    with pytest.raises(_lib.HaloUnsupported):
        upsampled_losses(torch.zeros((1, 1025, 2, 2), device=dev), torch.zeros((1, 4, 4), dtype=torch.int64, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the hook on a stand-in learner with a tiny hyper head
class TinyBackbone(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv = nn.Conv2d(3, C, kernel_size=8, stride=8)

    def forward(self, x):
        return {"out": self.conv(x)}


class TorchNL(nn.Module):
    """NegativeLearningLoss's formula in plain torch (core/loss/negative_learning_loss.py:11-16)"""

    def __init__(self, threshold=0.05):
        super().__init__()
        self.threshold = threshold

    def forward(self, predict):
        mask = (predict < self.threshold).detach()
        return torch.sum(-1 * mask * torch.log(1 - predict + 1e-6)) / torch.sum(mask)


class NoStepOptimizer(object):
    """zero_grad only: the parameter gradients of one step are what the test compares"""

    def __init__(self, params):
        self.params = list(params)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        pass


class StandInBase(object):
    def __init__(self, dev, neg=1.0, cons=0.0, K=19, C=8):
        from halo_amd.core.loss import LocalConsistentLoss
        from halo_amd.core.models.classifier import ASPP_Classifier_V2_Hyper
        torch.manual_seed(0)
        self.cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=K),
                                         SOLVER=types.SimpleNamespace(NEGATIVE_LOSS=neg, CONSISTENT_LOSS=cons))
        self.hyper = True
        self.feature_extractor = TinyBackbone(C).to(dev)
        self.classifier = ASPP_Classifier_V2_Hyper(C, [1, 2], [1, 2], K, C).to(dev)
        for m in self.classifier.conv2d_list:
            m.weight.data.normal_(0, 0.3)
        self.criterion = nn.CrossEntropyLoss(ignore_index=255)
        self.negative_criterion = TorchNL()
        self.local_consistent_loss = LocalConsistentLoss(K, "l1")
        self._opt = NoStepOptimizer(list(self.feature_extractor.parameters()) + list(self.classifier.parameters()))
        self.logged = {}

    def forward(self, x):
        return self.classifier(self.feature_extractor(x), size=x.shape[-2:])

    def optimizers(self):
        return [self._opt]

    def lr_schedulers(self):
        return []

    def log_metrics(self, batch_idx):
        pass

    def manual_backward(self, loss):
        loss.backward()

    def log(self, name, value, **kw):
        self.logged[name] = (float(value), kw)

    def grads(self):
        return [p.grad.detach().cpu().numpy().copy() for p in self._opt.params]


class SourceFreeLearner(StandInBase):
    """the reference's SourceFreeLearner.training_step, stated on the stand-in (core/train_learners.py:328-368)"""

    def training_step(self, batch, batch_idx):
        for opt in self.optimizers():
            opt.zero_grad()
        tgt_input, tgt_mask = batch["img"], batch["mask"]
        tgt_out = self.forward(tgt_input)[0]
        predict = torch.softmax(tgt_out, dim=1)
        loss = torch.Tensor([0]).cuda()
        if torch.sum(tgt_mask != 255) != 0:
            loss_sup = self.criterion(tgt_out, tgt_mask)
            loss += loss_sup
            self.log("loss_sup", loss_sup.item(), on_step=True, on_epoch=False, sync_dist=True, prog_bar=True)
        if self.cfg.SOLVER.NEGATIVE_LOSS > 0:
            negative_loss = self.negative_criterion(predict) * self.cfg.SOLVER.NEGATIVE_LOSS
            loss += negative_loss
            self.log("negative_loss", negative_loss.item(), on_step=True, on_epoch=False, sync_dist=True, prog_bar=True)
        self.log("loss", loss.item(), on_step=True, on_epoch=False, sync_dist=True, prog_bar=True)
        self.log_metrics(batch_idx)
        self.manual_backward(loss)
        for opt in self.optimizers():
            opt.step()


class SourceTargetLearner(SourceFreeLearner):
    """the reference's SourceTargetLearner.training_step, stated on the stand-in (core/train_learners.py:404-463)"""

    def training_step(self, batch, batch_idx):
        for opt in self.optimizers():
            opt.zero_grad()
        src_input, src_label = batch[0]["img"], batch[0]["label"]
        src_out = self.forward(src_input)[0]
        tgt_input, tgt_mask = batch[1]["img"], batch[1]["mask"]
        tgt_out = self.forward(tgt_input)[0]
        predict = torch.softmax(tgt_out, dim=1)
        loss = torch.Tensor([0]).cuda()
        kw = dict(on_step=True, on_epoch=False, sync_dist=True, prog_bar=True)
        loss_sup = self.criterion(src_out, src_label)
        loss += loss_sup
        self.log("loss_sup", loss_sup.item(), **kw)
        if torch.sum(tgt_mask != 255) != 0:
            loss_sup_tgt = self.criterion(tgt_out, tgt_mask)
            loss += loss_sup_tgt
            self.log("loss_sup_tgt", loss_sup_tgt.item(), **kw)
        if self.cfg.SOLVER.CONSISTENT_LOSS > 0:
            consistency_loss = self.local_consistent_loss(src_out, src_label) * self.cfg.SOLVER.CONSISTENT_LOSS
            loss += consistency_loss
            self.log("consistency_loss", consistency_loss.item(), **kw)
        if self.cfg.SOLVER.NEGATIVE_LOSS > 0:
            negative_loss = self.negative_criterion(predict) * self.cfg.SOLVER.NEGATIVE_LOSS
            loss += negative_loss
            self.log("negative_loss", negative_loss.item(), **kw)
        self.log("loss", loss.item(), **kw)
        self.log_metrics(batch_idx)
        self.manual_backward(loss)
        for opt in self.optimizers():
            opt.step()


def _image_batch(dev, rng, B, H, W, K, frac, key):
    x = torch.from_numpy(rng.standard_normal((B, 3, H, W), dtype=np.float32)).to(dev)
    y = rng.integers(0, K, (B, H, W))
    y[rng.random((B, H, W)) >= frac] = 255
    return {"img": x, key: torch.from_numpy(y).to(dev)}


def _compare_steps(plain, hooked, batch):
    plain.training_step(batch, 0)
    hooked.training_step(batch, 0)
    assert sorted(plain.logged) == sorted(hooked.logged)
    for k, (want, kw) in plain.logged.items():
        got, kw2 = hooked.logged[k]
        assert kw == kw2 and close(got, want, 2e-6 if k != "consistency_loss" else 1e-5), (k, got, want)
    for gw, gg in zip(plain.grads(), hooked.grads()):
        assert np.abs(gg - gw).max() <= 2e-5 * np.abs(gw).max() + 1e-12


@pytest.mark.parametrize("frac", [0.05, 0.0], ids=["active", "unlabelled"])
def test_hooked_source_free_step_logs_and_grads_like_the_unhooked(dev, frac):
    from halo_amd.hooks import use_fused_training_losses

    class Hooked(SourceFreeLearner):
        pass

    use_fused_training_losses(Hooked)
    rng = np.random.default_rng(21)
    batch = _image_batch(dev, rng, 2, 64, 128, 19, frac, "mask")
    plain, hooked = SourceFreeLearner(dev), Hooked(dev)
    _compare_steps(plain, hooked, batch)
    assert ("loss_sup" in plain.logged) == (frac > 0) and "negative_loss" in plain.logged


@pytest.mark.parametrize("cons,frac", [(0.0, 0.05), (0.5, 0.05), (0.5, 0.0)], ids=["plain", "consistency", "consistency_unlabelled"])
def test_hooked_source_target_step_logs_and_grads_like_the_unhooked(dev, cons, frac):
    from halo_amd.hooks import use_fused_training_losses

    class Hooked(SourceTargetLearner):
        pass

    use_fused_training_losses(Hooked)
    rng = np.random.default_rng(22)
    batch = [_image_batch(dev, rng, 2, 72, 128, 19, 0.9, "label"), _image_batch(dev, rng, 2, 64, 128, 19, frac, "mask")]
    plain, hooked = SourceTargetLearner(dev, cons=cons), Hooked(dev, cons=cons)
    _compare_steps(plain, hooked, batch)
    assert ("consistency_loss" in plain.logged) == (cons > 0) and ("loss_sup_tgt" in plain.logged) == (frac > 0)
