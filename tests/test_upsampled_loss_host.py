"""CPU checks of the fused training criterion (halo_train_loss.hip, halo_amd.training, halo_amd.hooks.use_fused_training_losses):
the ABI 10 entry points are exported, the workspace query, the argument checks that refuse before any launch, the fixture
against a live torch CPU chain, and the hook's choice of protocol.  The kernels themselves are held to the fixture in
tests/test_gpu_upsampled_loss.py."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "upsampled_loss.npz")
SYMBOLS = ("halo_upsampled_loss_workspace_bytes", "halo_upsampled_loss_fwd", "halo_upsampled_loss_bwd")


def test_abi_10_entry_points_are_exported():
    from halo_amd import _build, _lib
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        assert hasattr(h, s), s
        assert s in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 10 and _lib.lib().halo_version() == _lib.ABI_VERSION


def test_workspace_query_grows_with_the_output_image():
    from halo_amd import _lib
    q = _lib.lib().halo_upsampled_loss_workspace_bytes
    small, big = q(2, 19, 64, 128), q(2, 19, 640, 1280)
    assert 0 < small < big
    assert big >= 2 * (640 * 1280 // 1024) * 5 * 8                  # five float64 partials per 1024 output pixels and image
    assert q(4, 19, 640, 1280) > big
    assert q(0, 19, 64, 128) == 0 and q(2, 0, 64, 128) == 0 and q(2, 19, 0, 128) == 0


def _fwd(L, logit, label, ws, nws, B=1, K=19, h=4, w=8, H=16, W=32, dtype=2, terms=3, sums=None):
    return L.halo_upsampled_loss_fwd(logit, K * h * w, B, K, h, w, label, dtype, H, W, 255, 0.05, terms, sums, ws, nws, None)


def _bwd(L, logit, label, sums, grad, B=1, K=19, h=4, w=8, H=16, W=32, dtype=2, terms=3):
    return L.halo_upsampled_loss_bwd(logit, K * h * w, B, K, h, w, label, dtype, H, W, 255, 0.05, terms, sums, None, None, grad, None)


def test_argument_checks_refuse_before_launching():
    """Every case returns before a kernel could start: null pointers, and (with host addresses that are never dereferenced)
    empty shapes, too many classes, downsampling, an unknown label dtype, unknown term bits and a short workspace."""
    from halo_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.cast(buf, ctypes.c_void_p)
    nws = L.halo_upsampled_loss_workspace_bytes(1, 19, 16, 32)
    assert _fwd(L, None, None, None, 0) != 0
    assert _fwd(L, a, None, a, nws, sums=a) != 0
    assert _fwd(L, a, a, a, nws, sums=None) != 0
    assert _bwd(L, None, a, a, a) != 0
    assert _bwd(L, a, a, None, a) != 0
    assert _bwd(L, a, a, a, None) != 0
    for kw in ({"K": 0}, {"K": 1025}, {"H": 0}, {"W": 0}, {"B": 0}, {"H": 3}, {"W": 7}, {"dtype": 0}, {"dtype": 1}, {"dtype": 7},
               {"terms": 4}):
        assert _fwd(L, a, a, a, 1 << 16, sums=a, **kw) != 0, kw
        kb = {k: v for k, v in kw.items()}
        assert _bwd(L, a, a, a, a, **kb) != 0, kw
    assert _fwd(L, a, a, a, nws - 1, sums=a) == -3                  # HALO_E_WORKSPACE
    assert _fwd(L, a, a, None, nws, sums=a) != 0
    assert "workspace" in L.halo_last_error().decode()


def test_envelope_checks_raise_before_the_library():
    from halo_amd.training import upsampled_losses
    lg, lab = torch.zeros((1, 19, 4, 8)), torch.zeros((1, 16, 32), dtype=torch.int64)
    with pytest.raises(ValueError):
        upsampled_losses(lg, lab)                                    # CPU tensors: no CPU route
    with pytest.raises(TypeError):
        upsampled_losses(lg.double(), lab)
    with pytest.raises(TypeError):
        upsampled_losses(lg, lab.to(torch.int16))


def fixture_cases():
    z = np.load(FIX)
    return sorted({k.split("/")[0] for k in z.files if k.endswith("/values")})


@pytest.mark.parametrize("name", fixture_cases())
def test_fixture_equals_live_torch_cpu_chain(name):
    """the stored values are the torch chain's (the generator ran the reference's NegativeLearningLoss; this is its formula)"""
    z = np.load(FIX)
    lg, label = z[name + "/logits"], z[name + "/label"]
    x = torch.from_numpy(lg).requires_grad_(True)
    y = torch.from_numpy(label.astype(np.int64))
    up = F.interpolate(x, size=label.shape[-2:], mode="bilinear", align_corners=True)
    ce = nn.CrossEntropyLoss(ignore_index=255)(up, y)
    p = torch.softmax(up, dim=1)
    mask = (p < 0.05).detach()
    nl = torch.sum(-1 * mask * torch.log(1 - p + 1e-6)) / torch.sum(mask)
    want = z[name + "/values"]
    assert np.array_equal(np.array([ce.item(), nl.item()]), want, equal_nan=True)
    assert np.array_equal(np.array([int((y != 255).sum()), int(mask.sum())]), z[name + "/counts"])
    (g,) = torch.autograd.grad(nl, x)
    assert np.array_equal(g.numpy(), z[name + "/g_nl"])


def test_fixture_covers_the_cases_the_issue_lists():
    z = np.load(FIX)
    names = fixture_cases()
    assert {int(z[n + "/meta"][0]) for n in names} == {19, 16, 7}
    assert {z[n + "/label"].dtype for n in names} == {np.dtype(np.int64), np.dtype(np.int32), np.dtype(np.uint8)}
    empty = [n for n in names if int(z[n + "/counts"][0]) == 0]
    assert empty and all(np.isnan(z[n + "/values"][0]) and not z[n + "/g_ce"].any() for n in empty)
    assert "out of bounds" in str(z["k7_i64_bad_label/torch_error"])
    lab = z["k7_i64_bad_label/label"]
    assert ((lab >= 7) & (lab < 255)).any()


class SourceLearner(object):
    def training_step(self, batch, batch_idx):
        return "reference source"


class SourceFreeLearner(object):
    def training_step(self, batch, batch_idx):
        return "reference source-free"


class SourceTargetLearner(SourceFreeLearner):
    def training_step(self, batch, batch_idx):
        return "reference source-target"


class FullySupervisedLearner(SourceFreeLearner):
    def training_step(self, batch, batch_idx):
        return "reference fully-supervised"


def test_hook_picks_the_protocol_by_reference_class_name():
    from halo_amd.hooks import _training_protocol, fused_training_step, use_fused_training_losses
    for base in (SourceLearner, SourceFreeLearner, SourceTargetLearner, FullySupervisedLearner):
        sub = type("My" + base.__name__, (base,), {})
        assert _training_protocol(sub) == base.__name__
        use_fused_training_losses(sub)
        assert sub.training_step is fused_training_step
        assert sub._reference_training_step is base.__dict__["training_step"]
        assert base.training_step is not fused_training_step              # the base class is untouched
    assert _training_protocol(type("Deeper", (type("Mid", (SourceTargetLearner,), {}),), {})) == "SourceTargetLearner"


def test_hook_refuses_other_classes():
    from halo_amd.hooks import fused_training_step, use_fused_training_losses

    class Other(object):
        def training_step(self, batch, batch_idx):
            return None

    with pytest.raises(TypeError):
        use_fused_training_losses(Other)
    assert Other.__dict__["training_step"] is not fused_training_step
    with pytest.raises(TypeError):
        fused_training_step(Other(), {}, 0)


def test_hook_hands_an_unserved_head_output_to_the_reference_step():
    """a head that returns a bare tensor (the non-hyper DeepLab-v2 head) or CPU logits: the reference's own step runs"""
    from halo_amd.hooks import use_fused_training_losses

    class Learner(SourceFreeLearner):
        def __init__(self, out):
            self.cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=19), SOLVER=types.SimpleNamespace(NEGATIVE_LOSS=1.0))
            self.criterion = nn.CrossEntropyLoss(ignore_index=255)
            self.feature_extractor = lambda x: x
            self.classifier = lambda feat: out

        def optimizers(self):
            return []

    use_fused_training_losses(Learner)
    x = torch.zeros((1, 3, 16, 32))
    batch = {"img": x, "mask": torch.zeros((1, 16, 32), dtype=torch.int64)}
    assert Learner(torch.zeros((1, 19, 4, 8))).training_step(batch, 0) == "reference source-free"
    assert Learner((torch.zeros((1, 19, 4, 8)), None)).training_step(batch, 0) == "reference source-free"
