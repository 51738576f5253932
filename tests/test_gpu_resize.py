"""halo_amd.resize.bilinear_resize on the device (halo_bilinear_upsample forward, halo_resize.hip backward) and the
use_device_resize switch of the package's training paths.

Backward yardstick: a live CPU chain, torch's CPU autograd of F.interpolate(mode='bilinear', align_corners=True) in the same
dtype -- the same weights, another order of summation (tests/test_resize_host.py pins a numpy statement of the adjoint to it).
Tolerance, derived and not tuned: elementwise |got - want| <= 2 (n + 8) u A^T|g|, u the unit roundoff of the dtype, A^T|g| the
CPU backward applied to |g|, n = (2 ceil((H-1)/max(h-1,1)) + 1)(2 ceil((W-1)/max(w-1,1)) + 1) the terms of one sum at most
(recursive summation in two different orders plus the rounding of the weight products).  Where A^T|g| is 0 the result is 0."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def terms_bound(h, w, H, W):
    return (2 * math.ceil((H - 1) / max(h - 1, 1)) + 1) * (2 * math.ceil((W - 1) / max(w - 1, 1)) + 1)


def cpu_backward(g, in_shape):
    """torch's CPU autograd of F.interpolate at 4-d (B, C, h, w)"""
    x = torch.zeros(in_shape, dtype=g.dtype, requires_grad=True)
    y = F.interpolate(x, size=g.shape[-2:], mode="bilinear", align_corners=True)
    (gx,) = torch.autograd.grad(y, x, g)
    return gx


def device_backward(x, g, size):
    from halo_amd.resize import bilinear_resize
    x = x.detach().requires_grad_(True)
    y = bilinear_resize(x, size)
    (gx,) = torch.autograd.grad(y, x, g)
    return gx


def check_against_cpu(got, g_cpu, in_shape, tag):
    h, w = in_shape[-2:]
    H, W = g_cpu.shape[-2:]
    want = cpu_backward(g_cpu, in_shape).double()
    bound = 2 * (terms_bound(h, w, H, W) + 8) * U[g_cpu.dtype] * cpu_backward(g_cpu.abs(), in_shape).double()
    err = (got.cpu().double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max |err| = %.3g, max err / bound = %.3g" % (tag, float(err.max()), ratio))
    assert bool((err <= bound).all()), (tag, ratio)
    return bound


# (B, C, h, w, H, W): the four shapes of tools/time_resize.py, then a single cell, identity rows, odd sizes, x12.8
SHAPES = [(2, 256, 40, 80, 160, 320), (2, 19, 160, 320, 640, 1280), (2, 19, 180, 320, 720, 1280), (2, 64, 80, 160, 640, 1280),
          (2, 3, 1, 1, 40, 80), (2, 3, 24, 40, 24, 160), (2, 3, 33, 65, 129, 257), (1, 2, 80, 160, 1024, 2048)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d-%dx%d" % s)
def test_backward_against_cpu_chain(dev, shape, dtype):
    B, C, h, w, H, W = shape
    gen = torch.Generator().manual_seed(h * 7 + W)
    x = torch.zeros((B, C, h, w), dtype=dtype, device=dev)
    for kind in ("random", "ones"):
        g_cpu = torch.randn((B, C, H, W), dtype=dtype, generator=gen) if kind == "random" else torch.ones((B, C, H, W), dtype=dtype)
        got = device_backward(x, g_cpu.to(dev), (H, W))
        assert got.shape == x.shape and got.dtype == dtype
        check_against_cpu(got, g_cpu, (B, C, h, w), "%s %s %s" % (shape, dtype, kind))
        if kind == "ones":
            # the weights of an output pixel sum to 1: every plane's gradient sums to H * W
            sums = got.double().sum(dim=(-2, -1)).cpu()
            tol = 2 * (terms_bound(h, w, H, W) + 8) * U[dtype] * H * W
            print("plane sums: max |sum - H W| = %.3g, tol %.3g" % (float((sums - H * W).abs().max()), tol))
            assert bool(((sums - H * W).abs() <= tol).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_forward_is_bilinear_align_corners(dev, dtype):
    from halo_amd.core.utils.hyperbolic import bilinear_align_corners
    from halo_amd.resize import bilinear_resize
    torch.manual_seed(3)
    for shape, size in (((2, 19, 40, 80), (160, 320)), ((2, 3, 33, 65), (129, 257)), ((3, 9, 16), (36, 65)), ((5, 7), (11, 20))):
        x = torch.randn(shape, dtype=dtype, device=dev)
        with torch.no_grad():
            want = bilinear_align_corners(x, size)
            assert torch.equal(bilinear_resize(x, size), want)
        assert not bilinear_resize(x, size).requires_grad
        y = bilinear_resize(x.clone().requires_grad_(True), size)    # under autograd: the same kernel, the same bits
        assert y.requires_grad and torch.equal(y.detach(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_backward_is_bit_reproducible_also_on_a_side_stream(dev, dtype):
    torch.manual_seed(4)
    for (B, C, h, w, H, W) in ((2, 19, 45, 80, 180, 320), (2, 8, 20, 40, 256, 512), (1, 3, 1, 1, 40, 80)):
        x = torch.zeros((B, C, h, w), dtype=dtype, device=dev)
        g = torch.randn((B, C, H, W), dtype=dtype, device=dev)
        a, b = device_backward(x, g, (H, W)), device_backward(x, g, (H, W))
        assert torch.equal(a, b)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            c = device_backward(x, g, (H, W))
        side.synchronize()
        torch.cuda.current_stream(dev).wait_stream(side)
        assert torch.equal(a, c)


def test_gradcheck_float64(dev):
    from halo_amd.resize import bilinear_resize
    torch.manual_seed(5)
    x = torch.randn((2, 3, 5, 7), dtype=torch.float64, device=dev, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: bilinear_resize(t, (11, 20)), (x,), nondet_tol=0.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_strided_operands_give_equal_bits(dev, dtype):
    from halo_amd.resize import bilinear_resize
    torch.manual_seed(6)
    base = torch.randn((2, 5, 12, 40), dtype=dtype, device=dev)
    gbase = torch.randn((2, 5, 48, 160), dtype=dtype, device=dev)
    xs, gs = base[..., ::2], gbase[..., ::2]                         # (2, 5, 12, 20) and (2, 5, 48, 80), neither contiguous
    assert not xs.is_contiguous() and not gs.is_contiguous()
    outs = []
    for x, g in ((xs, gs), (xs.contiguous(), gs.contiguous()), (xs.contiguous().permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3), gs)):
        x = x.detach().requires_grad_(True)
        y = bilinear_resize(x, (48, 80))
        (gx,) = torch.autograd.grad(y, x, g)
        assert gx.shape == x.shape and gx.dtype == dtype
        outs.append((y.detach(), gx))
    for y, gx in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(gx, outs[0][1])
    # an odd width and an unaligned base take the scalar staging path: same definition
    g_cpu = torch.randn((1, 3, 37, 51), dtype=dtype)
    got = device_backward(torch.zeros((1, 3, 9, 13), dtype=dtype, device=dev), g_cpu.to(dev), (37, 51))
    check_against_cpu(got, g_cpu, (1, 3, 9, 13), "odd width %s" % dtype)
    flat = torch.randn(3 * 36 * 52 + 1, dtype=dtype, device=dev)
    g_dev = flat[1:].view(1, 3, 36, 52)                              # contiguous, 4 or 8 bytes off a 16-byte boundary
    got = device_backward(torch.zeros((1, 3, 9, 13), dtype=dtype, device=dev), g_dev, (36, 52))
    check_against_cpu(got, g_dev.cpu(), (1, 3, 9, 13), "unaligned %s" % dtype)


def test_offsets_beyond_2_to_31_elements(dev):
    """520 planes of 2048 x 2048 float32: 2.18e9 gradient elements.  Planes are independent, so the first and the last two are
    held to the CPU chain (random values there; the planes between hold ones and must sum to H W each)."""
    P, h, w, H, W = 520, 512, 512, 2048, 2048
    assert P * H * W > 2 ** 31
    g = torch.ones((1, P, H, W), dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(8)
    edge = torch.randn((1, 3, H, W), dtype=torch.float32, generator=gen)
    g[:, 0] = edge[:, 0].to(dev)
    g[:, -2:] = edge[:, 1:].to(dev)
    from halo_amd import _lib
    got = torch.empty((1, P, h, w), dtype=torch.float32, device=dev)     # the entry point itself: no forward, no second 8.7 GB map
    _lib.check(_lib.lib().halo_bilinear_upsample_bwd(_lib.ptr(g), _lib.ptr(got), _lib.F32, P, h, w, H, W, _lib.stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    del g
    check_against_cpu(torch.cat([got[:, :1], got[:, -2:]], 1), edge, (1, 3, h, w), "beyond 2^31")
    sums = got[0, 1:-2].double().sum(dim=(-2, -1)).cpu()
    assert bool(((sums - H * W).abs() <= 2 * (terms_bound(h, w, H, W) + 8) * U[torch.float32] * H * W).all())


# ---------------------------------------------------------------- the switch on stand-in heads and a stand-in learner
def grads_close(got, want):
    """the project's hooked-vs-unhooked rule (tests/test_gpu_upsampled_loss.py)"""
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    return np.abs(got - want).max() <= 2e-5 * np.abs(want).max() + 1e-12


@pytest.fixture
def resize_inputs(monkeypatch):
    """records the gradient arriving at every operand of halo_amd.resize.resize_or_interpolate (a tensor hook)"""
    import halo_amd.resize as rz
    seen = []
    inner = rz.resize_or_interpolate

    def recording(x, size):
        if x.requires_grad:
            x.register_hook(lambda g: seen.append(g.detach().clone()))
        return inner(x, size)

    monkeypatch.setattr(rz, "resize_or_interpolate", recording)
    return seen


def test_marked_v2_head(dev, resize_inputs):
    """DeepLab-v2 tail: the resize is the head's last statement, so the outputs ARE the resized tensors.  Marked against unmarked
    within 8 u max|x| (three roundings per bilerp on each side), parameter gradients within the hooked-vs-unhooked rule, two
    marked steps bit-equal behind the resize; the unmarked class returns today's statements' bits."""
    from halo_amd.core.models.classifier import ASPP_Classifier_V2_Hyper
    from halo_amd.hooks import use_device_resize

    class Marked(ASPP_Classifier_V2_Hyper):
        pass

    assert use_device_resize(Marked) is Marked and not getattr(ASPP_Classifier_V2_Hyper, "_halo_device_resize", False)
    torch.manual_seed(12)
    plain = ASPP_Classifier_V2_Hyper(8, [1, 2], [1, 2], 19, 16).to(dev).train()
    for m in plain.conv2d_list:
        m.weight.data.normal_(0, 0.3)
    marked = Marked(8, [1, 2], [1, 2], 19, 16).to(dev).train()
    marked.load_state_dict(plain.state_dict())
    feats = {"out": torch.randn(2, 8, 23, 40, device=dev)}
    size = (92, 161)

    def step(head):
        out, embed = head(feats, size=size)
        loss = out.square().mean() + (embed * embed).mean()
        return out.detach(), embed.detach(), torch.autograd.grad(loss, list(head.parameters()))

    po, pe, pg = step(plain)
    assert not resize_inputs                                         # the unmarked class never reaches the device resize
    mo, me, mg = step(marked)
    first = list(resize_inputs)
    assert len(first) == 2                                           # logits and embedding
    with torch.no_grad():
        lo, le = plain(feats)                                        # the low-resolution operands of both resizes
    assert float((mo - po).abs().max()) <= 8 * U[torch.float32] * float(lo.abs().max())
    assert float((me - pe).abs().max()) <= 8 * U[torch.float64] * float(le.abs().max())
    for a, b in zip(mg, pg):
        assert grads_close(a, b)
    del resize_inputs[:]
    mo2, me2, mg2 = step(marked)
    assert torch.equal(mo, mo2) and torch.equal(me, me2)
    assert len(resize_inputs) == 2 and all(torch.equal(a, b) for a, b in zip(first, resize_inputs))
    names = [n for n, _ in marked.named_parameters()]
    for n in ("conv_seg.P_MLR", "conv_seg.A_MLR"):                  # HyperMLR's own deterministic backward sits behind the resize
        assert torch.equal(mg[names.index(n)], mg2[names.index(n)])
    # unmarked: today's statements, bit for bit
    embed = plain.mapper.expmap(sum(conv(feats["out"]) for conv in plain.conv2d_list), dim=1)
    out = plain.conv_seg._hyper_logits(embed, out_dtype=torch.float32)
    assert torch.equal(po, F.interpolate(out, size=size, mode="bilinear", align_corners=True).detach())
    assert torch.equal(pe, F.interpolate(embed, size=size, mode="bilinear", align_corners=True).detach())
    with torch.no_grad():
        eo, ee = plain(feats, size=size)
        ko, ke = marked(feats, size=size)
    assert torch.equal(eo, ko) and torch.equal(ee, ke)             # inference: both classes run bilinear_align_corners


class _V3Head(nn.Module):
    """a stand-in v3+ hyperbolic head with the reference's attribute names (small layers)"""

    def __init__(self, C=64, K=5):
        super().__init__()
        from halo_amd.core.utils.hyperbolic import HyperMapper, HyperMLR
        self.parallel_branches = nn.ModuleList([nn.Conv2d(8, 8, 1), nn.Conv2d(8, 8, 3, padding=1)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(8, 8, 1))
        self.bottleneck = nn.Conv2d(24, 16, 1)
        self.shortcut = nn.Conv2d(4, 4, 1)
        self.decoder = nn.Conv2d(20, 16, 3, padding=1)
        self.conv_reduce = nn.Conv2d(16, C, 1)
        self.mapper = HyperMapper(c=1.0)
        self.conv_seg = HyperMLR(C, K, c=1.0)


@pytest.mark.parametrize("fused", [False, True], ids=["v3plus_hyper_forward", "fused_v3plus_hyper_forward"])
def test_marked_v3plus_head(dev, resize_inputs, fused):
    """Here the body resize feeds the decoder, so the outputs carry its rounding through convolutions and the hyperbolic tail: they
    are held to the project's hooked-vs-unhooked rule for float32 heads (2e-5 of the largest value, as tests/test_gpu_hfr.py
    holds its hooked head), the parameter gradients to the same rule; the gradients arriving at the two device resizes are
    bit-equal from step to step (the parameters behind them are convolution weights, whose backward is MIOpen's)."""
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import fused_v3plus_hyper_forward, use_device_resize, use_fused_feature_reweighting

    class Plain(_V3Head):
        forward = v3plus_hyper_forward

    class Marked(_V3Head):
        forward = v3plus_hyper_forward

    if fused:
        use_fused_feature_reweighting(Plain)
        use_fused_feature_reweighting(Marked)
    use_device_resize(Marked)
    assert Marked.forward is (fused_v3plus_hyper_forward if fused else v3plus_hyper_forward)
    torch.manual_seed(13)
    plain, marked = Plain().to(dev).train(), Marked().to(dev).train()
    marked.load_state_dict(plain.state_dict())
    feats = {"low": torch.randn(2, 4, 24, 40, device=dev), "out": torch.randn(2, 8, 12, 20, device=dev)}
    size = (96, 160)

    def step(head):
        out, embed = head(feats, size=size)
        loss = out.square().mean() + embed.sum()
        return out.detach(), embed.detach(), torch.autograd.grad(loss, list(head.parameters()))

    po, pe, pg = step(plain)
    assert not resize_inputs
    mo, me, mg = step(marked)
    first = list(resize_inputs)
    assert len(first) == 2                                           # the bottleneck's output and the logits; the pooled map is an expand
    assert grads_close(mo, po) and grads_close(me, pe)
    for a, b in zip(mg, pg):
        assert grads_close(a, b)
    del resize_inputs[:]
    mo2, _, _ = step(marked)
    assert torch.equal(mo, mo2)
    assert len(resize_inputs) == 2 and all(torch.equal(a, b) for a, b in zip(first, resize_inputs))
    # unmarked: the reference's statements, bit for bit
    pyramid = [branch(feats["out"]) for branch in plain.parallel_branches]
    pyramid.append(F.interpolate(plain.global_branch(feats["out"]), size=(12, 20), mode="bilinear", align_corners=True))
    body = F.interpolate(plain.bottleneck(torch.cat(pyramid, dim=1)), size=(24, 40), mode="bilinear", align_corners=True)
    dec = plain.conv_reduce(plain.decoder(torch.cat([body, plain.shortcut(feats["low"])], dim=1)))
    embed = plain.mapper.expmap(dec, dim=1)
    out = F.interpolate(plain.conv_seg._hyper_logits(embed, out_dtype=torch.float32), size=size, mode="bilinear", align_corners=True)
    assert torch.equal(po, out.detach()) and torch.equal(pe, embed.detach())


class _Backbone(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv = nn.Conv2d(3, C, kernel_size=8, stride=8)

    def forward(self, x):
        return {"out": self.conv(x)}


class _NoStep(object):
    def __init__(self, params):
        self.params = list(params)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        pass


class SourceTargetLearner(object):
    """what halo_amd.hooks.fused_training_step reads of the reference's learner of that name"""

    def __init__(self, dev, K=19, C=8):
        from halo_amd.core.loss import LocalConsistentLoss
        from halo_amd.core.models.classifier import ASPP_Classifier_V2_Hyper
        torch.manual_seed(0)
        self.cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=K), SOLVER=types.SimpleNamespace(NEGATIVE_LOSS=1.0, CONSISTENT_LOSS=0.5))
        self.feature_extractor = _Backbone(C).to(dev)
        self.classifier = ASPP_Classifier_V2_Hyper(C, [1, 2], [1, 2], K, C).to(dev)
        for m in self.classifier.conv2d_list:
            m.weight.data.normal_(0, 0.3)
        self.criterion = nn.CrossEntropyLoss(ignore_index=255)
        self.negative_criterion = types.SimpleNamespace(threshold=0.05)
        self.local_consistent_loss = LocalConsistentLoss(K, "l1")
        self._opt = _NoStep(list(self.feature_extractor.parameters()) + list(self.classifier.parameters()))
        self.logged = {}

    def training_step(self, batch, batch_idx):
        raise AssertionError("the reference's own step is not expected to run here")

    def optimizers(self):
        return [self._opt]

    def lr_schedulers(self):
        return []

    def log_metrics(self, batch_idx):
        pass

    def manual_backward(self, loss):
        loss.backward()

    def log(self, name, value, **kw):
        self.logged[name] = float(value)

    def grads(self):
        return [p.grad.detach().clone() for p in self._opt.params]


def test_marked_learner_builds_the_consistency_input_on_the_device(dev, resize_inputs):
    from halo_amd.hooks import use_device_resize, use_fused_training_losses

    class Hooked(SourceTargetLearner):
        pass

    class Marked(SourceTargetLearner):
        pass

    use_fused_training_losses(Hooked)
    use_fused_training_losses(use_device_resize(Marked))
    rng = np.random.default_rng(22)

    def image_batch(H, W, key, frac):
        y = rng.integers(0, 19, (2, H, W))
        y[rng.random((2, H, W)) >= frac] = 255
        return {"img": torch.from_numpy(rng.standard_normal((2, 3, H, W), dtype=np.float32)).to(dev), key: torch.from_numpy(y).to(dev)}

    batch = [image_batch(72, 128, "label", 0.9), image_batch(64, 128, "mask", 0.05)]
    hooked, marked = Hooked(dev), Marked(dev)
    hooked.training_step(batch, 0)
    assert not resize_inputs
    marked.training_step(batch, 0)
    first, g1 = list(resize_inputs), marked.grads()
    assert len(first) == 1 and first[0].shape == (2, 19, 9, 16)       # the source logits, resized for LocalConsistentLoss
    assert sorted(hooked.logged) == sorted(marked.logged) and "consistency_loss" in marked.logged
    for k, want in hooked.logged.items():
        assert abs(marked.logged[k] - want) <= 1e-5 * abs(want) + 1e-12, (k, marked.logged[k], want)
    for a, b in zip(g1, hooked.grads()):
        assert grads_close(a, b)
    del resize_inputs[:]
    marked.training_step(batch, 0)
    assert len(resize_inputs) == 1 and torch.equal(first[0], resize_inputs[0])


def test_switch_falls_back_inside_a_step_instead_of_raising(dev):
    """an operand the device resize refuses (float16, downsampling) takes F.interpolate under the switch"""
    from halo_amd.resize import resize_or_interpolate
    x = torch.randn((1, 2, 8, 8), device=dev)
    assert torch.equal(resize_or_interpolate(x, (4, 4)), F.interpolate(x, size=(4, 4), mode="bilinear", align_corners=True))
    xh = x.half().requires_grad_(True)
    y = resize_or_interpolate(xh, (16, 16))
    assert y.dtype == torch.float16 and y.requires_grad
    y.sum().backward()
    assert xh.grad is not None
