"""halo_amd.optim.fuse_step against the stock optimiser steps on the same device, bit for bit.

geoopt mode is compared with tests/optim_ref.py (geoopt's RiemannianSGD.step restated in stock torch statements, run live on the
device), torch mode with torch.optim.SGD as constructed by default (its foreach form on a device) and with foreach=False.  Every
case runs three consecutive steps at three learning rates from a real SequentialLR(LinearLR, PolynomialLR) and compares the
parameters, the momentum buffers and -- in geoopt mode, whose step rewrites it -- p.grad after each.  Integer views are compared;
NaNs must sit at the same places.  Which of ATen's statements contract to one fma on the device is thereby decided by the device:
a statement that rounded otherwise than halo_optim.hip says would fail every case here.
"""
import copy
import warnings

import numpy as np
import pytest
import torch
from torch import nn
from torch.optim.lr_scheduler import LinearLR, PolynomialLR, SequentialLR

from optim_ref import RiemannianSGD

pytestmark = pytest.mark.gpu

LEARNER_HYPER = dict(momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)
SIZES = ["0", "1", "3", "4", "5", "63", "64", "65", "255", "256", "257", "1023", "1025", "CH-1", "CH", "CH+1", "3*CH+7"]
REFERENCES = {"geoopt": ["restatement"], "torch": ["default", "single"]}
MODE_REFS = [(m, r) for m in ("geoopt", "torch") for r in REFERENCES[m]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def limits():
    from halo_amd import optim
    return optim.plan_limits()


def _size(text, chunk):
    return int(eval(text, {"CH": chunk}))


def same_bits(a, b):
    """equal integer views, NaNs at the same places (a NaN's payload is not compared)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    ints = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.contiguous().view(ints)[~na], b.contiguous().view(ints)[~na])


def values(rng, shape, dtype, special):
    """N(0, 1) with, scattered over a fifth of the places when `special`: NaN, +-inf, -0.0, float32 denormals and values whose product
    with a learning rate of 1e-3 .. 1e-1 is a float32 denormal"""
    x = rng.standard_normal(shape)
    if special and x.size:
        pool = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, 1.4e-45, 2e-37, -5e-38, 1.2e-38, 3e38, -3e38])
        at = rng.random(shape) < 0.2
        x[at] = rng.choice(pool, size=int(at.sum()))
    return torch.from_numpy(np.asarray(x)).to(dtype)


def make_optimizer(mode, reference, groups):
    if mode == "geoopt":
        return RiemannianSGD(groups, lr=0.01)
    return torch.optim.SGD(groups, lr=0.01) if reference == "default" else torch.optim.SGD(groups, lr=0.01, foreach=False)


def schedule(opt):
    """the learner's scheduler (core/train_learners.py:188-192) with a short warm-up: a different learning rate at every step"""
    return SequentialLR(opt, schedulers=[LinearLR(opt, start_factor=0.01, total_iters=2), PolynomialLR(opt, 6, power=0.9)], milestones=[2])


def offset_view(t, misaligned):
    """a copy of t whose first element sits one element into its storage when `misaligned`: off the 16-byte boundary"""
    if not misaligned:
        return t.clone()
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


class Twin:
    """the same param groups twice: one optimiser left as it is, one converted by fuse_step; both scheduled before the conversion,
    as the learner's configure_optimizers does"""

    def __init__(self, dev, mode, reference, specs, special=True, seed=0, misalign=()):
        """specs: one list per group of (shape, dtype) and the group's options"""
        from halo_amd.optim import fuse_step
        self.rng = np.random.default_rng(seed)
        self.mode, self.dev, self.special, self.misalign = mode, dev, special, misalign
        self.ref_params, self.got_params = [], []
        ref_groups, got_groups = [], []
        for shapes, options in specs:
            init = [values(self.rng, shape, dtype, special).to(dev) for shape, dtype in shapes]
            a = [nn.Parameter(offset_view(t, "p" in misalign)) for t in init]
            b = [nn.Parameter(offset_view(t, "p" in misalign)) for t in init]
            self.ref_params += a
            self.got_params += b
            ref_groups.append(dict(params=a, **options))
            got_groups.append(dict(params=b, **options))
        self.ref = make_optimizer(mode, reference, ref_groups)
        self.got = make_optimizer(mode, reference, got_groups)
        self.ref_sched, self.got_sched = schedule(self.ref), schedule(self.got)
        assert fuse_step(self.got) is self.got
        self.lrs = []

    def step(self, present=None, expect_reason=None):
        """one step on fresh gradients (new tensors, as a backward leaves them); present[i] False: parameter i gets none"""
        for i, (p, q) in enumerate(zip(self.ref_params, self.got_params)):
            if present is not None and not present[i]:
                p.grad = q.grad = None
                continue
            g = values(self.rng, tuple(p.shape), p.dtype, self.special).to(self.dev)
            p.grad, q.grad = offset_view(g, "g" in self.misalign), offset_view(g, "g" in self.misalign)
        self.lrs.append([g["lr"] for g in self.got.param_groups])
        self.ref.step()
        self.got.step()
        self.ref_sched.step()
        self.got_sched.step()
        if expect_reason is None:
            assert self.got.fallback_reason is None, self.got.fallback_reason
        else:
            assert expect_reason in self.got.fallback_reason
        self.compare()

    def compare(self):
        assert [g["lr"] for g in self.ref.param_groups] == [g["lr"] for g in self.got.param_groups]
        for i, (p, q) in enumerate(zip(self.ref_params, self.got_params)):
            assert same_bits(p.detach(), q.detach()), "parameter %d %s" % (i, tuple(p.shape))
            sp, sq = self.ref.state.get(p), self.got.state.get(q)
            assert (sp is None) == (sq is None) and sorted(sp or ()) == sorted(sq or ()), "state keys of parameter %d" % i
            if sp and "momentum_buffer" in sp:
                assert same_bits(sp["momentum_buffer"], sq["momentum_buffer"]), "momentum buffer %d %s" % (i, tuple(p.shape))
            assert (p.grad is None) == (q.grad is None)
            if self.mode == "geoopt" and p.grad is not None:
                assert same_bits(p.grad, q.grad), "gradient %d %s" % (i, tuple(p.shape))

    def misalign_buffers(self):
        """move every momentum buffer of both optimisers one element into a storage of its own"""
        for opt in (self.ref, self.got):
            for st in opt.state.values():
                st["momentum_buffer"] = offset_view(st["momentum_buffer"], True)


def run_three(twin, **kw):
    for _ in range(3):
        twin.step(**kw)
    assert len({tuple(l) for l in twin.lrs}) == 3                  # three different learning rates were stepped with


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode,reference", MODE_REFS)
def test_one_parameter_of_each_size(dev, limits, mode, reference, dtype, size):
    n = _size(size, limits[0])
    run_three(Twin(dev, mode, reference, [([((n,), dtype)], LEARNER_HYPER)], seed=n % 1000))


@pytest.mark.parametrize("which", ["p", "g", "buf"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode,reference", MODE_REFS)
def test_one_operand_off_the_16_byte_boundary(dev, limits, mode, reference, dtype, which):
    twin = Twin(dev, mode, reference, [([((limits[0] + 9,), dtype), ((3, 7), dtype)], LEARNER_HYPER)], seed=3,
                misalign=() if which == "buf" else (which,))
    twin.step()
    if which == "buf":
        twin.misalign_buffers()
        assert all(st["momentum_buffer"].data_ptr() % 16 != 0 for st in twin.got.state.values())
    twin.step()
    twin.step()
    for p in twin.got_params:                                      # the case is what it says: exactly one operand is off
        st = twin.got.state[p]
        assert [p.data_ptr() % 16 != 0, p.grad.data_ptr() % 16 != 0, st["momentum_buffer"].data_ptr() % 16 != 0] == [which == k for k in ("p", "g", "buf")]


HYPERS = [dict(momentum=m, dampening=d, weight_decay=wd, nesterov=False) for m in (0.0, 0.9) for d in (0.0, 0.1) for wd in (0.0, 5e-4)] + \
         [dict(momentum=0.9, dampening=0.0, weight_decay=wd, nesterov=True) for wd in (0.0, 5e-4)]


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "m%g-d%g-wd%g-%s" % (h["momentum"], h["dampening"], h["weight_decay"], "nag" if h["nesterov"] else "plain"))
@pytest.mark.parametrize("mode,reference", MODE_REFS)
def test_hyper_parameters_and_two_groups(dev, limits, mode, reference, hyper):
    """every combination of the hyper-parameters on a group of mixed dtypes, and a second group at ten times the learning rate"""
    first = [((5,), torch.float32), ((19, 64), torch.float64), ((limits[0] + 1,), torch.float32), ((257,), torch.float64)]
    second = [((33, 3), torch.float32), ((19, 64), torch.float64)]
    twin = Twin(dev, mode, reference, [(first, dict(hyper)), (second, dict(hyper, lr=0.1))], seed=11)
    run_three(twin)
    assert twin.lrs[0][1] == pytest.approx(10 * twin.lrs[0][0])


@pytest.mark.parametrize("mode,reference", MODE_REFS)
def test_one_group_of_many_tensors_mixed_dtypes_late_and_missing_gradients(dev, limits, mode, reference):
    cap = limits[1]
    shapes = [((300,), torch.float32), ((19, 64), torch.float64)] + [((5,), torch.float32)] * (cap + 1) + \
             [((19, 64), torch.float64), ((7,), torch.float32), ((9,), torch.float64), ((limits[0] + 3,), torch.float32)]
    late, never = 3, len(shapes) - 3                               # late sits in the first launch's table, never in the second's
    twin = Twin(dev, mode, reference, [(shapes, LEARNER_HYPER)], seed=17)
    present = [True] * len(shapes)
    present[never] = False
    present[late] = False
    twin.step(present=present)
    assert twin.got_params[late] not in twin.got.state and twin.got_params[never] not in twin.got.state
    present[late] = True                                           # its first use comes one step after its neighbours'
    twin.step(present=present)
    twin.step(present=present)
    assert twin.got_params[never] not in twin.got.state and "momentum_buffer" in twin.got.state[twin.got_params[late]]
    assert len({tuple(l) for l in twin.lrs}) == 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_infinite_parameters_without_weight_decay_differ_in_kind(dev, dtype):
    """wd = 0, p = +-inf, finite gradients: geoopt's step adds 0 * inf to the gradient and the parameter ends as NaN; torch's adds
    nothing and the parameter stays where it was.  Both are also what the stock steps do (the Twin compares)."""
    from halo_amd.optim import fuse_step
    hyper = dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False)
    n = 300
    at = torch.arange(n, device=dev) % 7 == 3
    sign = torch.where(torch.arange(n, device=dev) % 2 == 0, 1.0, -1.0).to(dtype)
    out = {}
    for mode, reference in MODE_REFS:
        twin = Twin(dev, mode, reference, [([((n,), dtype)], hyper)], special=False, seed=23)
        with torch.no_grad():
            for p in (twin.ref_params[0], twin.got_params[0]):
                p[at] = (sign * float("inf"))[at]
        twin.step()
        out[mode] = twin.got_params[0].detach().clone()
        assert torch.isfinite(out[mode][~at]).all()
    assert torch.isnan(out["geoopt"][at]).all()
    assert torch.equal(out["torch"][at], (sign * float("inf"))[at])


@pytest.mark.parametrize("mode,reference", MODE_REFS)
def test_an_unserved_group_runs_the_stock_step(dev, mode, reference):
    """a non-contiguous parameter: its group steps as the unconverted optimiser steps it, the other group stays on the kernel"""
    from halo_amd.optim import fuse_step
    rng = np.random.default_rng(29)
    init = [values(rng, (6, 4), torch.float32, False).to(dev), values(rng, (40,), torch.float32, False).to(dev)]
    params = [[nn.Parameter(init[0].clone().t()), nn.Parameter(init[1].clone())] for _ in range(2)]
    assert not params[0][0].is_contiguous()
    opts = [make_optimizer(mode, reference, [dict(params=[p[0]], **LEARNER_HYPER), dict(params=[p[1]], lr=0.1, **LEARNER_HYPER)]) for p in params]
    scheds = [schedule(o) for o in opts]
    fuse_step(opts[1])
    assert "param group 0: a non-contiguous parameter" == opts[1].fallback_reason
    for _ in range(3):
        grads = [values(rng, tuple(p.shape), torch.float32, False).to(dev) for p in params[0]]
        for ps in params:
            for p, g in zip(ps, grads):
                p.grad = g.clone()
        for o, s in zip(opts, scheds):
            o.step()
            s.step()
        assert opts[1].group_fallback_reasons == ["a non-contiguous parameter", None]
        for p, q in zip(*params):
            assert same_bits(p.detach(), q.detach())
            assert same_bits(opts[0].state[p]["momentum_buffer"], opts[1].state[q]["momentum_buffer"])
            if mode == "geoopt":
                assert same_bits(p.grad, q.grad)


# ---------------------------------------------------------------- the learner pattern (tests/test_gpu_upsampled_loss.py's stand-in)
class StandInLearner(object):
    """optimizers() / lr_schedulers() / manual_backward around a two-layer model, configure_optimizers as the reference states it
    (core/train_learners.py:167-208): two optimisers, the head at ten times the learning rate, warm-up then polynomial decay"""

    def __init__(self, dev, hyper):
        torch.manual_seed(3)
        self.hyper = hyper
        self.feature_extractor = nn.Sequential(nn.Linear(16, 32), nn.BatchNorm1d(32), nn.ReLU()).to(dev)
        self.classifier = nn.Linear(32, 4).to(dev)
        if hyper:                                                  # the hyperbolic head's float64 pair (core/utils/hyperbolic.py:115-116)
            self.classifier.P_MLR = nn.Parameter(torch.randn(4, 32, dtype=torch.float64, device=dev) * 0.05)
        self._optimizers, self._schedulers = self.configure_optimizers()

    def configure_optimizers(self):
        optim = RiemannianSGD if self.hyper else torch.optim.SGD
        optimizer_fea = optim(self.feature_extractor.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4)
        optimizer_cls = optim(self.classifier.parameters(), lr=0.01 * 10, momentum=0.9, weight_decay=5e-4)
        return [optimizer_fea, optimizer_cls], [schedule(optimizer_fea), schedule(optimizer_cls)]

    def optimizers(self):
        return self._optimizers

    def lr_schedulers(self):
        return self._schedulers

    def manual_backward(self, loss):
        loss.backward()

    def training_step(self, batch, batch_idx):
        for opt in self.optimizers():
            opt.zero_grad()
        x, y = batch
        feat = self.feature_extractor(x)
        out = self.classifier(feat)
        if self.hyper:
            out = out + (feat.double() @ self.classifier.P_MLR.t()).float()
        loss = nn.functional.cross_entropy(out, y)
        self.manual_backward(loss)
        for opt in self.optimizers():
            opt.step()
        for sched in self.lr_schedulers():
            sched.step()

    def tensors(self):
        mods = (self.feature_extractor, self.classifier)
        return [t.detach() for m in mods for t in list(m.parameters()) + list(m.buffers())]


def same_state_dict(a, b):
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(same_state_dict(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_state_dict(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)
    return a == b


@pytest.mark.parametrize("hyper", [True, False], ids=["hyper", "euclid"])
def test_hooked_learner_trains_like_the_unhooked(dev, hyper):
    from halo_amd.hooks import use_fused_optimizer_step

    class Hooked(StandInLearner):
        pass

    assert use_fused_optimizer_step(Hooked) is Hooked
    rng = np.random.default_rng(31)
    batches = [(torch.from_numpy(rng.standard_normal((8, 16)).astype(np.float32)).to(dev), torch.from_numpy(rng.integers(0, 4, 8)).to(dev))
               for _ in range(6)]
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)                # e.g. "lr_scheduler.step() before optimizer.step()"
        plain, hooked = StandInLearner(dev, hyper), Hooked(dev, hyper)
        assert all(type(o).__dict__.get("_halo_fused_mode") == ("geoopt" if hyper else "torch") for o in hooked.optimizers())
        assert all(o.fallback_reason is None for o in hooked.optimizers())
        for i, batch in enumerate(batches[:5]):
            plain.training_step(batch, i)
            hooked.training_step(batch, i)
        assert all(o.fallback_reason is None for o in hooked.optimizers())
    for a, b in zip(plain.tensors(), hooked.tensors()):
        assert same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)
    for o, f in zip(plain.optimizers(), hooked.optimizers()):
        assert same_state_dict(o.state_dict(), f.state_dict())
    # a state_dict saved from either loads into the other: swap them, step once more, still the same bits
    saved = [(copy.deepcopy(o.state_dict()), copy.deepcopy(f.state_dict())) for o, f in zip(plain.optimizers(), hooked.optimizers())]
    for (from_plain, from_hooked), o, f in zip(saved, plain.optimizers(), hooked.optimizers()):
        o.load_state_dict(from_hooked)
        f.load_state_dict(from_plain)
    plain.training_step(batches[5], 5)
    hooked.training_step(batches[5], 5)
    for a, b in zip(plain.tensors(), hooked.tensors()):
        assert same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)
    for o, f in zip(plain.optimizers(), hooked.optimizers()):
        assert same_state_dict(o.state_dict(), f.state_dict())
