"""Host-side checks of the fused optimiser step (halo_optim.hip, halo_amd/optim.py, the hook): no GPU, no kernel launch."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from optim_ref import RiemannianSGD

SYMBOLS = ("halo_sgd_plan_limits", "halo_sgd_plan", "halo_sgd_step")
E_ARG, E_UNSUPPORTED = -1, -2


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo_hip.h")).read(), flags=re.S)


def test_header_table_and_library_agree_and_the_abi_is_13():
    from halo_amd import _build, _lib
    text = _header()
    h = ctypes.CDLL(_build.build())
    for s in SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % s, text)
        assert decl, "%s is not declared" % s
        assert s in _lib.SIGNATURES and hasattr(h, s), s
        restype, argtypes = _lib.SIGNATURES[s]
        assert restype is ctypes.c_int and len(argtypes) == len(decl.group(1).split(",")), s
    assert "halo_optim.hip" in _build.SOURCES
    assert _lib.ABI_VERSION == 13 and "#define HALO_ABI_VERSION 13" in text and _lib.lib().halo_version() == 13
    assert "#define HALO_SGD_GEOOPT %d" % _lib.SGD_GEOOPT in text and "#define HALO_SGD_TORCH %d" % _lib.SGD_TORCH in text


@pytest.mark.parametrize("struct,cls", [("halo_sgd_tensor", "SgdTensor"), ("halo_sgd_args", "SgdArgs")])
def test_descriptor_layouts_are_the_headers(tmp_path, struct, cls):
    from halo_amd import _build, _lib
    binding = getattr(_lib, cls)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), flags=re.S).group(1)
    declared = [re.search(r"(\w+)\s*$", stmt).group(1) for stmt in body.split(";") if stmt.strip()]
    names = [f[0] for f in binding._fields_]
    assert declared == names
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "halo_hip.h"\nint main(void)\n{\n'
                   '    printf("%%zu\\n", sizeof(%s));\n' % struct
                   + "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (struct, f) for f in declared) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run([_build.host_cc(), "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(binding)
    assert got[1:] == [getattr(binding, f).offset for f in names]


def test_plan_limits_are_a_pure_host_query():
    from halo_amd import _lib, optim
    chunk, cap = optim.plan_limits()
    assert chunk >= 1024 and chunk % 1024 == 0            # 256 lanes x 16 bytes of either dtype divide it
    assert cap >= 2 and cap * (3 * 8 + 4 + 4 + 1) + 64 <= 4096          # three pointers, count, first block, flags per tensor in 4 KB
    assert _lib.lib().halo_sgd_plan_limits(None, None) == E_ARG


def _check_plan(sizes):
    """the plan of `sizes` covers every element of every tensor exactly once: block -> tensor by the kernel's search (the last
    tensor of the launch whose first block is not above the block), block -> elements by the chunk rule of the header"""
    from halo_amd import optim
    chunk, cap = optim.plan_limits()
    launch_of, first_block, launches = optim.plan(sizes)
    live = [i for i, n in enumerate(sizes) if n > 0]
    assert [i for i, l in enumerate(launch_of) if l >= 0] == live
    assert all(first_block[i] == -1 for i, n in enumerate(sizes) if n == 0)
    assert launches == -(-len(live) // cap)
    assert [launch_of[i] for i in live] == [k // cap for k in range(len(live))]           # in list order, cap per launch
    for l in range(launches):
        members = [i for i in live if launch_of[i] == l]
        starts = np.array([first_block[i] for i in members], dtype=np.int64)
        counts = np.array([-(-sizes[i] // chunk) for i in members], dtype=np.int64)
        assert starts[0] == 0 and np.array_equal(starts[1:], np.cumsum(counts)[:-1])     # the grid is filled without a gap
        total = int(starts[-1] + counts[-1])
        assert total < 2 ** 31
        blocks = np.arange(total, dtype=np.int64)
        t = np.searchsorted(starts, blocks, side="right") - 1                              # the kernel's search
        c = blocks - starts[t]
        n = np.array([sizes[i] for i in members], dtype=np.int64)[t]
        lo, hi = c * chunk, np.minimum(n, (c + 1) * chunk)
        assert (lo < hi).all() and (hi <= n).all()                                         # inside its own tensor, never empty
        for j, i in enumerate(members):
            mine = t == j
            assert mine.sum() == counts[j]
            assert lo[mine][0] == 0 and hi[mine][-1] == sizes[i]
            assert np.array_equal(lo[mine][1:], hi[mine][:-1])                             # consecutive, disjoint, complete


def test_plan_covers_every_element_once():
    from halo_amd import optim
    chunk, cap = optim.plan_limits()
    rng = np.random.default_rng(5)
    _check_plan([1])
    _check_plan([0, 0, 5, 0, chunk, 0, chunk + 1, 0])
    _check_plan([0] * (cap + 3) + [7])
    _check_plan([2 ** 31 - 1, 3, 0, 1])                                   # one huge tensor between small ones
    _check_plan([5, 2 ** 31 - 1])
    for count in (cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1):
        _check_plan([5] * count)
        sizes = [int(x) for x in rng.choice([0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7], size=count)]
        _check_plan(sizes)
        _check_plan([0] + sizes + [0])
    assert optim.plan([]) == ([], [], 0) and optim.plan([0, 0]) == ([-1, -1], [-1, -1], 0)


def test_plan_and_step_refuse_what_they_do_not_serve():
    from halo_amd import _lib, optim
    L = _lib.lib()
    with pytest.raises(_lib.HaloUnsupported):
        optim.plan([4, 2 ** 31])
    with pytest.raises(_lib.HaloHipError):
        optim.plan([4, -1])
    size = ctypes.sizeof(_lib.SgdArgs)

    def call(tensors, **kw):
        table = (_lib.SgdTensor * max(1, len(tensors)))(*[_lib.SgdTensor(**t) for t in tensors])
        fields = dict(struct_bytes=size, mode=_lib.SGD_GEOOPT, lr=0.1, momentum=0.9, count=len(tensors), tensors=table)
        fields.update(kw)
        return L.halo_sgd_step(ctypes.byref(_lib.SgdArgs(**fields)), None)
    one = dict(p=16, g=32, buf=48, n=4, dtype=_lib.F32, first=1)          # never dereferenced: every case fails a check before a launch
    assert call([one], struct_bytes=size - 8) == E_ARG
    assert call([one], mode=2) == E_ARG
    assert call([dict(one, n=2 ** 31)]) == E_UNSUPPORTED and b"2^31" in L.halo_last_error()
    assert call([dict(one, n=-1)]) == E_ARG
    assert call([dict(one, dtype=_lib.I32)]) == E_UNSUPPORTED
    assert call([dict(one, g=None)]) == E_ARG
    assert call([dict(one, buf=None)]) == E_ARG                           # momentum > 0 needs the buffer
    assert call([one], nesterov=1, momentum=0.0) == E_ARG
    assert call([one, dict(one, p=None)]) == E_ARG                        # the second tensor's fault, found before the first's launch
    assert call([], count=0) == 0 and call([dict(one, n=0, p=None)]) == 0   # nothing to do: no launch


def _params(n=3):
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(4, 3)) for _ in range(n)]


def test_cpu_parameters_raise():
    from halo_amd import _lib, optim
    for opt in (torch.optim.SGD(_params(), lr=0.1, momentum=0.9), RiemannianSGD(_params(), lr=0.1, momentum=0.9)):
        cls = type(opt)
        with pytest.raises(_lib.HaloHipError, match="no CPU path"):
            optim.fuse_step(opt)
        assert type(opt) is cls                                           # refused before anything changed


class _Ball:
    name = "PoincareBall"


def test_class_recognition():
    from halo_amd import optim
    assert optim.recognise(torch.optim.SGD(_params(), lr=0.1)) == "torch"
    assert optim.recognise(RiemannianSGD(_params(), lr=0.1)) == "geoopt"

    class Derived(RiemannianSGD):                                         # inherits the step: still geoopt's
        pass
    assert optim.recognise(Derived(_params(), lr=0.1)) == "geoopt"

    class OwnStep(torch.optim.SGD):
        def step(self, closure=None):
            return None
    assert optim.recognise(OwnStep(_params(), lr=0.1)) is None
    adam = torch.optim.Adam(_params(), lr=0.1)
    assert optim.recognise(adam) is None
    assert optim.fuse_step(adam) is adam and type(adam) is torch.optim.Adam and "neither" in adam.fallback_reason

    class RiemannianAdam(torch.optim.Optimizer):                          # the name alone is not enough, nor are the keys
        def __init__(self, params):
            super().__init__(params, dict(lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False, stabilize=None))

        def step(self, closure=None):
            return None
    assert optim.recognise(RiemannianAdam(_params())) is None
    assert optim.recognise(object()) is None

    p = _params(1)[0]
    p.manifold = _Ball()                                                  # a look-alike of geoopt's ManifoldParameter on the ball
    ball = RiemannianSGD([p], lr=0.1, momentum=0.9)
    assert optim.recognise(ball) == "geoopt"                              # the class is geoopt's; the parameter is what is not served
    assert "PoincareBall" in optim.fallback_reason(ball)
    assert "PoincareBall" in optim.group_fallback_reason(ball, ball.param_groups[0])


@pytest.fixture
def stubbed(monkeypatch):
    """the device requirement lifted and the kernel call replaced by a recorder: what is left is the host side of the step"""
    from halo_amd import optim
    calls = []
    monkeypatch.setattr(optim, "_require_device", lambda p: None)
    monkeypatch.setattr(optim, "_launch", lambda mode, group, entries: calls.append((mode, group["lr"], [(e[0], e[3]) for e in entries])))
    return calls


def _schedule(opt):
    from torch.optim.lr_scheduler import LinearLR, PolynomialLR, SequentialLR
    return SequentialLR(opt, schedulers=[LinearLR(opt, start_factor=0.01, total_iters=2), PolynomialLR(opt, 8, power=0.9)], milestones=[2])


@pytest.mark.parametrize("kind", ["torch", "geoopt"])
@pytest.mark.parametrize("order", ["scheduler_first", "conversion_first"])
def test_schedulers_see_the_converted_step(stubbed, kind, order):
    from halo_amd import optim
    params = _params()
    make = torch.optim.SGD if kind == "torch" else RiemannianSGD
    opt = make(params, lr=0.1, momentum=0.9, weight_decay=5e-4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if order == "scheduler_first":
            sched = _schedule(opt)
            assert optim.fuse_step(opt) is opt
        else:
            assert optim.fuse_step(opt) is opt
            sched = _schedule(opt)
        assert isinstance(opt, make) and optim.recognise(opt) == kind and opt.fallback_reason is None
        assert optim.fuse_step(opt) is opt                                # idempotent
        seen = []
        for step in range(5):
            for p in params[:2]:
                p.grad = torch.ones_like(p)
            assert opt.step(lambda: 7.0) == 7.0                           # the closure's value comes back
            seen.append(opt.param_groups[0]["lr"])
            sched.step()                                                  # no "before optimizer.step()" warning, none about an overridden step
    assert len(stubbed) == 5 and all(c[0] == kind for c in stubbed)
    assert [c[1] for c in stubbed] == seen and len(set(seen)) == 5        # the learning rate is read from the group at every step
    assert [[f for _, f in c[2]] for c in stubbed] == [[True, True]] + [[False, False]] * 4
    assert all([p for p, _ in c[2]] == params[:2] for c in stubbed)       # the parameter without a gradient is left out
    # the stock state keys, and only for parameters that have stepped
    state = opt.state_dict()["state"]
    assert sorted(state) == [0, 1] and all(sorted(s) == ["momentum_buffer"] for s in state.values())
    if kind == "geoopt":
        assert opt.param_groups[0]["step"] == 5


def test_unserved_groups_run_the_stock_step(stubbed):
    from halo_amd import optim
    params = _params(4)
    opt = torch.optim.SGD([{"params": params[:2]}, {"params": params[2:], "maximize": True}], lr=0.5)
    optim.fuse_step(opt)
    assert opt.fallback_reason == "param group 1: maximize" and opt.group_fallback_reasons == [None, "maximize"]
    before = [p.detach().clone() for p in params]
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    assert len(stubbed) == 1 and [p for p, _ in stubbed[0][2]] == params[:2]
    assert all(torch.equal(p, b) for p, b in zip(params[:2], before[:2]))                 # the stub moved nothing
    assert all(torch.equal(p, b + 0.5) for p, b in zip(params[2:], before[2:]))           # the stock step of group 1 alone: ascent
    assert len(opt.param_groups) == 2
    for key, why in (("lr", "a tensor lr"), ("weight_decay", "a tensor weight_decay")):
        g = dict(opt.param_groups[0])
        g[key] = torch.tensor(0.1)
        assert optim.group_fallback_reason(opt, g) == why
    assert optim.group_fallback_reason(opt, dict(opt.param_groups[0], differentiable=True)) == "differentiable"
    half = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))], lr=0.1)
    assert "float16" in optim.fallback_reason(half)
    strided = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3, 4).t())], lr=0.1)
    assert "non-contiguous parameter" in optim.fallback_reason(strided)
    sparse = torch.optim.SGD(_params(1), lr=0.1)
    sparse.param_groups[0]["params"][0].grad = torch.zeros(4, 3).to_sparse()
    assert "sparse gradient" in optim.fallback_reason(sparse)


def test_hook_converts_what_configure_optimizers_returns(stubbed):
    from halo_amd import hooks, optim

    class Learner:
        def __init__(self):
            self.params = _params()

        def configure_optimizers(self):
            a = RiemannianSGD(self.params[:2], lr=0.1, momentum=0.9)
            b = torch.optim.Adam(self.params[2:], lr=0.1)
            self.made = ([a, b], [_schedule(a)])
            return self.made

    class Hooked(Learner):
        pass

    assert hooks.use_fused_optimizer_step(Hooked) is Hooked and hooks.use_fused_optimizer_step(Hooked) is Hooked
    learner = Hooked()
    optimizers, schedulers = learner.configure_optimizers()
    assert optimizers is learner.made[0] and schedulers is learner.made[1]               # the same objects come back
    assert optim.recognise(optimizers[0]) == "geoopt" and type(optimizers[0]) is not RiemannianSGD and isinstance(optimizers[0], RiemannianSGD)
    assert type(optimizers[1]) is torch.optim.Adam and optimizers[1].fallback_reason
    assert schedulers[0].optimizer is optimizers[0]
    assert type(Learner().configure_optimizers()[0][0]) is RiemannianSGD                  # the unhooked class is as it was
    with pytest.raises(TypeError):
        hooks.use_fused_optimizer_step(object)
