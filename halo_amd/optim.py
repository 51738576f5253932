"""The optimiser step of the training loop in one HIP pass per param group (halo_optim.hip).

The reference's learners (core/train_learners.py:167-208) build two geoopt RiemannianSGD instances when MODEL.HYPER is set and two
torch.optim.SGD instances otherwise.  Every parameter of its models is a plain nn.Parameter, so geoopt's step runs on its default
Euclidean manifold: per tensor a clone (first step), add_, mul_, add_, mul, add, copy_, copy_, in a Python loop.  `fuse_step
(optimizer)` converts a live optimiser of either kind in place: the same object, the same param_groups, the same state keys
(`momentum_buffer`), the same state_dict, and a `step` that hands each group's tensors to halo_sgd_step, which reproduces the bits
of the stock chain (include/halo_hip.h states both chains).  The two kinds differ -- the first step's buffer, the in-place change of
p.grad, one rounding of the update against two -- so each optimiser keeps its own statements.

What is served is decided from the groups and the tensors alone, at every step: a group the kernel does not serve (fallback_reason)
runs the optimiser's own stock step for that group, and an optimiser of another class is returned as it came.  Parameters on the
CPU raise HaloHipError: there is no CPU path.
"""
import ctypes as C
import functools
import weakref

import torch

from . import _lib

_GEOOPT_KEYS = ("lr", "momentum", "dampening", "weight_decay", "nesterov", "stabilize")
_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _step_owner(cls):
    """the class of the MRO whose `step` the optimiser runs"""
    for klass in cls.__mro__:
        if "step" in klass.__dict__:
            return klass
    return None


def recognise(optimizer):
    """"torch" for torch.optim.SGD, "geoopt" for geoopt's RiemannianSGD, None for anything else.  geoopt is recognised without
    importing it: a class named RiemannianSGD in the MRO that provides the step, and its param-group keys.  A subclass that
    overrides `step` is neither."""
    if not isinstance(optimizer, torch.optim.Optimizer):
        return None
    cls = type(optimizer)
    if getattr(cls, "_halo_fused_mode", None) is not None:
        return cls._halo_fused_mode
    owner = _step_owner(cls)
    if owner is torch.optim.SGD:
        return "torch"
    if owner is not None and owner.__name__ == "RiemannianSGD" and not issubclass(cls, torch.optim.SGD):
        if all(all(k in g for k in _GEOOPT_KEYS) for g in optimizer.param_groups):
            return "geoopt"
    return None


def _is_euclidean(p):
    man = getattr(p, "manifold", None)
    return man is None or getattr(man, "name", type(man).__name__) == "Euclidean"


def _require_device(p):
    if not p.is_cuda:
        raise _lib.HaloHipError("halo_amd.optim runs on ROCm devices only (got a %s parameter); there is no CPU path" % p.device)


def _plain_number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def group_fallback_reason(optimizer, group, mode=None):
    """why this param group runs the optimiser's stock step (None: halo_sgd_step serves it).  Looks at the group's options, its
    parameters and the gradients they hold right now."""
    mode = mode or recognise(optimizer)
    if mode is None:
        return "%s is neither torch.optim.SGD nor geoopt's RiemannianSGD" % type(optimizer).__name__
    for key in ("lr", "weight_decay", "momentum", "dampening"):
        if torch.is_tensor(group[key]):
            return "a tensor %s" % key
        if not _plain_number(group[key]):
            return "%s is %r, not a number" % (key, group[key])
    if mode == "torch":
        if group.get("maximize"):
            return "maximize"
        if group.get("differentiable"):
            return "differentiable"
        if group.get("fused"):
            return "fused=True asks for torch's own fused kernel, which rounds differently"
    if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
        return "nesterov without momentum or with dampening"
    device = None
    for p in group["params"]:
        if not _is_euclidean(p):
            return "a parameter on the %s manifold" % getattr(p.manifold, "name", type(p.manifold).__name__)
        _require_device(p)
        if p.dtype not in _DTYPES:
            return "a %s parameter" % p.dtype
        if p.layout != torch.strided or not p.is_contiguous():
            return "a non-contiguous parameter"
        if device is None:
            device = p.device
        elif p.device != device:
            return "parameters on %s and %s" % (device, p.device)
        g = p.grad
        if g is None:
            continue
        if g.is_sparse or g.layout != torch.strided:
            return "a sparse gradient"
        if not g.is_contiguous():
            return "a non-contiguous gradient"
        if g.dtype != p.dtype or g.device != p.device or g.shape != p.shape:
            return "a gradient of another dtype, device or shape than its parameter"
        if g.requires_grad:
            return "a gradient that requires grad"
        st = optimizer.state.get(p)                                # .get: looking must not create the entry the stock step creates
        buf = st.get("momentum_buffer") if st else None
        if buf is not None and (not torch.is_tensor(buf) or buf.dtype != p.dtype or buf.device != p.device or buf.shape != p.shape
                                or not buf.is_contiguous()):
            return "a momentum buffer of another dtype, device, shape or layout than its parameter"
        if mode == "geoopt" and buf is None and group["momentum"] > 0 and st:
            return "a parameter state without its momentum buffer"
    return None


def fallback_reason(optimizer):
    """why fuse_step leaves (part of) this optimiser on its stock step: None when every group is served, else the first unserved
    group's reason.  CPU parameters raise HaloHipError."""
    mode = recognise(optimizer)
    if mode is None:
        return group_fallback_reason(optimizer, None, mode)
    for i, group in enumerate(optimizer.param_groups):
        why = group_fallback_reason(optimizer, group, mode)
        if why is not None:
            return "param group %d: %s" % (i, why)
    return None


def _launch(mode, group, entries):
    """halo_sgd_step on (p, g, buf, first) entries of one device"""
    n = len(entries)
    table = (_lib.SgdTensor * n)()
    for t, (p, g, buf, first) in zip(table, entries):
        t.p, t.g, t.buf = p.data_ptr(), g.data_ptr(), (None if buf is None else buf.data_ptr())
        t.n, t.dtype, t.first = p.numel(), _DTYPES[p.dtype], first
    args = _lib.SgdArgs(struct_bytes=C.sizeof(_lib.SgdArgs), mode=_lib.SGD_GEOOPT if mode == "geoopt" else _lib.SGD_TORCH,
                        nesterov=1 if group["nesterov"] else 0, lr=float(group["lr"]), momentum=float(group["momentum"]),
                        dampening=float(group["dampening"]), weight_decay=float(group["weight_decay"]), count=n, tensors=table)
    _lib.check(_lib.lib().halo_sgd_step(C.byref(args), _lib.stream_ptr(entries[0][0].device)), "halo_sgd_step")


def _fused_group(self, mode, group):
    """one served group: the host side of the stock step (state keys, the group's step count), then one call"""
    state = self.state
    entries = []
    if mode == "geoopt":
        # rsgd.py: `if "step" not in group: group["step"] = 0`, `group["step"] += 1`; `state = self.state[point]` for every
        # parameter with a gradient (an empty state without momentum), the buffer made on the first use with momentum > 0
        if "step" not in group:
            group["step"] = 0
        group["step"] += 1
        use_momentum = group["momentum"] > 0
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            st = state[p]
            first = len(st) == 0
            buf = None
            if use_momentum:
                if first:
                    st["momentum_buffer"] = torch.empty_like(g)
                buf = st["momentum_buffer"]
            entries.append((p, g, buf, first))
        # `stabilize` has nothing to do for plain parameters (stabilize_group skips them)
    else:
        # sgd.py: `state = self.state[p]` only with momentum != 0; `state["momentum_buffer"]` is the clone of the first gradient
        use_momentum = group["momentum"] != 0
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            buf, first = None, False
            if use_momentum:
                st = state[p]
                buf = st.get("momentum_buffer")
                first = buf is None
                if first:
                    buf = st["momentum_buffer"] = torch.empty_like(g)
            entries.append((p, g, buf, first))
    if entries:
        _launch(mode, group, entries)


def _fused_step(self, closure=None):
    mode = type(self)._halo_fused_mode
    loss = None
    if closure is not None:
        if mode == "torch":
            with torch.enable_grad():
                loss = closure()
        else:
            loss = closure()
    reasons = []
    for group in self.param_groups:
        why = group_fallback_reason(self, group, mode)
        reasons.append(why)
        if why is None:
            with torch.no_grad():
                _fused_group(self, mode, group)
        else:
            _stock_group(self, group)
    self.group_fallback_reasons = reasons
    self.fallback_reason = next(("param group %d: %s" % (i, w) for i, w in enumerate(reasons) if w is not None), None)
    return loss


def _stock_group(self, group):
    """the optimiser's own step on this group alone"""
    stock = type(self)._halo_stock_step
    groups = self.param_groups
    self.param_groups = [group]
    try:
        stock(self)                                                # sets the grad mode it wants itself
    finally:
        self.param_groups = groups


_FUSED_CLASSES = {}


def _fused_class(cls, mode):
    fused = _FUSED_CLASSES.get(cls)
    if fused is None:
        stock = cls.step
        stock = getattr(stock, "__wrapped__", stock) if getattr(stock, "hooked", False) else stock      # under Optimizer.profile_hook_step
        step = torch.optim.Optimizer.profile_hook_step(_fused_step)                                   # step pre / post hooks, profiler name
        step.hooked = True
        fused = type(cls.__name__, (cls,), {"step": step, "_halo_fused_mode": mode, "_halo_stock_step": staticmethod(stock),
                                            "__module__": cls.__module__, "__doc__": cls.__doc__})
        _FUSED_CLASSES[cls] = fused
    return fused


def _rebind_scheduler_wrapper(optimizer):
    """An LR scheduler built before the conversion left `optimizer.step` on the INSTANCE: a wrapper that notes the call for the
    scheduler's order warning and then runs the step function it captured, the stock one.  Put the same wrapper around the class's
    step as it is now, so the note is still taken and the fused step runs."""
    inst = optimizer.__dict__.get("step")
    if inst is None or not getattr(inst, "_wrapped_by_lr_sched", False):
        return
    func = type(optimizer).step
    ref = weakref.ref(optimizer)

    @functools.wraps(func)
    def wrapper(*args, **kwargs):
        opt = ref()
        opt._opt_called = True
        return func.__get__(opt, type(opt))(*args, **kwargs)

    wrapper._wrapped_by_lr_sched = True
    optimizer.step = wrapper


def fuse_step(optimizer):
    """Convert a live torch.optim.SGD or geoopt RiemannianSGD in place so that `step` runs halo_sgd_step; returns the same object.
    param_groups, state (`momentum_buffer`), state_dict() / load_state_dict() and step's `closure` stay as they are, schedulers
    built before or after keep working, and learning rates are read from param_groups at every step.  `optimizer.fallback_reason`
    says why (part of) it stays on the stock step (None: every group is served); it is refreshed by every step.  An optimiser of
    another class is returned unconverted with the reason set.  Idempotent."""
    mode = recognise(optimizer)
    if mode is None:
        optimizer.fallback_reason = group_fallback_reason(optimizer, None, None)
        return optimizer
    why = fallback_reason(optimizer)                               # raises HaloHipError for CPU parameters, before anything changes
    if getattr(type(optimizer), "_halo_fused_mode", None) is None:
        optimizer.__class__ = _fused_class(type(optimizer), mode)
        _rebind_scheduler_wrapper(optimizer)
    optimizer.fallback_reason = why
    optimizer.group_fallback_reasons = [group_fallback_reason(optimizer, g, mode) for g in optimizer.param_groups]
    return optimizer


def plan_limits():
    """(elements per workgroup chunk, tensors per launch) of halo_sgd_step: a pure host query"""
    chunk, cap = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().halo_sgd_plan_limits(C.byref(chunk), C.byref(cap)), "halo_sgd_plan_limits")
    return chunk.value, cap.value


def plan(sizes):
    """halo_sgd_plan on a list of element counts: (launch of each tensor or -1, its first block there, the number of launches)"""
    n = len(sizes)
    arr = (C.c_int64 * max(n, 1))(*sizes)
    launch_of, first_block, launches = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))(), C.c_int64()
    _lib.check(_lib.lib().halo_sgd_plan(arr, n, launch_of, first_block, C.byref(launches)), "halo_sgd_plan")
    return list(launch_of[:n]), list(first_block[:n]), launches.value


__all__ = ["fuse_step", "fallback_reason", "group_fallback_reason", "recognise", "plan_limits", "plan"]
