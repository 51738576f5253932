"""geoopt's RiemannianSGD step for plain parameters, restated in stock torch statements, and a stand-in optimiser class built on it.

geoopt is not installable where this suite runs ("geoopt is not available"); this file does for its optimiser what
tests/golden/_shims/geoopt does for its manifold math: the statements of geoopt/optim/rsgd.py (RiemannianSGD.step, geoopt 0.5) and
of geoopt/optim/mixin.py (OptimMixin), restated from knowledge of that source, each next to the source line it restates (quoted
after `# rsgd:` / `# mixin:`), specialised to what every parameter of the reference's models is: a plain nn.Parameter, which the
step puts on `self._default_manifold = Euclidean()`, where (geoopt/manifolds/euclidean.py)

    egrad2rgrad(x, u) = u          retr(x, u) = x + u          transp(x, y, v) = v
    retr_transp(x, u, v) = (retr(x, u), transp(x, retr(x, u), v)) = (x + u, v)            (geoopt/manifolds/base.py)

The statements run as ATen kernels on whatever device the tensors live on; halo_amd.optim's kernel is compared with them bit for
bit on the same device (tests/test_gpu_optim.py).  Must be re-verified against the wheel the moment one is reachable.
"""
import torch


def rsgd_point_step(point, state, learning_rate, momentum, dampening, weight_decay, nesterov):
    """the body of RiemannianSGD.step's loop for one plain parameter `point` with a dense gradient; `state` is self.state[point]"""
    grad = point.grad                                              # rsgd: grad = point.grad
    if len(state) == 0:                                            # rsgd: if len(state) == 0:
        if momentum > 0:                                           # rsgd:     if momentum > 0:
            state["momentum_buffer"] = grad.clone()                # rsgd:         state["momentum_buffer"] = grad.clone()
    # rsgd: manifold = self._default_manifold                      (point is no ManifoldParameter / ManifoldTensor)
    grad.add_(point, alpha=weight_decay)                           # rsgd: grad.add_(point, alpha=weight_decay)
    # rsgd: grad = manifold.egrad2rgrad(point, grad)               the identity
    if momentum > 0:                                               # rsgd: if momentum > 0:
        momentum_buffer = state["momentum_buffer"]                 # rsgd:     momentum_buffer = state["momentum_buffer"]
        momentum_buffer.mul_(momentum).add_(grad, alpha=1 - dampening)      # rsgd:     momentum_buffer.mul_(momentum).add_(grad, alpha=1 - dampening)
        if nesterov:                                               # rsgd:     if nesterov:
            grad = grad.add_(momentum_buffer, alpha=momentum)      # rsgd:         grad = grad.add_(momentum_buffer, alpha=momentum)
        else:                                                      # rsgd:     else:
            grad = momentum_buffer                                 # rsgd:         grad = momentum_buffer
        # rsgd:     new_point, new_momentum_buffer = manifold.retr_transp(point, -learning_rate * grad, momentum_buffer)
        new_point, new_momentum_buffer = point + (-learning_rate * grad), momentum_buffer
        momentum_buffer.copy_(new_momentum_buffer)                 # rsgd:     momentum_buffer.copy_(new_momentum_buffer)
        point.copy_(new_point)                                     # rsgd:     point.copy_(new_point)
    else:                                                          # rsgd: else:
        new_point = point + (-learning_rate * grad)                # rsgd:     new_point = manifold.retr(point, -learning_rate * grad)
        point.copy_(new_point)                                     # rsgd:     point.copy_(new_point)


class RiemannianSGD(torch.optim.Optimizer):
    """Stand-in for geoopt.optim.RiemannianSGD (class RiemannianSGD(OptimMixin, torch.optim.Optimizer)) for plain parameters:
    the same constructor, param-group keys, state keys and step statements.  A parameter that carries a non-Euclidean `manifold`
    is refused: the stand-in has no manifold code."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, stabilize=None):
        if lr < 0.0:                                               # rsgd: if lr < 0.0: raise ValueError(...)
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._stabilize = stabilize                                # mixin: self._stabilize = stabilize
        super().__init__(params, defaults)                         # mixin: super().__init__(*args, **kwargs)

    def add_param_group(self, param_group):
        param_group.setdefault("stabilize", self._stabilize)       # mixin: param_group.setdefault("stabilize", self._stabilize)
        return super().add_param_group(param_group)

    def step(self, closure=None):
        loss = None
        if closure is not None:                                    # rsgd: if closure is not None: loss = closure()
            loss = closure()
        with torch.no_grad():                                      # rsgd: with torch.no_grad():
            for group in self.param_groups:                        # rsgd: for group in self.param_groups:
                if "step" not in group:                            # rsgd:     if "step" not in group: group["step"] = 0
                    group["step"] = 0
                weight_decay = group["weight_decay"]
                momentum = group["momentum"]
                dampening = group["dampening"]
                nesterov = group["nesterov"]
                learning_rate = group["lr"]
                group["step"] += 1                                 # rsgd:     group["step"] += 1
                for point in group["params"]:                      # rsgd:     for point in group["params"]:
                    grad = point.grad
                    if grad is None:                               # rsgd:         if grad is None: continue
                        continue
                    if grad.is_sparse:                             # rsgd:         if grad.is_sparse: raise RuntimeError(...)
                        raise RuntimeError("RiemannianSGD does not support sparse gradients, use SparseRiemannianSGD instead")
                    state = self.state[point]                      # rsgd:         state = self.state[point]
                    manifold = getattr(point, "manifold", None)
                    if manifold is not None and getattr(manifold, "name", "") != "Euclidean":
                        raise NotImplementedError("the stand-in steps plain parameters only")
                    rsgd_point_step(point, state, learning_rate, momentum, dampening, weight_decay, nesterov)
                # rsgd:     if group["stabilize"] is not None and group["step"] % group["stabilize"] == 0: self.stabilize_group(group)
                # mixin / rsgd: stabilize_group skips every p that is no ManifoldParameter / ManifoldTensor: nothing to do
        return loss
