"""Timing aid: the optimiser step of the training loop, halo_amd.optim.fuse_step against the stock steps, in one process on the same
gradients.  The parameter set is a stand-in with the reference's shapes (nothing of its code runs here):

  backbone  the 104 convolution weights of a ResNet-101 (bottleneck blocks 3 / 4 / 23 / 3; its norms are frozen buffers);
  head      the tensors of the DeepLab-v3+ hyperbolic head with HFR (core/models/classifier.py:382-494): ASPP branches, bottleneck,
            shortcut, decoder, their norms' weights and biases, conv_reduce, the weighted-normalisation MLP and HyperMLR's two
            float64 (19, 64) tensors.

Two optimisers as the learner builds them (core/train_learners.py:174-177): backbone at the base learning rate, head at ten times
it, momentum 0.9, weight decay 5e-4.  Sides:

  restated      geoopt's RiemannianSGD.step as restated in tests/optim_ref.py: what a MODEL.HYPER run steps with without this package;
  sgd           torch.optim.SGD as constructed by default (its foreach form);
  sgd_fused     torch.optim.SGD(fused=True) where this torch constructs it: a yardstick, it rounds differently from both stock chains;
  halo_geoopt   fuse_step on the restated optimiser;
  halo_torch    fuse_step on torch.optim.SGD.

Every step draws one set of random gradients and hands each side its own copy (new tensors, as a backward leaves them), outside the
timed window; the device is idle when a window opens.  Per side and step: the device time between two HIP events around the two
step() calls and the host wall time of those calls (no synchronise inside).  The sides alternate step by step; medians, best and
worst over the steps after warm-up.  At the end the fused sides' parameters must equal their stock sides' bit for bit.  One run is
one process; the speed statement asks for two (run the tool twice, the second time with --append).

    python tools/time_optimizer_step.py [--out profiles/r28_time_optimizer_step.txt] [--append] [--steps 30] [--warmup 5]
"""
import argparse
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from halo_amd import optim  # noqa: E402
from optim_ref import RiemannianSGD  # noqa: E402

F32, F64 = torch.float32, torch.float64


def resnet101_conv_shapes():
    shapes = [(64, 3, 7, 7)]
    inplanes = 64
    for planes, blocks in ((64, 3), (128, 4), (256, 23), (512, 3)):
        for b in range(blocks):
            shapes += [(planes, inplanes, 1, 1), (planes, planes, 3, 3), (planes * 4, planes, 1, 1)]
            if b == 0:
                shapes.append((planes * 4, inplanes, 1, 1))          # the downsample convolution
            inplanes = planes * 4
    assert len(shapes) == 104
    return [(s, F32) for s in shapes]


def v3plus_hyper_head_shapes(inplanes=2048, out=512, reduced=64, classes=19):
    def norm(c):
        return [((c,), F32), ((c,), F32)]

    def separable(cin, cout):
        return [((cin, 1, 3, 3), F32)] + norm(cin) + [((cout, cin, 1, 1), F32)] + norm(cout)
    shapes = [((out, inplanes, 1, 1), F32)] + norm(out)                       # the 1 x 1 branch
    for _ in range(3):
        shapes += separable(inplanes, out)                                      # the dilated branches
    shapes += [((out, inplanes, 1, 1), F32)] + norm(out)                      # global branch
    shapes += [((out, out * 5, 3, 3), F32)] + norm(out)                       # bottleneck
    shapes += [((48, 256, 1, 1), F32)] + norm(48)                             # shortcut
    shapes += separable(560, 512) + separable(512, 512)                        # decoder
    shapes += [((reduced, 512, 1, 1), F32), ((reduced,), F32)]                # conv_reduce
    shapes += [((reduced, reduced), F32), ((reduced,), F32)] + norm(reduced) + [((reduced, reduced), F32), ((reduced,), F32)]   # wn_mlp
    shapes += [((classes, reduced), F64), ((classes, reduced), F64)]          # HyperMLR.P_MLR, A_MLR
    return shapes


class Side:
    def __init__(self, name, make, init, dev):
        self.name = name
        self.params = [[torch.nn.Parameter(t.clone()) for t in part] for part in init]
        self.opts = make(self.params)
        self.device_ms, self.host_ms = [], []
        self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def give(self, grads):
        for part, gpart in zip(self.params, grads):
            for p, g in zip(part, gpart):
                p.grad = g.clone()

    def step(self, keep):
        torch.cuda.synchronize()
        self.ev[0].record()
        t0 = time.perf_counter()
        for o in self.opts:
            o.step()
        t1 = time.perf_counter()
        self.ev[1].record()
        torch.cuda.synchronize()
        if keep:
            self.device_ms.append(self.ev[0].elapsed_time(self.ev[1]))
            self.host_ms.append((t1 - t0) * 1e3)


def fmt(xs):
    return "%7.3f / %7.3f / %7.3f" % (min(xs), statistics.median(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file, line by line")
    ap.add_argument("--append", action="store_true", help="add to --out (the second process of a pair)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=int, default=240, help="alarm for the whole run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_optimizer_step.py needs a ROCm device")
    signal.alarm(args.seconds)                                     # no handler: an overrun ends the process
    dev = torch.device("cuda:0")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a" if args.append else "w")

    def say(s):
        print(s, flush=True)
        if out is not None:
            out.write(s + "\n")
            out.flush()

    gen = torch.Generator(device=dev).manual_seed(0)
    parts = [resnet101_conv_shapes(), v3plus_hyper_head_shapes()]
    init = [[torch.randn(s, device=dev, dtype=d, generator=gen) * 0.05 for s, d in part] for part in parts]
    elements = [sum(t.numel() for t in part) for part in init]
    nbytes = sum(t.numel() * t.element_size() for part in init for t in part)
    hyper = dict(momentum=0.9, weight_decay=5e-4)
    lrs = (2.5e-4, 2.5e-3)

    def stock(cls, **kw):
        return lambda params: [cls(part, lr=lr, **hyper, **kw) for part, lr in zip(params, lrs)]

    def fused(cls):
        return lambda params: [optim.fuse_step(cls(part, lr=lr, **hyper)) for part, lr in zip(params, lrs)]
    makers = [("restated", stock(RiemannianSGD)), ("sgd", stock(torch.optim.SGD)), ("sgd_fused", stock(torch.optim.SGD, fused=True)),
              ("halo_geoopt", fused(RiemannianSGD)), ("halo_torch", fused(torch.optim.SGD))]
    sides, missing = [], []
    for name, make in makers:
        try:
            sides.append(Side(name, make, init, dev))
        except Exception as exc:                                   # fused=True where this torch does not construct it
            if name != "sgd_fused":
                raise
            missing.append("%s: not constructed by this torch (%s)" % (name, str(exc).splitlines()[0]))
    for s in sides:
        if s.name.startswith("halo"):
            assert all(o.fallback_reason is None for o in s.opts), [o.fallback_reason for o in s.opts]

    say("process %d on %s, torch %s" % (os.getpid(), torch.cuda.get_device_name(0), torch.__version__))
    say("stand-in parameter set: backbone %d tensors / %.1f M elements, head %d tensors / %.1f M elements (2 of them float64), %.1f MB"
        % (len(init[0]), elements[0] / 1e6, len(init[1]), elements[1] / 1e6, nbytes / 1e6))
    chunk, cap = optim.plan_limits()
    launches = [optim.plan([t.numel() for t in part])[2] for part in init]
    say("fused step: %d + %d launches per step (chunk %d elements, %d tensors per launch); algorithmic traffic with momentum: geoopt "
        "mode 3 reads + 3 writes = %.1f MB, torch mode 3 reads + 2 writes = %.1f MB per step" % (launches[0], launches[1], chunk, cap, 6 * nbytes / 1e6, 5 * nbytes / 1e6))
    for line in missing:
        say(line)
    say("per step (both optimisers), ms over %d steps after %d warm-up steps: best / median / worst" % (args.steps, args.warmup))

    for step in range(args.warmup + args.steps):
        grads = [[torch.randn(t.shape, device=dev, dtype=t.dtype, generator=gen) * 0.01 for t in part] for part in init]
        for s in sides:
            s.give(grads)
        del grads
        order = sides[step % len(sides):] + sides[:step % len(sides)]      # the sides alternate, and so does who goes first
        for s in order:
            s.step(keep=step >= args.warmup)

    by = {s.name: s for s in sides}
    for s in sides:
        say("  %-12s device %s    host %s" % (s.name, fmt(s.device_ms), fmt(s.host_ms)))
    med = statistics.median
    for a, b in (("halo_geoopt", "restated"), ("halo_torch", "sgd"), ("halo_torch", "sgd_fused"), ("halo_geoopt", "sgd_fused")):
        if a in by and b in by:
            say("  %s against %s (medians): device x%.2f, host x%.2f" % (a, b, med(by[b].device_ms) / med(by[a].device_ms), med(by[b].host_ms) / med(by[a].host_ms)))
    g = by["halo_geoopt"]
    say("  halo_geoopt: %.2f TB/s of its algorithmic traffic over the median device time" % (6 * nbytes / (med(g.device_ms) * 1e-3) / 1e12))
    same = {}
    for a, b in (("halo_geoopt", "restated"), ("halo_torch", "sgd")):
        same[a] = all(torch.equal(p.detach().view(torch.int32 if p.dtype == F32 else torch.int64), q.detach().view(torch.int32 if q.dtype == F32 else torch.int64))
                      for pa, pb in zip(by[a].params, by[b].params) for p, q in zip(pa, pb))
        say("  %s equals %s bit for bit after %d steps: %s" % (a, b, args.warmup + args.steps, same[a]))
    wins = med(g.device_ms) < med(by["restated"].device_ms) and med(g.host_ms) < med(by["restated"].host_ms)
    say("  fused geoopt-mode step beats the restated chain on both clocks: %s" % wins)
    if out is not None:
        out.close()
    if not all(same.values()):
        raise SystemExit("a fused side differs from its stock side")
    if not wins:
        raise SystemExit("the fused geoopt-mode step does not beat the restated chain")


if __name__ == "__main__":
    main()
