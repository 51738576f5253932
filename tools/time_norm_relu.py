"""Timing aid: halo_amd.norm.norm_relu (halo_norm.hip) against the stock chain it replaces -- FrozenBatchNorm2d (x * scale + bias as
torch statements, scale and bias recomputed per call), the in-place `out += identity` and ReLU(inplace=True) -- under autograd, in the
same process on the same device, float32:

  operator   the backbone's activation shapes at the 640 x 1280 training crop (batch 2: forward and forward + backward) and at the
             1024 x 2048 acquisition geometry (batch 1: forward), without a residual (bn1 / bn2 + ReLU), with a plain residual
             (bn3, += identity, ReLU) and with the downsample norm folded in (first block of a layer);
  backbone   a randomly initialised ResNet-101-shaped stand-in written for this tool (7 x 7 stem inside a sequential container,
             3 / 4 / 23 / 3 bottlenecks, layers 3 and 4 dilated: output stride 8; no pretrained weights), unhooked against hooked
             with halo_amd.hooks.use_fused_frozen_norm + fuse_norm_relu_pairs: forward (no_grad) and forward + backward (gradients
             for every conv weight) at 2 x 3 x 640 x 1280, forward at 1 x 3 x 1024 x 2048.

HIP events around n calls after warm-up calls of every timed closure; `repeats` windows per figure, printed as best / median /
worst.  The two sides alternate window by window.  Also reported: the fused forward's achieved bytes/s against its algorithmic
traffic (one read per operand, one write) and torch.cuda.max_memory_allocated over one forward + backward above what is held
before it.  One process; every step (a shape, a model pass) runs under its own alarm, whose expiry ends the process, and the first
failure ends the run; the lines so far are in --out.

    python tools/time_norm_relu.py [--out profiles/r09_time_norm_relu.txt] [--n 10] [--repeats 7] [--skip-backbone]
"""
import argparse
import copy
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd import norm  # noqa: E402
from halo_amd.hooks import fuse_norm_relu_pairs, use_fused_frozen_norm  # noqa: E402
from halo_amd.norm import fallback_reason, norm_relu  # noqa: E402

DEFAULT_RULE = dict(norm.AUTOGRAD_MIN_ELEMENTS)      # the envelope's size rule under autograd; the operator part times the kernels at
SERVE_ALL = {"plain": 0, "affine": 0}                # every size and says which shapes the rule leaves to the stock statements

# (C, stride of the plane against the input) of the backbone's norms: stem, then (width, 4 * width) of layers 1-4 at output stride 8
PLANES = [(64, 2), (64, 4), (256, 4), (128, 8), (512, 8), (256, 8), (1024, 8), (512, 8), (2048, 8)]
RESIDUAL = {(256, 4), (512, 8), (1024, 8), (2048, 8)}            # the block outputs: the shapes that also run with a residual
GEOMETRIES = [("train B=2", 2, 640, 1280, True), ("acquire B=1", 1, 1024, 2048, False)]


class FrozenBatchNorm2d(nn.Module):
    """the frozen norm of the backbone and the heads: four buffers, y = x * scale + bias"""

    def __init__(self, n):
        super().__init__()
        for name, v in (("weight", torch.ones(n)), ("bias", torch.zeros(n)), ("running_mean", torch.zeros(n)), ("running_var", torch.ones(n))):
            self.register_buffer(name, v)

    def forward(self, x):
        scale = self.weight * self.running_var.rsqrt()
        bias = self.bias - self.running_mean * scale
        scale = scale.reshape(1, -1, 1, 1)
        bias = bias.reshape(1, -1, 1, 1)
        return x * scale + bias


class Bottleneck(nn.Module):
    def __init__(self, cin, width, stride=1, dilation=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = FrozenBatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, dilation, dilation, bias=False)
        self.bn2 = FrozenBatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, 4 * width, 1, bias=False)
        self.bn3 = FrozenBatchNorm2d(4 * width)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def resnet101_shaped():
    layers = [nn.Conv2d(3, 64, 7, 2, 3, bias=False), FrozenBatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)]
    cin = 64
    for width, blocks, stride, dilation in ((64, 3, 1, 1), (128, 4, 2, 1), (256, 23, 1, 2), (512, 3, 1, 4)):
        for k in range(blocks):
            down = None
            if k == 0:
                down = nn.Sequential(nn.Conv2d(cin, 4 * width, 1, stride, bias=False), FrozenBatchNorm2d(4 * width))
            # the first block of a dilated layer keeps the previous layer's dilation, as torchvision's replace_stride_with_dilation does
            layers.append(Bottleneck(cin, width, stride if k == 0 else 1, max(dilation // 2, 1) if k == 0 else dilation, down))
            cin = 4 * width
    return nn.Sequential(*layers)


def randomize(module, gen, dev):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, FrozenBatchNorm2d):
                n = m.weight.numel()
                m.weight.copy_(0.25 + 1.5 * torch.rand(n, device=dev, generator=gen))
                m.bias.copy_(0.4 * torch.randn(n, device=dev, generator=gen))
                m.running_mean.copy_(0.5 * torch.randn(n, device=dev, generator=gen))
                m.running_var.copy_(0.3 + 1.5 * torch.rand(n, device=dev, generator=gen))


def stock_chain(x, bn, residual=None, residual_bn=None, act=nn.ReLU(inplace=True)):
    out = bn(x)
    if residual is not None:
        out += residual if residual_bn is None else residual_bn(residual)
    return act(out)


def windows(fns, n, repeats, warm=3):
    """per closure the sorted per-call times (ms) of `repeats` windows of n calls; the closures alternate window by window"""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / n)
    return [sorted(t) for t in out]


def fmt(t):
    return "%.4f / %.4f / %.4f" % (t[0], t[len(t) // 2], t[-1])


def med(t):
    return t[len(t) // 2]


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def compare(say, label, f, s, note="   FUSED LOSES"):
    say("    %-8s fused %s   stock %s   stock/fused (medians) x%.2f%s" % (label, fmt(f), fmt(s), med(s) / med(f),
                                                                           "" if med(f) <= med(s) else note))


def time_operator(say, dev, args, geometry, B, ih, iw, train, C, stride, variant):
    gen = torch.Generator(device=dev).manual_seed(0)
    H, W = ih // stride, iw // stride
    x = torch.randn((B, C, H, W), device=dev, generator=gen).requires_grad_(train)
    r = torch.randn((B, C, H, W), device=dev, generator=gen).requires_grad_(train) if variant != "none" else None
    bn, rbn = FrozenBatchNorm2d(C).to(dev), FrozenBatchNorm2d(C).to(dev) if variant == "affine" else None
    randomize(bn, gen, dev)
    if rbn is not None:
        randomize(rbn, gen, dev)
    norm.AUTOGRAD_MIN_ELEMENTS = DEFAULT_RULE
    excluded = fallback_reason(x, bn, r, rbn) is not None            # by the size rule: everything else is inside the envelope
    norm.AUTOGRAD_MIN_ELEMENTS = SERVE_ALL
    assert fallback_reason(x, bn, r, rbn) is None, fallback_reason(x, bn, r, rbn)
    g = torch.randn((B, C, H, W), device=dev, generator=gen) if train else None
    leaves = [x] if r is None else [x, r]
    sides = {}
    for tag, op in (("fused", norm_relu), ("stock", stock_chain)):
        def fwd(op=op):
            with torch.no_grad():
                op(x, bn, r, rbn)

        def both(op=op):
            torch.autograd.grad(op(x, bn, r, rbn), leaves, g)
        sides[tag] = dict(fwd=fwd, both=both)
    kinds = ("fwd", "both") if train else ("fwd",)
    order = [(t, k) for k in kinds for t in ("fused", "stock")]
    times = dict(zip(order, windows([sides[t][k] for t, k in order], args.n, args.repeats)))
    nbytes = x.numel() * 4
    units = 2 if r is None else 3                      # reads of x (and r), one write of y
    say("%-11s %-7s %s  (x: %.0f MB)" % (geometry, variant, "x".join(map(str, (B, C, H, W))), nbytes / 1e6))
    compare(say, "forward", times[("fused", "fwd")], times[("stock", "fwd")])
    if train:
        compare(say, "fwd+bwd", times[("fused", "both")], times[("stock", "both")],
                "   fused loses: left to the stock statements under autograd" if excluded else "   FUSED LOSES")
        if excluded:
            say("    under autograd the envelope leaves this shape to the stock statements (halo_amd.norm.AUTOGRAD_MIN_ELEMENTS)")
    say("    fused forward: %.2f TB/s of its algorithmic traffic (%d x %.0f MB)" % (units * nbytes / (med(times[("fused", "fwd")]) * 1e-3) / 1e12,
                                                                                 units, nbytes / 1e6))
    with torch.no_grad():
        same = torch.equal(norm_relu(x, bn, r, rbn), stock_chain(x, bn, r, rbn))
    line = "    y torch.equal to the stock chain: %s" % same
    if train:
        line += "; peak memory above the operands over one fwd+bwd: fused %.1f MiB, stock %.1f MiB" % (peak_mb(sides["fused"]["both"]),
                                                                                                      peak_mb(sides["stock"]["both"]))
    say(line)
    if not same:
        raise SystemExit("the fused forward differs from the stock chain")
    return all(med(times[("fused", k)]) <= med(times[("stock", k)]) for k in kinds if not (excluded and k == "both"))


def time_backbone(say, dev, args):
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    plain = resnet101_shaped().to(dev)
    randomize(plain, gen, dev)
    hooked = copy.deepcopy(plain)
    Hooked = use_fused_frozen_norm(type("Bottleneck", (Bottleneck,), {}))
    blocks = 0
    for m in hooked.modules():
        if type(m) is Bottleneck:
            m.__class__ = Hooked
            blocks += 1
    pairs = fuse_norm_relu_pairs(hooked)
    norms = sum(isinstance(m, FrozenBatchNorm2d) for m in plain.modules())
    say("ResNet-101-shaped stand-in, random weights: %d frozen norms, %d bottlenecks hooked, %d (norm, ReLU) pair fused" % (norms, blocks, pairs))
    n, rep = max(args.n // 4, 2), args.repeats
    for label, B, ih, iw, train in (("train 2x3x640x1280", 2, 640, 1280, True), ("acquire 1x3x1024x2048", 1, 1024, 2048, False)):
        signal.alarm(args.step_seconds * 8)
        x = torch.randn((B, 3, ih, iw), device=dev, generator=gen)
        sides = {}
        for tag, model in (("fused", hooked), ("stock", plain)):
            params = [p for p in model.parameters()]

            def fwd(model=model):
                with torch.no_grad():
                    model(x)

            def both(model=model, params=params):
                out = model(x)
                torch.autograd.grad(out, params, g)
            sides[tag] = dict(fwd=fwd, both=both)
        with torch.no_grad():
            y_s, y_s2, y_f = plain(x), plain(x), hooked(x)
        spread, diff = float((y_s - y_s2).abs().max()), float((y_s - y_f).abs().max())
        g = torch.randn(y_s.shape, device=dev, generator=gen) if train else None
        del y_s, y_s2, y_f
        say("backbone %s: largest output difference unhooked/unhooked %.3g, hooked/unhooked %.3g (the convolutions are the library's)"
            % (label, spread, diff))
        kinds = ("fwd", "both") if train else ("fwd",)
        for rule_name, rule in (("the envelope's size rule", DEFAULT_RULE), ("every size served", SERVE_ALL)):
            if not train and rule is SERVE_ALL:
                continue                                   # without a gradient the rule excludes nothing
            norm.AUTOGRAD_MIN_ELEMENTS = rule
            order = [(t, k) for k in kinds for t in ("fused", "stock")]
            times = dict(zip(order, windows([sides[t][k] for t, k in order], n, rep, warm=2)))
            say("  %s:" % rule_name)
            compare(say, "forward", times[("fused", "fwd")], times[("stock", "fwd")])
            if train:
                compare(say, "fwd+bwd", times[("fused", "both")], times[("stock", "both")])
                say("    peak memory above the model and the input over one fwd+bwd: hooked %.0f MiB, unhooked %.0f MiB"
                    % (peak_mb(sides["fused"]["both"]), peak_mb(sides["stock"]["both"])))
        norm.AUTOGRAD_MIN_ELEMENTS = DEFAULT_RULE
        del sides, times, x, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file, line by line")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-seconds", type=int, default=60, help="alarm per operator shape (eight times that per backbone geometry)")
    ap.add_argument("--skip-backbone", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_norm_relu.py needs a ROCm device")
    dev = torch.device("cuda:0")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")

    def say(s):
        print(s, flush=True)
        if out is not None:
            out.write(s + "\n")
            out.flush()

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    losers = []
    for geometry, B, ih, iw, train in GEOMETRIES:
        seen = set()
        for C, stride in PLANES:
            for variant in ("none", "plain", "affine"):
                if (C, stride, variant) in seen or (variant != "none" and (C, stride) not in RESIDUAL):
                    continue
                seen.add((C, stride, variant))
                signal.alarm(args.step_seconds)                 # no handler: an overrun ends the process
                if not time_operator(say, dev, args, geometry, B, ih, iw, train, C, stride, variant):
                    losers.append((geometry, C, stride, variant))
                signal.alarm(0)
                torch.cuda.empty_cache()
    say("served operator shapes at which the fused side's median is above the stock chain's: %s" % (losers or "none"))
    if not args.skip_backbone:
        time_backbone(say, dev, args)
        signal.alarm(0)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
