"""Timing aid: halo_amd.hooks.fuse_residual_chains (norm_relu_fork, halo_fork_affine_relu_bwd) against the configuration it is added
to, under autograd, in one process on one device, float32:

  parent     use_fused_frozen_norm + fuse_norm_relu_pairs: a block output that the next block reads twice gets its two gradients
             added by the autograd engine's own kernel before the tail's backward reads the sum;
  chained    that plus fuse_residual_chains: the tail's backward takes both gradients in its one pass.

  tails      a chain of three identical bottlenecks without a downsample (width C / 4, the dilation of the backbone's layer of that
             width), forward + backward with gradients for the input and every conv weight, at the four block-output shapes of
             the 640 x 1280 training crop, batch 2.  Two of the chain's three outputs are forked, and served with
             FORK_AUTOGRAD_MIN_ELEMENTS = 0.  At 2 x 512 x 80 x 160 the envelope's size rule leaves the tails to the stock
             statements in the parent configuration and, chained, the last of the three.
  backbone   the ResNet-101-shaped stand-in of tools/time_norm_relu.py with its blocks regrouped into four nn.Sequential layers
             (3 / 4 / 23 / 3, as the reference's ResNet holds them), at 2 x 3 x 640 x 1280: forward + backward, parent and chained,
             and the stock model for reference.

HIP events around n calls after three warm-up calls of every closure; the configurations alternate window by window (parent,
chained, parent, chained, ...), `repeats` windows each, printed as best / median / worst.  The parent's own spread is the distance
between the medians of its even and of its odd windows; a shape "wins" when the chained median is below the parent's by more
than that.  Also reported: torch.cuda.max_memory_allocated over one forward + backward above what is held before it.  Every step
runs under its own alarm, whose expiry ends the process; the lines so far are in --out.  Run it twice; the rule asks for a win in
both runs.

    python tools/time_residual_chain.py [--out profiles/r18_time_residual_chain.txt] [--n 10] [--repeats 8] [--skip-backbone]
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
from halo_amd.hooks import fuse_norm_relu_pairs, fuse_residual_chains, use_fused_frozen_norm  # noqa: E402
from tools.time_norm_relu import Bottleneck, fmt, med, peak_mb, randomize, resnet101_shaped  # noqa: E402

DEFAULT_RULE = dict(norm.AUTOGRAD_MIN_ELEMENTS)
DEFAULT_FORK = norm.FORK_AUTOGRAD_MIN_ELEMENTS
# (C, H, W, dilation) of the block outputs at the 640 x 1280 crop, output stride 8, batch 2
TAILS = [(256, 160, 320, 1), (512, 80, 160, 1), (1024, 80, 160, 2), (2048, 80, 160, 4)]


def bound(model):
    """a deep copy in the parent configuration"""
    twin = copy.deepcopy(model)
    Hooked = use_fused_frozen_norm(type("Bottleneck", (Bottleneck,), {}))
    for m in twin.modules():
        if type(m) is Bottleneck:
            m.__class__ = Hooked
    fuse_norm_relu_pairs(twin)
    return twin


def layered_backbone():
    """tools/time_norm_relu.py's stand-in with its 33 blocks in four nn.Sequential layers"""
    flat = list(resnet101_shaped().children())
    stem, blocks, layers = flat[:4], flat[4:], []
    for count in (3, 4, 23, 3):
        layers.append(nn.Sequential(*blocks[:count]))
        blocks = blocks[count:]
    return nn.Sequential(*stem, *layers)


def alternating(fns, n, repeats, warm=3):
    """per closure the per-call times (ms) of `repeats` windows of n calls in the order they ran; the closures alternate window by
    window"""
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
    return out


def own_spread(t):
    """the distance between the medians of a configuration's even and odd windows: what two measurements of the same thing differ by"""
    return abs(med(sorted(t[0::2])) - med(sorted(t[1::2])))


def closure(model, x, g, rule, fork_rule):
    params = [x] + [p for p in model.parameters()]

    def both():
        norm.AUTOGRAD_MIN_ELEMENTS, norm.FORK_AUTOGRAD_MIN_ELEMENTS = rule, fork_rule
        torch.autograd.grad(model(x), params, g)
    return both


def report(say, label, parent, other, counts=None):
    p, c = sorted(parent), sorted(other)
    gain, spread = med(p) - med(c), own_spread(parent)
    say("    %-28s %s   parent - this (medians) %+.4f ms, parent's own spread %.4f ms: %s%s"
        % (label, fmt(c), gain, spread, "WINS" if gain > spread else "does not win", "" if counts is None else "   " + counts))
    return gain > spread


def time_tail(say, dev, args, C, H, W, dilation):
    gen = torch.Generator(device=dev).manual_seed(C)
    torch.manual_seed(C)
    plain = nn.Sequential(*[Bottleneck(C, C // 4, 1, dilation) for _ in range(3)]).to(dev)
    randomize(plain, gen, dev)
    parent = bound(plain)
    chained = bound(plain)
    assert fuse_residual_chains(chained) == 1
    x = torch.randn((2, C, H, W), device=dev, generator=gen).requires_grad_(True)
    g = torch.randn((2, C, H, W), device=dev, generator=gen)
    numel = x.numel()
    say("tails 2 x %d x %d x %d (%d MB each, two of three forked), chain of three bottlenecks of width %d, dilation %d"
        % (C, H, W, numel * 4 // 10**6, C // 4, dilation))
    configs = [("parent", closure(parent, x, g, DEFAULT_RULE, DEFAULT_FORK)), ("chained", closure(chained, x, g, DEFAULT_RULE, 0))]
    if numel < DEFAULT_RULE["plain"]:
        say("    the envelope's size rule leaves these tails to the stock statements in the parent; chained, the two forked tails run the "
            "fused passes and the last one the stock statements")
    counts = {}
    for name, fn in configs:
        before = dict(norm.launches)
        fn()
        counts[name] = "launches fwd %d, bwd %d, fork_bwd %d" % tuple(norm.launches[k] - before[k] for k in ("fwd", "bwd", "fork_bwd"))
    times = alternating([fn for _, fn in configs], args.n, args.repeats)
    say("    %-28s %s   %s" % ("parent", fmt(sorted(times[0])), counts["parent"]))
    wins = [report(say, name, times[0], t, counts[name]) for (name, _), t in zip(configs[1:], times[1:])]
    say("    peak memory above the model and the input over one fwd+bwd: %s"
        % ", ".join("%s %.0f MiB" % (name, peak_mb(fn)) for name, fn in configs))
    norm.AUTOGRAD_MIN_ELEMENTS, norm.FORK_AUTOGRAD_MIN_ELEMENTS = DEFAULT_RULE, DEFAULT_FORK
    return wins[-1]


def time_backbone(say, dev, args):
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    plain = layered_backbone().to(dev)
    randomize(plain, gen, dev)
    parent = bound(plain)
    chained = bound(plain)
    boxes = fuse_residual_chains(chained)
    x = torch.randn((2, 3, 640, 1280), device=dev, generator=gen)
    with torch.no_grad():
        y = plain(x)
    g = torch.randn(y.shape, device=dev, generator=gen)
    del y
    say("backbone 2 x 3 x 640 x 1280, ResNet-101-shaped stand-in in four layers: %d layers chained" % boxes)

    def run(model, fork_rule):
        params = [p for p in model.parameters()]

        def both():
            norm.AUTOGRAD_MIN_ELEMENTS, norm.FORK_AUTOGRAD_MIN_ELEMENTS = DEFAULT_RULE, fork_rule
            torch.autograd.grad(model(x), params, g)
        return both
    configs = [("parent", run(parent, DEFAULT_FORK)), ("chained", run(chained, DEFAULT_FORK)), ("stock", run(plain, DEFAULT_FORK))]
    counts = {}
    for name, fn in configs:
        before = dict(norm.launches)
        fn()
        counts[name] = "launches fwd %d, bwd %d, fork_bwd %d" % tuple(norm.launches[k] - before[k] for k in ("fwd", "bwd", "fork_bwd"))
    times = alternating([fn for _, fn in configs], max(args.n // 4, 2), args.repeats)
    say("    %-28s %s   %s" % ("parent", fmt(sorted(times[0])), counts["parent"]))
    for (name, _), t in zip(configs[1:], times[1:]):
        report(say, name, times[0], t, counts[name])
    say("    peak memory above the model and the input over one fwd+bwd: %s"
        % ", ".join("%s %.0f MiB" % (name, peak_mb(fn)) for name, fn in configs))
    norm.AUTOGRAD_MIN_ELEMENTS, norm.FORK_AUTOGRAD_MIN_ELEMENTS = DEFAULT_RULE, DEFAULT_FORK


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file, line by line")
    ap.add_argument("--append", action="store_true", help="append to --out (the second run)")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--step-seconds", type=int, default=120, help="alarm per tail shape (four times that for the backbone)")
    ap.add_argument("--skip-backbone", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_residual_chain.py needs a ROCm device")
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

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms of forward + backward over %d windows of %d calls per configuration, alternating: best / median / worst"
        % (args.repeats, args.n))
    say("FORK_AUTOGRAD_MIN_ELEMENTS as shipped: %d (the backbone part runs with it); the tails part serves the fork at every size" % DEFAULT_FORK)
    winners = []
    for C, H, W, dilation in TAILS:
        signal.alarm(args.step_seconds)                     # no handler: an overrun ends the process
        if time_tail(say, dev, args, C, H, W, dilation):
            winners.append("2 x %d x %d x %d" % (C, H, W))
        signal.alarm(0)
        torch.cuda.empty_cache()
    say("tail shapes at which the fork wins in this run: %s" % (", ".join(winners) or "none"))
    if not args.skip_backbone:
        signal.alarm(args.step_seconds * 4)
        time_backbone(say, dev, args)
        signal.alarm(0)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
