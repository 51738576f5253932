"""Timing aid: the frozen-norm passes under torch.autocast, halo_amd.norm.norm_relu_autocast against the stock statements (what a
hooked model ran under autocast before the operator existed: every fused pass fell back to them), for float16 and bfloat16.

Part 1, the operator alone at the shapes of the 640 x 1280 training crop, batch 2:

  half     relu(bn(x)) handed to a convolution (a block's bn1 / bn2): stock = the chain and autocast's cast of its result;
  float    a block tail with a float32 identity, and the stem's pair: stock = the chain;
  both     a block tail whose successor reads it as conv input and as identity: stock = the chain and the cast;
  affine   a tail behind a downsample convolution (half residual, its norm folded in), one per layer, outputs="both".

Each is timed forward under no_grad and forward + backward (gradients arrive at every output; x and the residual want theirs).

Part 2, the ResNet-101-shaped stand-in backbone of tools/time_residual_chain.py at 2 x 3 x 640 x 1280 under autocast: unhooked;
hooked with autocast_fallback_reason answering "not served" (the hooks then do what they did before: the stock statements);
hooked as shipped.  Forward under no_grad and forward + backward, with peak memory.

The configurations of a comparison alternate window by window; per configuration best / median / worst per-call time over the
windows.  One run is one process; a speed statement asks for two (run the tool twice, the second time with --append).

    python tools/time_autocast_norm.py [--out profiles/r29_time_autocast_norm.txt] [--append] [--n 10] [--repeats 6] [--skip-backbone]
                                       [--labels both,affine] [--dtypes float16]

HALO_LIB_PATH=<another build of the library> times that build (an A/B of a kernel variant runs the tool once per library, in
separate processes, alternating).
"""
import argparse
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from halo_amd import norm  # noqa: E402
from halo_amd.hooks import fuse_residual_chains  # noqa: E402
from tools.time_norm_relu import FrozenBatchNorm2d, fmt, med, peak_mb, randomize  # noqa: E402
from tools.time_residual_chain import alternating, bound, layered_backbone, own_spread  # noqa: E402

# (label, outputs, residual, C, H, W)
OPERATORS = ([("half", "half", "none", C, H, W) for C, H, W in ((64, 160, 320), (128, 80, 160), (256, 80, 160), (512, 80, 160))]
             + [(o, o, "plain", C, H, W) for o in ("float", "both") for C, H, W in ((256, 160, 320), (512, 80, 160), (1024, 80, 160), (2048, 80, 160))]
             + [("affine", "both", "affine", C, H, W) for C, H, W in ((256, 160, 320), (512, 80, 160), (1024, 80, 160), (2048, 80, 160))]
             + [("stem", "float", "none", 64, 320, 640)])
SERVED = norm.autocast_fallback_reason


def _tuple(out):
    return out if isinstance(out, tuple) else (out,)


def time_operator(say, dev, args, dt, label, outputs, residual, C, H, W):
    """(forward wins, forward + backward wins) of one operator configuration"""
    gen = torch.Generator(device=dev).manual_seed(C + H)
    bn = FrozenBatchNorm2d(C).to(dev)
    rbn = FrozenBatchNorm2d(C).to(dev) if residual == "affine" else None
    randomize(bn, gen, dev)
    if rbn is not None:
        randomize(rbn, gen, dev)
    shape = (2, C, H, W)
    x = torch.randn(shape, device=dev, generator=gen).to(dt).requires_grad_(True)
    r = None
    if residual != "none":
        r = torch.randn(shape, device=dev, generator=gen).to(dt if residual == "affine" else torch.float32).requires_grad_(True)
    ins = [x] if r is None else [x, r]
    gs = {"float": [torch.float32], "half": [dt], "both": [torch.float32, dt]}[outputs]
    gs = [torch.randn(shape, device=dev, generator=gen).to(t) for t in gs]

    def fused():
        return _tuple(norm.norm_relu_autocast(x, bn, r, rbn, outputs))

    def stock():
        return _tuple(norm.autocast_statement(x, bn, r, rbn, outputs))
    wins = []
    with torch.autocast("cuda", dtype=dt):
        assert norm.autocast_fallback_reason(x, bn, r, rbn, outputs) is None
        for a, b in zip(fused(), stock()):
            assert a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.detach()), torch.nan_to_num(b.detach()))
        for a, b in zip(torch.autograd.grad(fused(), ins, gs), torch.autograd.grad(stock(), ins, gs)):
            assert a.dtype == b.dtype and torch.equal(a, b)

        def forward(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        def both(f):
            return lambda: torch.autograd.grad(f(), ins, gs)
        say("  %-6s %s 2 x %d x %d x %d, outputs=%s, residual %s" % (label, str(dt).replace("torch.", ""), C, H, W, outputs, residual))
        for what, wrap in (("fwd", forward), ("fwd+bwd", both)):
            tf, ts = alternating([wrap(fused), wrap(stock)], args.n, args.repeats)
            gain, spread = med(sorted(ts)) - med(sorted(tf)), own_spread(ts)
            win = gain > spread
            wins.append(win)
            say("    %-8s fused %s   stock %s   stock/fused (medians) x%.2f, stock's own spread %.4f ms: %s"
                % (what, fmt(sorted(tf)), fmt(sorted(ts)), med(sorted(ts)) / med(sorted(tf)), spread, "WINS" if win else "FUSED DOES NOT WIN"))
    return wins


def time_backbone(say, dev, args, dt):
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    plain = layered_backbone().to(dev)
    randomize(plain, gen, dev)
    hooked = bound(plain)
    boxes = fuse_residual_chains(hooked)
    x = torch.randn((2, 3, 640, 1280), device=dev, generator=gen)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        y = plain(x)
    g = torch.randn(y.shape, device=dev, generator=gen).to(y.dtype)
    del y
    say("backbone 2 x 3 x 640 x 1280 under autocast(%s), ResNet-101-shaped stand-in, use_fused_frozen_norm + fuse_norm_relu_pairs + "
        "fuse_residual_chains (%d layers chained)" % (str(dt).replace("torch.", ""), boxes))

    def run(model, served, grad):
        params = [p for p in model.parameters()]

        def call():
            norm.autocast_fallback_reason = SERVED if served else (lambda *a, **k: "not served: the configuration before this operator")
            try:
                with torch.autocast("cuda", dtype=dt):
                    if grad:
                        torch.autograd.grad(model(x), params, g)
                    else:
                        with torch.no_grad():
                            model(x)
            finally:
                norm.autocast_fallback_reason = SERVED
        return call
    for what, grad in (("fwd (no_grad)", False), ("fwd+bwd", True)):
        configs = [("unhooked", run(plain, True, grad)), ("hooked before", run(hooked, False, grad)), ("hooked", run(hooked, True, grad))]
        counts = {}
        for name, fn in configs:
            before = dict(norm.launches)
            fn()
            counts[name] = "launches " + ", ".join("%s %d" % (k, norm.launches[k] - before[k]) for k in ("fwd", "bwd", "fork_bwd", "ac_fwd", "ac_bwd"))
        times = alternating([fn for _, fn in configs], max(args.n // 4, 2), args.repeats)
        say("  %s" % what)
        base = sorted(times[1])
        for (name, fn), t in zip(configs, times):
            t = sorted(t)
            say("    %-14s %s   hooked before / this (medians) x%.3f   peak %.0f MiB   %s" % (name, fmt(t), med(base) / med(t), peak_mb(fn), counts[name]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file, line by line")
    ap.add_argument("--append", action="store_true", help="append to --out (the second process of a pair)")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--step-seconds", type=int, default=60, help="alarm per operator configuration (four times that for a backbone)")
    ap.add_argument("--skip-backbone", action="store_true")
    ap.add_argument("--labels", default=None, help="comma-separated operator labels to time (half, float, both, affine, stem); default all")
    ap.add_argument("--dtypes", default="float16,bfloat16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_autocast_norm.py needs a ROCm device")
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

    def overrun(signum, frame):                             # leave a line behind, then end the process
        say("TIME LIMIT: the step above ran past its alarm; the process ends here")
        os._exit(3)
    signal.signal(signal.SIGALRM, overrun)
    halves = [getattr(torch, n) for n in args.dtypes.split(",")]
    operators = [c for c in OPERATORS if args.labels is None or c[0] in args.labels.split(",")]
    say("process %d on %s, torch %s, library %s" % (os.getpid(), torch.cuda.get_device_name(0), torch.__version__,
                                                     os.environ.get("HALO_LIB_PATH") or "as built"))
    say("per-call ms over %d windows of %d calls per configuration, alternating: best / median / worst" % (args.repeats, args.n))
    say("AUTOCAST_AUTOGRAD_MIN_ELEMENTS as shipped: %r (the backbone part runs with it); the operator part serves every size" % (norm.AUTOCAST_AUTOGRAD_MIN_ELEMENTS,))
    shipped, norm.AUTOCAST_AUTOGRAD_MIN_ELEMENTS = norm.AUTOCAST_AUTOGRAD_MIN_ELEMENTS, {}
    losers = []
    for dt in halves:
        for cfg in operators:
            signal.alarm(args.step_seconds)
            fwd, both = time_operator(say, dev, args, dt, *cfg)
            signal.alarm(0)
            if not both:
                losers.append("%s %s 2 x %d x %d x %d" % (cfg[0], str(dt).replace("torch.", ""), *cfg[3:]))
            torch.cuda.empty_cache()
    say("forward + backward does not win at: %s" % ("; ".join(losers) or "no shape timed"))
    norm.AUTOCAST_AUTOGRAD_MIN_ELEMENTS = shipped
    if not args.skip_backbone:
        for dt in halves:
            signal.alarm(args.step_seconds * 4)
            time_backbone(say, dev, args, dt)
            signal.alarm(0)
            torch.cuda.empty_cache()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
