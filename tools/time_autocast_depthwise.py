"""Timing aid: the depthwise half of a separable block under torch.autocast, halo_amd.dwconv.depthwise_bn_relu_autocast
(halo_half_dwconv3x3_* of halo_dwconv.hip) against halo_amd.dwconv.autocast_statement -- the stock statements under autocast with
the casts on both ends included: autocast's cast of a float32 x in front of the conv, and its cast of the ReLU's float32 result in
front of the pointwise conv.  float16 and bfloat16, a float32 and a half x, at the separable blocks of the v3+ heads:

    aspp        B x 2048 x 80 x 160 and B x 2048 x 90 x 160, d = 6, 12, 18
    dec0 / dec1 B x 560 and B x 512 x 160 x 320 and x 180 x 320, d = 1
    each at B = 2 and B = 1, and the test-time shapes 2 x 2048 x 128 x 256 (d = 6, 12, 18) and 2 x 512 x 256 x 512

Per shape: forward under no_grad, forward + backward for x alone, forward + backward for x and the weight.  HIP events around n
calls after three warm-up calls of every closure; `repeats` windows per figure, printed as best / median / worst; the two sides
alternate window by window.  The fused side WINS a figure only when its median lies below the stock side's by more than the stock
side's own best-to-worst spread.  --head adds tools/time_euclid_head.py's stand-in head under autocast, blocks under
use_fused_depthwise, marked by use_autocast_depthwise against unmarked: forward under no_grad and forward + backward.  One run is
one process; a speed statement asks for two (the second with --append).

    python tools/time_autocast_depthwise.py [--out profiles/r31_time_autocast_depthwise.txt] [--append] [--head] [--n 5] [--repeats 5]
                                            [--dtypes float16,bfloat16] [--only aspp]

HALO_LIB_PATH=<another build of the library> times that build.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd import dwconv  # noqa: E402
from tools.time_dwconv import FrozenBatchNorm2d, fmt, med, windows  # noqa: E402

# (label, B, C, H, W, dilations)
SHAPES = ([("aspp", B, 2048, H, 160, (6, 12, 18)) for B in (2, 1) for H in (80, 90)]
          + [("dec", B, C, H, 320, (1,)) for B in (2, 1) for C in (560, 512) for H in (160, 180)]
          + [("test aspp", 2, 2048, 128, 256, (6, 12, 18)), ("test dec", 2, 512, 256, 512, (1,))])


def verdict(f, s):
    """the fused side's sorted times against the stock side's: the rule of the module docstring"""
    if med(s) - med(f) > s[-1] - s[0]:
        return "WINS"
    if med(f) - med(s) > f[-1] - f[0]:
        return "LOSES"
    return "undecided"


def modules(C, d, dev, gen):
    conv = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False).to(dev)
    bn = FrozenBatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, device=dev, generator=gen)), bn.bias.copy_(0.2 * torch.randn(C, device=dev, generator=gen))
        bn.running_mean.copy_(0.2 * torch.randn(C, device=dev, generator=gen)), bn.running_var.copy_(0.5 + torch.rand(C, device=dev, generator=gen))
    return conv, bn


def time_shape(say, dev, args, dt, half_x, label, B, C, H, W, d):
    """the verdicts of the three figures of one configuration"""
    gen = torch.Generator(device=dev).manual_seed(C + H + d)
    conv, bn = modules(C, d, dev, gen)
    x = torch.randn((B, C, H, W), device=dev, generator=gen)
    x = (x.to(dt) if half_x else x).requires_grad_(True)
    g = torch.randn((B, C, H, W), device=dev, generator=gen).to(dt)
    sides = {"fused": dwconv.depthwise_bn_relu_autocast, "stock": dwconv.autocast_statement}
    out = []
    # every call enters autocast anew, as a step does: autocast caches its casts of float32 leaves for the life of one context, and
    # a cast cached under no_grad has no graph
    with torch.autocast("cuda", dtype=dt):
        assert dwconv.autocast_fallback_reason(x, conv, bn) is None
        with torch.no_grad():
            a, b = sides["fused"](x, conv, bn), sides["stock"](x, conv, bn)
        differ = int((a != b).sum())
        del a, b

    def forward(fn):
        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=dt):
                fn(x, conv, bn)
        return run

    def backward(fn, leaves):
        def run():
            with torch.autocast("cuda", dtype=dt):
                y = fn(x, conv, bn)
            torch.autograd.grad(y, leaves, g)
        return run
    say("  %-9s %s x %s  %d x %d x %d x %d, d = %d   (elements that differ from the stock chain: %d of %d)"
        % (label, str(dt).replace("torch.", ""), "half" if half_x else "float32", B, C, H, W, d, differ, x.numel()))
    for what, wrap in (("fwd", forward), ("fwd+bwd x", lambda fn: backward(fn, [x])), ("fwd+bwd x,w", lambda fn: backward(fn, [x, conv.weight]))):
        conv.weight.requires_grad_(what == "fwd+bwd x,w")
        f, s = windows([wrap(sides["fused"]), wrap(sides["stock"])], args.n, args.repeats)
        out.append(verdict(f, s))
        say("    %-12s fused %s   stock %s   stock/fused (medians) x%.2f   stock's spread %.4f ms   fused %s"
            % (what, fmt(f), fmt(s), med(s) / med(f), s[-1] - s[0], out[-1]))
    return out


def time_heads(say, dev, args, dt):
    from halo_amd import hooks
    from tools.time_euclid_head import CROPS, Block, Head
    heads = {}
    for tag in ("marked", "unmarked"):
        blk = hooks.use_fused_depthwise(type("Block_" + tag, (Block,), {}))
        cls = hooks.use_v3plus_forward(type("Head_" + tag, (Head,), {}))
        if tag == "marked":
            hooks.use_autocast_depthwise(blk)
        heads[tag] = cls(blk).to(dev).eval()
    heads["marked"].load_state_dict(heads["unmarked"].state_dict())
    for where, h, w, H, W in CROPS:
        gen = torch.Generator(device=dev).manual_seed(1)
        feats = {"out": torch.randn((2, 2048, h, w), device=dev, generator=gen).relu_().requires_grad_(True),
                 "low": torch.randn((2, 256, H, W), device=dev, generator=gen).relu_().requires_grad_(True)}
        fwd, both = {}, {}
        for tag, head in heads.items():
            leaves = [feats["out"], feats["low"]] + [p for p in head.parameters() if p.requires_grad]

            def forward(head=head):
                with torch.no_grad(), torch.autocast("cuda", dtype=dt):
                    head(feats)

            def step(head=head, leaves=leaves):
                with torch.autocast("cuda", dtype=dt):
                    out = head(feats)[0]
                torch.autograd.grad(out.float().square().mean(), leaves)
            fwd[tag], both[tag] = forward, step
        before = dict(dwconv.autocast_launches)
        both["marked"]()
        ran = {k: dwconv.autocast_launches[k] - before[k] for k in before}
        say("head under autocast(%s), %s: top 2x2048x%dx%d, low 2x256x%dx%d   (launches of one marked step: %s)"
            % (str(dt).replace("torch.", ""), where, h, w, H, W, ran))
        for what, sides in (("fwd (no_grad)", fwd), ("fwd+bwd", both)):
            m, u = windows([sides["marked"], sides["unmarked"]], max(args.n // 2, 2), args.repeats)
            say("    %-14s marked %s   unmarked %s   unmarked - marked (medians) %.3f ms   x%.3f   unmarked's spread %.4f   marked %s"
                % (what, fmt(m), fmt(u), med(u) - med(m), med(u) / med(m), u[-1] - u[0], verdict(m, u)))
        del fwd, both, feats
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file, line by line")
    ap.add_argument("--append", action="store_true", help="append to --out (the second process of a pair)")
    ap.add_argument("--head", action="store_true", help="also time the stand-in head, marked against unmarked")
    ap.add_argument("--skip-shapes", action="store_true", help="the head alone")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dtypes", default="float16,bfloat16")
    ap.add_argument("--only", default=None, help="time the shapes whose label contains this")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_autocast_depthwise.py needs a ROCm device")
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
    say("process %d on %s, torch %s, library %s" % (os.getpid(), torch.cuda.get_device_name(0), torch.__version__,
                                                     os.environ.get("HALO_LIB_PATH") or "as built"))
    say("per-call ms over %d windows of %d calls per side, alternating: best / median / worst" % (args.repeats, args.n))
    halves = [getattr(torch, n) for n in args.dtypes.split(",")]
    not_won = []
    if not args.skip_shapes:
        for label, B, C, H, W, dil in SHAPES:
            if args.only and args.only not in label:
                continue
            for d in dil:
                for dt in halves:
                    for half_x in (False, True):
                        got = time_shape(say, dev, args, dt, half_x, label, B, C, H, W, d)
                        for what, v in zip(("fwd", "fwd+bwd x", "fwd+bwd x,w"), got):
                            if v != "WINS":
                                not_won.append("%s %s x %s %dx%dx%dx%d d=%d %s: %s" % (label, str(dt).replace("torch.", ""),
                                                                                       "half" if half_x else "float32", B, C, H, W, d, what, v))
                        torch.cuda.empty_cache()
        say("figures the fused side does not win: %s" % ("; ".join(not_won) or "none of those timed"))
    if args.head:
        for dt in halves:
            time_heads(say, dev, args, dt)
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
