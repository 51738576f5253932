"""Timing aid: halo_amd.fanout.fan_depthwise_bn_relu (the multi-dilation backward of halo_dwconv.hip with the gradients of x's other
readers added where its sum leaves LDS) against the composition it replaces, in the same process on the same device, float32, at
the ASPP pyramid of the v3+ heads (C = 2048, d = 6, 12, 18):

    (a) the operator.  composed: halo_amd.dwconv.multi_depthwise_bn_relu over x, a second reader of x that sends a dense gradient back
        and a third, x.mean((-1, -2), keepdim=True), whose MeanBackward1 writes a full-size gradient; the autograd engine adds the
        three.  joined: fan_depthwise_bn_relu(x, blocks, 2) with the dense gradient at its first alias and
        halo_amd.fanout.plane_mean over its second.  Timed: forward + backward with the gradient of x alone, with the weights' as
        well, and the forward alone (the data gradient is the difference of the first and the last), at
            target      2 x 2048 x 80 x 160 (640 x 1280 crop)
            source      2 x 2048 x 90 x 160 (720 x 1280 crop)
            target/B=1  1 x 2048 x 80 x 160
    (b) the stand-in head of tools/time_euclid_head.py (the reference's widths) under every mark of that tool and
        use_fused_aspp_depthwise, with and without halo_amd.hooks.use_joined_aspp_gradients, forward + backward, at the two crops.

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst.  The two sides alternate window by window.  The whole measurement is made `runs` times; the summary at the
end holds every figure to the rule of DESIGN 23: the joined side WINS a run when its median is below the composed side's by more
than the spread of the composed side's medians between the runs.  No hardware counters are read.

    python tools/time_aspp_fanout.py [--out profiles/r24_time_aspp_fanout.txt] [--n 10] [--repeats 7] [--runs 2] [--no-head]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd import dwconv, fanout  # noqa: E402
from tools.time_dwconv import FrozenBatchNorm2d, fmt, med, peak_mb, windows  # noqa: E402

DILATIONS = (6, 12, 18)
SHAPES = [("target", 2, 2048, 80, 160), ("source", 2, 2048, 90, 160), ("target/B=1", 1, 2048, 80, 160)]


def time_operator(dev, say, n, repeats, record):
    act = nn.ReLU(inplace=True)
    for crop, B, C, H, W in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((B, C, H, W), device=dev, generator=gen).requires_grad_(True)
        blocks = []
        for d in DILATIONS:
            conv = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False).to(dev)
            bn = FrozenBatchNorm2d(C).to(dev)
            with torch.no_grad():
                bn.weight.copy_(0.25 + 1.5 * torch.rand(C, device=dev, generator=gen))
                bn.bias.copy_(0.4 * torch.randn(C, device=dev, generator=gen))
                bn.running_mean.copy_(0.5 * torch.randn(C, device=dev, generator=gen))
                bn.running_var.copy_(0.3 + 1.5 * torch.rand(C, device=dev, generator=gen))
            blocks.append((conv, bn, act))
        assert fanout.fan_fallback_reason(x, blocks, 2) is None, fanout.fan_fallback_reason(x, blocks, 2)
        weights = [b[0].weight for b in blocks]
        gs = [torch.randn((B, C, H, W), device=dev, generator=gen) for _ in blocks]
        gs += [torch.randn((B, C, H, W), device=dev, generator=gen), torch.randn((B, C, 1, 1), device=dev, generator=gen)]

        def joined(t):
            ys, xs = fanout.fan_depthwise_bn_relu(t, blocks, 2)
            return list(ys) + [xs[0], fanout.plane_mean(xs[1])]

        def composed(t):
            return list(dwconv.multi_depthwise_bn_relu(t, blocks)) + [t.view_as(t), t.mean((-1, -2), keepdim=True)]

        ops = {"joined": joined, "composed": composed}
        sides = {}
        for tag, op in ops.items():
            def fwd(op=op):
                with torch.no_grad():
                    op(x)

            def both(op=op):
                return torch.autograd.grad(op(x), [x] + weights, gs)

            def data(op=op):
                for w in weights:                         # a weight that requires a gradient gets one whatever grad() is asked for
                    w.requires_grad_(False)
                try:
                    return torch.autograd.grad(op(x), [x], gs)
                finally:
                    for w in weights:
                        w.requires_grad_(True)
            sides[tag] = dict(fwd=fwd, both=both, data=data)
        kinds = ("fwd", "both", "data")
        order = [(t, k) for k in kinds for t in ("joined", "composed")]
        times = dict(zip(order, windows([sides[t][k] for t, k in order], n, repeats)))
        nbytes = x.numel() * 4
        say("%-10s %s  d = %s  (x: %.0f MB)" % (crop, "x".join(map(str, (B, C, H, W))), DILATIONS, nbytes / 1e6))
        for k, label in (("fwd", "forward"), ("both", "fwd+bwd (x, w)"), ("data", "fwd+bwd (x)")):
            f, s = times[("joined", k)], times[("composed", k)]
            say("    %-15s joined %s   composed %s   composed - joined (medians) %.4f ms   x%.2f"
                % (label, fmt(f), fmt(s), med(s) - med(f), med(s) / med(f)))
            if k != "fwd":
                record("operator, %s, %s" % (crop, label), med(f), med(s))
        fb = med(times[("joined", "data")]) - med(times[("joined", "fwd")])
        cb = med(times[("composed", "data")]) - med(times[("composed", "fwd")])
        say("    data gradient alone (fwd+bwd (x) less forward, medians): joined %.4f   composed %.4f   x%.2f   (6 x %.0f MB saved on paper: %.2f TB/s)"
            % (fb, cb, cb / fb, nbytes / 1e6, 6 * nbytes / max(cb - fb, 1e-9) * 1e3 / 1e12))
        got, want = sides["joined"]["both"](), sides["composed"]["both"]()
        same = all(torch.equal(a, b) for a, b in zip(got[1:], want[1:]))
        with torch.no_grad():
            same = same and all(torch.equal(a, b) for a, b in zip(ops["joined"](x), ops["composed"](x)))
        say("    same bits (y_i, the mean, g_w_i): %s; max |g_x - the engine's sum| = %.3g; peak memory above the operands over one fwd+bwd: "
            "joined %.1f MiB, composed %.1f MiB"
            % (same, float((got[0] - want[0]).abs().max()), peak_mb(sides["joined"]["both"]), peak_mb(sides["composed"]["both"])))
        del got, want, sides, times, x, gs, blocks, weights, ops
        torch.cuda.empty_cache()


def time_heads(dev, say, n, repeats, record):
    """tools/time_euclid_head.py's head under every mark of that tool and use_fused_aspp_depthwise, with and without
    use_joined_aspp_gradients"""
    from halo_amd import hooks
    from tools.time_euclid_head import CROPS, Block, Head
    MarkedBlock = type("MarkedBlock", (Block,), {})
    hooks.use_fused_depthwise(MarkedBlock), hooks.use_fused_pointwise_norm(MarkedBlock)
    heads = {}
    for tag in ("joined", "parent"):
        cls = hooks.use_v3plus_forward(type("Head_" + tag, (Head,), {}))
        for mark in (hooks.use_device_resize, hooks.use_fused_decoder_front, hooks.use_folded_image_pooling, hooks.use_fused_decoder_dropout,
                     hooks.use_fused_aspp_depthwise):
            mark(cls)
        if tag == "joined":
            hooks.use_joined_aspp_gradients(cls)
        heads[tag] = cls(MarkedBlock).to(dev).train()
        hooks.fuse_norm_relu_pairs(heads[tag])
    heads["joined"].load_state_dict(heads["parent"].state_dict())
    for where, h, w, H, W in CROPS:
        gen = torch.Generator(device=dev).manual_seed(1)
        feats = {"out": torch.randn((2, 2048, h, w), device=dev, generator=gen).relu_().requires_grad_(True),
                 "low": torch.randn((2, 256, H, W), device=dev, generator=gen).relu_().requires_grad_(True)}
        g = torch.randn((2, 19, H, W), device=dev, generator=gen)
        sides = {}
        for tag, head in heads.items():
            leaves = [feats["out"], feats["low"]] + [p for p in head.parameters() if p.requires_grad]

            def both(head=head, leaves=leaves):
                torch.autograd.grad(head(feats)[0], leaves, g)
            sides[tag] = both
        before = {**dwconv.launches, **fanout.launches}
        sides["joined"]()
        ran = {k: v - before[k] for k, v in {**dwconv.launches, **fanout.launches}.items()}
        m, s = windows([sides["joined"], sides["parent"]], n, repeats)
        say("head, %s: top 2x2048x%dx%d, low 2x256x%dx%d   (passes of one marked step: %s)" % (where, h, w, H, W, ran))
        say("    forward + backward   marked %s   parent %s   parent - marked (medians) %.3f ms   x%.3f   parent's window spread %.4f"
            % (fmt(m), fmt(s), med(s) - med(m), med(s) / med(m), s[-1] - s[0]))
        record("head, %s, forward + backward" % where, med(m), med(s))
        del sides, feats, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no-head", action="store_true", help="leave out (b), the whole head")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_aspp_fanout.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines, figures = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def record(what, joined_ms, composed_ms):
        figures.setdefault(what, []).append((joined_ms, composed_ms))

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst (the head: 5 windows of 3 calls)" % (args.repeats, args.n))
    from halo_amd import norm
    for run in range(args.runs):
        say("---- run %d of %d" % (run + 1, args.runs))
        time_operator(dev, say, args.n, args.repeats, record)
        if not args.no_head:
            rules = norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS                 # as tools/time_euclid_head.py runs its heads
            norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS = {k: 0 for k in rules[0]}, 0
            time_heads(dev, say, 3, 5, record)
            norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS = rules
    say("---- summary: medians per run, joined / composed (or marked / parent); margin = the composed side's spread between the runs")
    for what, runs in figures.items():
        margin = max(c for _, c in runs) - min(c for _, c in runs)
        wins = all(c - j > margin for j, c in runs)
        verdict = "one run: no margin, no verdict" if len(runs) < 2 else "WINS in every run" if wins else "does not win in every run"
        say("    %-44s %s   margin %.4f   %s" % (what, "   ".join("%.4f / %.4f" % r for r in runs), margin, verdict))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
