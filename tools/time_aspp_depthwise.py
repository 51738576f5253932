"""Timing aid: halo_amd.dwconv.multi_depthwise_bn_relu (the LDS-resident multi-dilation passes of halo_dwconv.hip) against the
composition it replaces -- one halo_amd.dwconv.depthwise_bn_relu per dilation over the same input, whose three input gradients the
autograd engine adds -- in the same process on the same device, float32, at the ASPP pyramid of the v3+ heads (C = 2048,
d = 6, 12, 18):

    target      2 x 2048 x 80 x 160 (640 x 1280 crop)
    source      2 x 2048 x 90 x 160 (720 x 1280 crop)
    target/B=1  1 x 2048 x 80 x 160 under no_grad (RegionSelection, validation)

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst.  The two sides alternate window by window.  Reported: forward alone (no_grad), forward + backward with the
gradients of x and the three weights, forward + backward with the gradient of x alone, the fused forward's achieved bytes/s against
its one-read-N-writes traffic, torch.cuda.max_memory_allocated over one forward + backward above what the operands hold, and
whether the two sides returned the same bits.  Run it twice (the second time with --append): the serving rule compares the two
runs' medians.  --head adds the whole stand-in head of tools/time_euclid_head.py under every mark of that tool, with and
without halo_amd.hooks.use_fused_aspp_depthwise (5 windows of 3 calls).

    python tools/time_aspp_depthwise.py [--out profiles/r23_time_aspp_depthwise.txt] [--append] [--head] [--n 10] [--repeats 7]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from halo_amd.dwconv import depthwise_bn_relu, launches, multi_depthwise_bn_relu, multi_fallback_reason  # noqa: E402
from tools.time_dwconv import FrozenBatchNorm2d, fmt, med, peak_mb, windows  # noqa: E402

DILATIONS = (6, 12, 18)
SHAPES = [("target", 2, 2048, 80, 160), ("source", 2, 2048, 90, 160), ("target/B=1", 1, 2048, 80, 160)]


def time_heads(dev, say, n, repeats):
    """tools/time_euclid_head.py's head under every mark of that tool, with and without use_fused_aspp_depthwise"""
    from halo_amd import hooks
    from tools.time_euclid_head import CROPS, Block, Head
    MarkedBlock = type("MarkedBlock", (Block,), {})
    hooks.use_fused_depthwise(MarkedBlock), hooks.use_fused_pointwise_norm(MarkedBlock)
    heads = {}
    for tag in ("pyramid", "parent"):
        cls = hooks.use_v3plus_forward(type("Head_" + tag, (Head,), {}))
        for mark in (hooks.use_device_resize, hooks.use_fused_decoder_front, hooks.use_folded_image_pooling, hooks.use_fused_decoder_dropout):
            mark(cls)
        if tag == "pyramid":
            hooks.use_fused_aspp_depthwise(cls)
        heads[tag] = cls(MarkedBlock).to(dev).train()
        hooks.fuse_norm_relu_pairs(heads[tag])
    heads["pyramid"].load_state_dict(heads["parent"].state_dict())
    for where, h, w, H, W in CROPS:
        gen = torch.Generator(device=dev).manual_seed(1)
        feats = {"out": torch.randn((2, 2048, h, w), device=dev, generator=gen).relu_().requires_grad_(True),
                 "low": torch.randn((2, 256, H, W), device=dev, generator=gen).relu_().requires_grad_(True)}
        g = torch.randn((2, 19, H, W), device=dev, generator=gen)
        sides = {}
        for tag, head in heads.items():
            leaves = [feats["out"], feats["low"]] + [p for p in head.parameters() if p.requires_grad]

            def fwd(head=head):
                with torch.no_grad():
                    head(feats)

            def both(head=head, leaves=leaves):
                torch.autograd.grad(head(feats)[0], leaves, g)
            sides[tag] = dict(fwd=fwd, both=both)
        before = dict(launches)
        sides["pyramid"]["both"]()
        ran = {k: launches[k] - before[k] for k in before}
        order = [(t, k) for k in ("fwd", "both") for t in ("pyramid", "parent")]
        times = dict(zip(order, windows([sides[t][k] for t, k in order], n, repeats)))
        say("head, %s: top 2x2048x%dx%d, low 2x256x%dx%d   (multi-dilation passes of one marked step: %s)" % (where, h, w, H, W, ran))
        for k, label in (("fwd", "forward, no_grad"), ("both", "forward + backward")):
            m, s = times[("pyramid", k)], times[("parent", k)]
            say("    %-20s marked %s   parent %s   parent - marked (medians) %.3f ms   x%.3f   parent's spread %.4f"
                % (label, fmt(m), fmt(s), med(s) - med(m), med(s) / med(m), s[-1] - s[0]))
        del sides, times, feats, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--head", action="store_true", help="also time the whole v3+ head of tools/time_euclid_head.py, marked and unmarked")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_aspp_depthwise.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    act = nn.ReLU(inplace=True)
    for crop, B, C, H, W in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((B, C, H, W), device=dev, generator=gen).requires_grad_(B > 1)
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
        assert multi_fallback_reason(x, blocks) is None, multi_fallback_reason(x, blocks)
        weights = [b[0].weight for b in blocks]
        gs = [torch.randn((B, C, H, W), device=dev, generator=gen) for _ in blocks] if B > 1 else None
        ops = {"fused": lambda t: multi_depthwise_bn_relu(t, blocks), "composed": lambda t: tuple(depthwise_bn_relu(t, *b) for b in blocks)}
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
        kinds = ("fwd", "both", "data") if B > 1 else ("fwd",)
        order = [(t, k) for k in kinds for t in ("fused", "composed")]
        times = dict(zip(order, windows([sides[t][k] for t, k in order], args.n, args.repeats)))
        nbytes = x.numel() * 4
        say("%-10s %s  d = %s  (x: %.0f MB)" % (crop, "x".join(map(str, (B, C, H, W))), DILATIONS, nbytes / 1e6))
        for k, label in (("fwd", "forward"), ("both", "fwd+bwd (x, w)"), ("data", "fwd+bwd (x)")):
            if k not in kinds:
                continue
            f, s = times[("fused", k)], times[("composed", k)]
            say("    %-15s fused %s   composed %s   composed/fused (medians) x%.2f%s"
                % (label, fmt(f), fmt(s), med(s) / med(f), "" if med(f) <= med(s) else "   FUSED LOSES"))
        if B > 1:
            fb = med(times[("fused", "data")]) - med(times[("fused", "fwd")])
            cb = med(times[("composed", "data")]) - med(times[("composed", "fwd")])
            say("    data gradient alone (fwd+bwd (x) less forward, medians): fused %.4f   composed %.4f   x%.2f" % (fb, cb, cb / fb))
        traffic = (1 + len(DILATIONS)) * nbytes
        say("    fused forward: %.2f TB/s of its one-read-%d-writes traffic (%.0f MB)"
            % (traffic / (med(times[("fused", "fwd")]) * 1e-3) / 1e12, len(DILATIONS), traffic / 1e6))
        with torch.no_grad():
            same = all(torch.equal(a, b) for a, b in zip(ops["fused"](x), ops["composed"](x)))
        if B > 1:
            got, want = sides["fused"]["both"](), sides["composed"]["both"]()
            same = same and all(torch.equal(a, b) for a, b in zip(got[1:], want[1:]))
            # the engine adds the composition's three g_x in an order of its own: (a + b) + c in another association
            say("    same bits (y_i, g_w_i): %s; max |g_x - the engine's sum| = %.3g; peak memory above the operands over one fwd+bwd: "
                "fused %.1f MiB, composed %.1f MiB"
                % (same, float((got[0] - want[0]).abs().max()), peak_mb(sides["fused"]["both"]), peak_mb(sides["composed"]["both"])))
            del got, want
        else:
            say("    same bits (y_i): %s" % same)
        del sides, times, x, gs, blocks, weights, ops
        torch.cuda.empty_cache()
    if args.head:
        from halo_amd import norm
        rules = norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS                 # as tools/time_euclid_head.py runs its heads
        norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS = {k: 0 for k in rules[0]}, 0
        time_heads(dev, say, 3, 5)
        norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS = rules
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
