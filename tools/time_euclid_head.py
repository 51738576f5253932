"""Timing aid: the Euclidean DeepLab-v3+ head (DepthwiseSeparableASPP in its old decoder layout, the head of configs/gtav/ripu.yaml)
bound with halo_amd.hooks.use_v3plus_forward and marked with every head-level and block-level hook, against the same head on its
stock statements, in the same process on the same device, float32.

A stand-in head with the reference's widths (2048 -> 4 x 512 -> 512, shortcut 256 -> 48, decoder 560 -> 512 -> 512, Dropout2d(0.1),
19 classes) in train() mode at the two crops of that configuration:

    target crop   top 2 x 2048 x 80 x 160, low 2 x 256 x 160 x 320
    source crop   top 2 x 2048 x 90 x 160, low 2 x 256 x 180 x 320

and the two-output pass of its decoder on its own, halo_amd.norm.norm_relu_dropout2d_pair, against norm_relu followed by the stock
nn.Dropout2d and against the stock statements, forward + backward with the gradient of z alone (a training step never uses
decoder_out) and with both gradients.

HIP events around n calls after three warm-up calls of every timed closure; `repeats` windows per figure, printed as
best / median / worst.  The sides alternate window by window.  The whole measurement is made `runs` times.  The size rules of the
envelopes (halo_amd.norm.AUTOGRAD_MIN_ELEMENTS, PAIR_AUTOGRAD_MIN_ELEMENTS) are switched off for the run: the measurement decides
them.  A side WINS when its median is below the other's by more than the other side's own best-to-worst spread.  No hardware
counters are read.

    python tools/time_euclid_head.py [--out profiles/r16_time_euclid_head.txt] [--n 3] [--repeats 5] [--runs 2]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from halo_amd import hooks, norm  # noqa: E402
from tools.time_dwconv import FrozenBatchNorm2d, fmt, med, windows  # noqa: E402

CROPS = [("target crop", 80, 160, 160, 320), ("source crop", 90, 160, 180, 320)]
PAIR_SHAPES = [(2, 512, 160, 320), (2, 512, 180, 320), (1, 512, 160, 320), (2, 512, 80, 160), (1, 512, 90, 160)]


def _randomize(bn, gen):
    n = bn.weight.numel()
    with torch.no_grad():
        bn.weight.copy_(0.25 + 1.5 * torch.rand(n, generator=gen)), bn.bias.copy_(0.4 * torch.randn(n, generator=gen))
        bn.running_mean.copy_(0.5 * torch.randn(n, generator=gen)), bn.running_var.copy_(0.3 + 1.5 * torch.rand(n, generator=gen))
    return bn


class Block(nn.Module):
    """DepthwiseSeparableConv2d's attribute names and statements"""

    def __init__(self, cin, cout, d, gen):
        super().__init__()
        self.depthwise_conv = nn.Conv2d(cin, cin, 3, 1, d, d, groups=cin, bias=False)
        self.depthwise_bn = _randomize(FrozenBatchNorm2d(cin), gen)
        self.depthwise_activate = nn.ReLU(inplace=True)
        self.pointwise_conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.pointwise_bn = _randomize(FrozenBatchNorm2d(cout), gen)
        self.pointwise_activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.depthwise_activate(self.depthwise_bn(self.depthwise_conv(x)))
        return self.pointwise_activate(self.pointwise_bn(self.pointwise_conv(x)))


class Head(nn.Module):
    """the Euclidean v3+ head's attribute layout, old decoder layout, reference widths; forward: the stock statements"""

    def __init__(self, block, top=2048, mid=512, low=256, short=48, K=19):
        super().__init__()
        gen = torch.Generator().manual_seed(0)
        norm_ = lambda n: _randomize(FrozenBatchNorm2d(n), gen)
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(top, mid, 1, bias=False), norm_(mid), nn.ReLU(inplace=True))] + [
            block(top, mid, d, gen) for d in (6, 12, 18)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Conv2d(top, mid, 1, bias=False), norm_(mid), nn.ReLU(inplace=True))
        self.bottleneck = nn.Sequential(nn.Conv2d(5 * mid, mid, 3, padding=1, bias=False), norm_(mid), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(low, short, 1, bias=False), norm_(short), nn.ReLU(inplace=True))
        self.old_decoder = True
        self.decoder = nn.Sequential(block(mid + short, mid, 1, gen), block(mid, mid, 1, gen), nn.Dropout2d(0.1), nn.Conv2d(mid, K, 1))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data = torch.randn(m.weight.shape, generator=gen) * (2.0 / m.weight[0].numel() ** 0.5)

    def forward(self, x, size=None):
        low, x = x["low"], x["out"]
        aspp = [branch(x) for branch in self.parallel_branches]
        aspp.append(F.interpolate(self.global_branch(x), size=x.size()[2:], mode="bilinear", align_corners=True))
        top = F.interpolate(self.bottleneck(torch.cat(aspp, dim=1)), size=low.size()[2:], mode="bilinear", align_corners=True)
        feats = torch.cat([top, self.shortcut(low)], dim=1)
        for i in range(len(self.decoder)):
            feats = self.decoder[i](feats)
            if i == 1:
                decoder_out = feats
        if size is not None:
            feats = F.interpolate(feats, size=size, mode="bilinear", align_corners=True)
        return feats, decoder_out


def verdict(a, b):
    """a against b: the rule of the module docstring"""
    if med(b) - med(a) > b[-1] - b[0]:
        return "wins"
    if med(a) - med(b) > a[-1] - a[0]:
        return "LOSES"
    return "no difference"


def time_heads(dev, say, n, repeats):
    class Marked(Head):
        pass

    class MarkedBlock(Block):
        pass

    hooks.use_v3plus_forward(Marked)
    for mark in (hooks.use_device_resize, hooks.use_fused_decoder_front, hooks.use_folded_image_pooling, hooks.use_fused_decoder_dropout):
        mark(Marked)
    hooks.use_fused_depthwise(MarkedBlock), hooks.use_fused_pointwise_norm(MarkedBlock)
    stock, marked = Head(Block).to(dev).train(), Marked(MarkedBlock).to(dev).train()
    marked.load_state_dict(stock.state_dict())
    say("pairs fused by fuse_norm_relu_pairs: %d" % hooks.fuse_norm_relu_pairs(marked))
    for where, h, w, H, W in CROPS:
        gen = torch.Generator(device=dev).manual_seed(1)
        feats = {"out": torch.randn((2, 2048, h, w), device=dev, generator=gen).relu_().requires_grad_(True),
                 "low": torch.randn((2, 256, H, W), device=dev, generator=gen).relu_().requires_grad_(True)}
        g = torch.randn((2, 19, H, W), device=dev, generator=gen)
        sides = {}
        for tag, head in (("marked", marked), ("stock", stock)):
            leaves = [feats["out"], feats["low"]] + [p for p in head.parameters() if p.requires_grad]

            def fwd(head=head):
                with torch.no_grad():
                    head(feats)

            def both(head=head, leaves=leaves):
                torch.autograd.grad(head(feats)[0], leaves, g)
            sides[tag] = dict(fwd=fwd, both=both)
        before = dict(norm.launches)
        sides["marked"]["both"]()
        ran = {k: norm.launches[k] - before[k] for k in before if norm.launches[k] != before[k]}
        order = [(t, k) for k in ("fwd", "both") for t in ("marked", "stock")]
        times = dict(zip(order, windows([sides[t][k] for t, k in order], n, repeats)))
        say("%s: top 2x2048x%dx%d, low 2x256x%dx%d   (halo_norm.hip passes of one marked step: %s)" % (where, h, w, H, W, ran))
        for k, label in (("fwd", "forward, no_grad"), ("both", "forward + backward")):
            m, s = times[("marked", k)], times[("stock", k)]
            say("    %-20s marked %s   stock %s   stock - marked (medians) %.3f ms   stock/marked x%.3f   stock spread %.4f   marked %s"
                % (label, fmt(m), fmt(s), med(s) - med(m), med(s) / med(m), s[-1] - s[0], verdict(m, s)))
        del sides, times, feats, g
        torch.cuda.empty_cache()


def time_pair(dev, say, n, repeats):
    drop = nn.Dropout2d(0.1).train()
    for shape in PAIR_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(2)
        x = torch.randn(shape, device=dev, generator=gen).requires_grad_(True)
        gz, gy = torch.randn(shape, device=dev, generator=gen), torch.randn(shape, device=dev, generator=gen)
        bn = _randomize(FrozenBatchNorm2d(shape[1]), torch.Generator().manual_seed(3)).to(dev)
        assert norm.pair_fallback_reason(x, bn, drop) is None and norm.fallback_reason(x, bn) is None

        def two_statements():
            y = norm.norm_relu(x, bn)
            return y, drop(y)
        ops = (("pair", lambda: norm.norm_relu_dropout2d_pair(x, bn, drop)), ("norm_relu + Dropout2d", two_statements),
               ("stock", lambda: norm.pair_statement(x, bn, drop)))
        closures, order = [], []
        for tag, op in ops:
            closures.append(lambda op=op: torch.autograd.grad(op()[1], x, gz))
            closures.append(lambda op=op: torch.autograd.grad(list(op()), x, [gy, gz]))
            order += [(tag, "g_z"), (tag, "g_y, g_z")]
        times = dict(zip(order, windows(closures, n, repeats)))
        say("pair operator at %dx%dx%dx%d  (%d elements), forward + backward" % (shape + (x.numel(),)))
        for grads in ("g_z", "g_y, g_z"):
            p = times[("pair", grads)]
            for tag in ("norm_relu + Dropout2d", "stock"):
                o = times[(tag, grads)]
                say("    %-9s pair %s   %-21s %s   other - pair (medians) %.4f ms   other/pair x%.3f   other's spread %.4f   pair %s"
                    % (grads, fmt(p), tag, fmt(o), med(o) - med(p), med(o) / med(p), o[-1] - o[0], verdict(p, o)))
        with torch.no_grad():                      # the same bits, checked where they are timed
            torch.manual_seed(1)
            a = ops[0][1]()
            torch.manual_seed(1)
            b = ops[2][1]()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            del a, b
        del closures, times, ops, x, gy, gz, bn
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-heads", action="store_true", help="time the pair operator alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_euclid_head.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("per-call ms over %d windows of %d calls: best / median / worst" % (args.repeats, args.n))
    rules = norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS
    norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS = {k: 0 for k in rules[0]}, 0
    for run in range(args.runs):
        say("---- run %d of %d" % (run + 1, args.runs))
        if not args.skip_heads:
            time_heads(dev, say, args.n, args.repeats)
        time_pair(dev, say, max(args.n, 5), args.repeats)
    norm.AUTOGRAD_MIN_ELEMENTS, norm.PAIR_AUTOGRAD_MIN_ELEMENTS = rules
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
