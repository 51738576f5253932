"""Timing aid: the joint depthwise backward (halo_joint_dwconv3x3_affine_relu_bwd / halo_joint_upcat_dwconv3x3_affine_relu_bwd of
halo_dwconv.hip: g_x and g_w from one walk) against the two entries it replaces (..._bwd_data, then ..._bwd_weight) on the same
operands, in the same process on the same device, float32, at the separable blocks of the v3+ heads:

    dec1        B x 512 x 160 x 320, d = 1                       (the 16-byte route <4, true>)
    aspp        B x 2048 x 80 x 160 and B x 2048 x 90 x 160, d = 6, 12, 18     (<4, false>)
    front       a B x 512 x 80 x 160 with s B x 48 x 160 x 320, and 90 x 160 with 180 x 320 (the decoder front; the resize
                backward behind g_up is the same call on both sides and is left out)
    each at B = 2 and B = 1

The baseline is always the parents' two entries, never the joint entry against itself.  HIP events around n calls after three
warm-up calls of every timed closure; `repeats` windows per figure, printed as best / median / worst; the two sides alternate window
by window; outputs and workspaces are allocated once, outside the windows.  The joint side WINS a shape only when its median lies
below the separate side's by more than the separate side's own best-to-worst spread.  --head adds one stand-in head
(tools/time_euclid_head.py's, blocks under use_fused_depthwise, head under use_device_resize + use_fused_decoder_front), forward +
backward, block and head classes marked by use_joint_depthwise_backward against unmarked, once under the served speed rule
(halo_amd.dwconv.JOINT_MIN_ELEMENTS) and once with the rule switched off, so that every block of the marked head runs the joint
pass.  Run it twice (the second time with --append): a route is served only where it wins in both processes.

    python tools/time_joint_depthwise.py [--out profiles/r25_time_joint_depthwise.txt] [--append] [--head] [--n 10] [--repeats 7]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from halo_amd import _lib, dwconv  # noqa: E402
from tools.time_dwconv import fmt, med, windows  # noqa: E402

PLAIN = [("dec1", 512, 160, 320, (1,)), ("aspp target", 2048, 80, 160, (6, 12, 18)), ("aspp source", 2048, 90, 160, (6, 12, 18))]
FRONT = [("front target", 512, 80, 160, 48, 160, 320), ("front source", 512, 90, 160, 48, 180, 320)]


def verdict(j, s):
    """the joint side's times against the separate side's: the rule of the module docstring"""
    if med(s) - med(j) > s[-1] - s[0]:
        return "wins"
    if med(j) - med(s) > j[-1] - j[0]:
        return "LOSES"
    return "no difference"


def operands(shape, C, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    g = torch.randn(shape, device=dev, generator=gen)
    w = torch.randn((C, 1, 3, 3), device=dev, generator=gen)
    scale = 0.25 + 1.5 * torch.rand(C, device=dev, generator=gen)
    shift = 0.4 * torch.randn(C, device=dev, generator=gen)
    return gen, g, w, scale, shift


def time_plain(dev, say, B, C, H, W, d, n, repeats):
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    shape = (B, C, H, W)
    gen, g, w, scale, shift = operands(shape, C, dev, d)
    x = torch.randn(shape, device=dev, generator=gen)
    y = torch.empty_like(x)
    _lib.check(L.halo_dwconv3x3_affine_relu_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, C, H, W, d, st))
    need = L.halo_dwconv_workspace_bytes(B, C, H, W, d)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    out = {k: (torch.empty_like(x), torch.empty_like(w)) for k in ("joint", "separate")}
    P = _lib.ptr

    def joint():
        gx, gw = out["joint"]
        _lib.check(L.halo_joint_dwconv3x3_affine_relu_bwd(P(g), P(y), P(x), P(w), P(scale), P(gx), P(gw), B, C, H, W, d, P(ws), need, st))

    def separate():
        gx, gw = out["separate"]
        _lib.check(L.halo_dwconv3x3_affine_relu_bwd_data(P(g), P(y), P(w), P(scale), P(gx), B, C, H, W, d, st))
        _lib.check(L.halo_dwconv3x3_affine_relu_bwd_weight(P(g), P(y), P(x), P(scale), P(gw), B, C, H, W, d, P(ws), need, st))
    j, s = windows([joint, separate], n, repeats)
    same = all(torch.equal(a, b) for a, b in zip(out["joint"], out["separate"]))
    nbytes = x.numel() * 4
    say("    %-20s d = %-2d  joint %s   separate %s   separate/joint (medians) x%.3f   separate's spread %.4f   joint %s   same bits: %s   "
        "joint: %.2f TB/s of its four transfers (%.0f MB each)"
        % ("x".join(map(str, shape)), d, fmt(j), fmt(s), med(s) / med(j), s[-1] - s[0], verdict(j, s), same, 4 * nbytes / (med(j) * 1e-3) / 1e12,
           nbytes / 1e6))
    return verdict(j, s)


def time_front(dev, say, B, Ca, h, wi, Cs, H, W, n, repeats):
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    C = Ca + Cs
    gen, g, w, scale, shift = operands((B, C, H, W), C, dev, h)
    a = torch.randn((B, Ca, h, wi), device=dev, generator=gen)
    s_ = torch.randn((B, Cs, H, W), device=dev, generator=gen)
    y = torch.empty((B, C, H, W), device=dev)
    P = _lib.ptr
    _lib.check(L.halo_upcat_dwconv3x3_affine_relu_fwd(P(a), P(s_), P(w), P(scale), P(shift), P(y), B, Ca, Cs, h, wi, H, W, st))
    need = L.halo_dwconv_workspace_bytes(B, C, H, W, 1)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    out = {k: (torch.empty((B, Ca, H, W), device=dev), torch.empty_like(s_), torch.empty_like(w)) for k in ("joint", "separate")}

    def joint():
        gup, gs, gw = out["joint"]
        _lib.check(L.halo_joint_upcat_dwconv3x3_affine_relu_bwd(P(g), P(y), P(a), P(s_), P(w), P(scale), P(gup), P(gs), P(gw), B, Ca, Cs, h, wi,
                                                                H, W, P(ws), need, st))

    def separate():
        gup, gs, gw = out["separate"]
        _lib.check(L.halo_upcat_dwconv3x3_affine_relu_bwd_data(P(g), P(y), P(w), P(scale), P(gup), P(gs), B, Ca, Cs, H, W, st))
        _lib.check(L.halo_upcat_dwconv3x3_affine_relu_bwd_weight(P(g), P(y), P(a), P(s_), P(scale), P(gw), B, Ca, Cs, h, wi, H, W, P(ws), need,
                                                                 st))
    j, s = windows([joint, separate], n, repeats)
    same = all(torch.equal(p, q) for p, q in zip(out["joint"], out["separate"]))
    say("    a %s  s %s   joint %s   separate %s   separate/joint (medians) x%.3f   separate's spread %.4f   joint %s   same bits: %s"
        % ("x".join(map(str, a.shape)), "x".join(map(str, s_.shape)), fmt(j), fmt(s), med(s) / med(j), s[-1] - s[0], verdict(j, s), same))
    return verdict(j, s)


def time_heads(dev, say, n, repeats, label):
    """tools/time_euclid_head.py's head, forward + backward: block and head classes marked by use_joint_depthwise_backward against
    the same classes unmarked"""
    from halo_amd import hooks
    from tools.time_euclid_head import CROPS, Block, Head
    heads = {}
    for tag in ("marked", "unmarked"):
        blk = hooks.use_fused_depthwise(type("Block_" + tag, (Block,), {}))
        cls = hooks.use_v3plus_forward(type("Head_" + tag, (Head,), {}))
        hooks.use_device_resize(cls), hooks.use_fused_decoder_front(cls)
        if tag == "marked":
            hooks.use_joint_depthwise_backward(blk), hooks.use_joint_depthwise_backward(cls)
        heads[tag] = cls(blk).to(dev).train()
    heads["marked"].load_state_dict(heads["unmarked"].state_dict())
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
        before = dict(dwconv.joint_launches)
        sides["marked"]()
        ran = {k: dwconv.joint_launches[k] - before[k] for k in before}
        m, u = windows([sides["marked"], sides["unmarked"]], n, repeats)
        say("head, %s, %s: top 2x2048x%dx%d, low 2x256x%dx%d, forward + backward   (joint passes of one marked step: %s)"
            % (label, where, h, w, H, W, ran))
        say("    marked %s   unmarked %s   unmarked - marked (medians) %.3f ms   x%.3f   unmarked's spread %.4f   marked %s"
            % (fmt(m), fmt(u), med(u) - med(m), med(u) / med(m), u[-1] - u[0], verdict(m, u)))
        del sides, feats, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--head", action="store_true", help="also time the stand-in head, marked against unmarked")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_joint_depthwise.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s   process %d" % (torch.cuda.get_device_name(0), os.getpid()))
    say("per-call ms over %d windows of %d calls: best / median / worst; backward for x and w alone" % (args.repeats, args.n))
    for name, C, H, W, dil in PLAIN:
        say("%s" % name)
        for B in (2, 1):
            for d in dil:
                time_plain(dev, say, B, C, H, W, d, args.n, args.repeats)
                torch.cuda.empty_cache()
    for name, Ca, h, wi, Cs, H, W in FRONT:
        say("%s" % name)
        for B in (2, 1):
            time_front(dev, say, B, Ca, h, wi, Cs, H, W, args.n, args.repeats)
            torch.cuda.empty_cache()
    if args.head:
        rule = dwconv.JOINT_MIN_ELEMENTS
        time_heads(dev, say, 3, 5, "the served rule %s" % (rule,))
        dwconv.JOINT_MIN_ELEMENTS = {k: 0 for k in rule}
        try:
            time_heads(dev, say, 3, 5, "the rule switched off")
        finally:
            dwconv.JOINT_MIN_ELEMENTS = rule
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
