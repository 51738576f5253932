"""Timing aid: the scorer at wide acquisition windows (size = 2 RADIUS_K + 1; the module's default is 33), 1024 x 2048, 19 classes.

One invocation is one process and measures, for k in {5, 9, 17, 33}:

    score_maps(("entropy", "ripu"), size=k) at B = 1 and B = 4, with and without normalize      (box sum + window histogram + tail)
    FloatingRegionScore(size=k).compute_region_uncertainty("entropy", ...)                       (pixel entropy + box sum)
    FloatingRegionScore(size=k).compute_region_impurity(pred, 19)                                (window histogram, int64 labels)

on seeded inputs made on the device: logits that are constant over 32 x 32 blocks plus noise, so that a window holds a few
classes, as a network's prediction does.  HIP events around n calls after a warm-up call of the closure (which also sizes n, so
that a window lasts about 60 ms whatever the kernels' speed); `repeats` windows per figure, printed best / median / worst in ms per
call.  The figures depend on nothing the package added with the tiled kernels, so the same file measures an older commit (run it
there with the same arguments).  `--json` keeps the windows; with two such files of the older commit and two of this one,

    python tools/time_wide_windows.py --compare OLD_A.json OLD_B.json NEW_A.json NEW_B.json [--out profiles/r27_time_wide_windows.txt]

prints the table and applies the project's speed rule to every figure: the new side WINS when its median is below the old side's
in both processes by more than the old side's own best-to-worst spread over all its windows.  No hardware counters are read.

    python tools/time_wide_windows.py --label new --json a.json [--sizes 5 9 17 33] [--repeats 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, O = 1024, 2048, 19


def windows(fn, repeats, budget_ms=60.0, nmax=500):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                              # first launch: code objects, workspaces
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    n = max(1, min(nmax, int(budget_ms / max(a.elapsed_time(b), 1e-3))))
    out = []
    for _ in range(repeats):
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / n)
    return sorted(out), n


def measure(args):
    import torch
    from halo_amd.core.active import floating_region as fr
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_wide_windows.py needs a ROCm device")
    dev = torch.device("cuda:0")
    lines, figures = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s   label: %s" % (torch.cuda.get_device_name(0), args.label))
    say("%d x %d, %d classes; per-call ms over %d windows: best / median / worst (calls per window)" % (H, W, O, args.repeats))
    gen = torch.Generator(device=dev).manual_seed(0)
    coarse = torch.randn((4, O, H // 32, W // 32), device=dev, generator=gen) * 3
    logit = coarse.repeat_interleave(32, dim=2).repeat_interleave(32, dim=3) + 0.7 * torch.randn((4, O, H, W), device=dev, generator=gen)
    logit = logit.contiguous()
    prob = torch.softmax(logit[0], dim=0).contiguous()
    pred = prob.argmax(dim=0).contiguous()
    route = getattr(fr, "window_route", None)
    for k in args.sizes:
        if route is not None:
            say("k = %d   routes: box %s, hist %s" % (k, route("box", k, "zeros", O, (H, W)), route("hist", k, "zeros", O, (H, W))))
        else:
            say("k = %d" % k)
        frs = fr.FloatingRegionScore(in_channels=O, size=k, purity_type="ripu")
        cases = []
        for B in (1, 4):
            for norm in (False, True):
                cases.append(("score_maps B=%d %s" % (B, "normalize" if norm else "raw"),
                              lambda B=B, norm=norm: fr.score_maps(logit[:B], None, "entropy", "ripu", norm, None, size=k)))
        cases.append(("compute_region_uncertainty", lambda: frs.compute_region_uncertainty("entropy", logit[0], prob)))
        cases.append(("compute_region_impurity", lambda: frs.compute_region_impurity(pred, O)))
        for name, fn in cases:
            with torch.no_grad():
                t, n = windows(fn, args.repeats)
            figures["k=%d %s" % (k, name)] = t
            say("  %-34s %9.4f / %9.4f / %9.4f   (%d)" % (name, t[0], t[len(t) // 2], t[-1], n))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"label": args.label, "device": torch.cuda.get_device_name(0), "figures": figures}, f, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def compare(args):
    old = [json.load(open(p)) for p in args.compare[:2]]
    new = [json.load(open(p)) for p in args.compare[2:]]
    lines = ["%s (old) against %s (new) on %s, %d x %d, %d classes, two processes each; ms per call, median of each process" %
             (old[0]["label"], new[0]["label"], new[0]["device"], H, W, O),
             "spread = the old side's worst - best window over both processes; WIN = new median below old median - spread in both processes",
             "%-44s %12s %12s %10s %12s %12s %8s  %s" % ("figure", "old A", "old B", "spread", "new A", "new B", "old/new", "rule")]
    lost = []
    for key in old[0]["figures"]:
        o = [r["figures"][key] for r in old]
        n = [r["figures"][key] for r in new]
        med = lambda t: t[len(t) // 2]                                      # noqa: E731
        spread = max(max(t) for t in o) - min(min(t) for t in o)
        win = all(med(n[p]) < med(o[p]) - spread for p in range(2))
        if not win:
            lost.append(key)
        ratio = (med(o[0]) + med(o[1])) / (med(n[0]) + med(n[1]))
        lines.append("%-44s %12.4f %12.4f %10.4f %12.4f %12.4f %8.1f  %s" % (key, med(o[0]), med(o[1]), spread, med(n[0]), med(n[1]), ratio,
                                                                             "WIN" if win else "no win"))
    lines.append("figures without a win: %s" % (", ".join(lost) if lost else "none"))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--sizes", type=int, nargs="+", default=[5, 9, 17, 33])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None, help="keep every window's time in this file")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--compare", nargs=4, default=None, metavar="JSON", help="two files of the old commit, two of the new one")
    args = ap.parse_args()
    if args.compare:
        compare(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
