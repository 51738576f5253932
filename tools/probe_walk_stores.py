"""Does the cache policy of the plane walk's 16-byte result store decide whether the walk sees the slow HBM stretches?

    python tools/probe_walk_stores.py [--gib 96] [--repeats 6] [--out profiles/r26_walk_store_modes.txt]

One process, one buffer.  Per 16 GiB window the walk of halo_hbm_walk_probe_ex (C = 256 planes of 16 MiB, the bench's float64 shape)
runs with every store mode of tools/halo_probe.STORE_MODES, interleaved, the mode order rotated per repeat; then the skews
(where chunk o's result lands in the result plane) for the plain store and for the best mode.  Prints TB/s per window and mode,
the plain store's own spread per window, and which mode wins by the rule:

    on EVERY window the mode's median rate exceeds the plain store's by more than the plain store's spread (max - min) there, AND
    on the slow windows (plain below the midpoint of plain's fastest and slowest window; every window when they differ by less
    than 2 %) it recovers at least half of (no store - plain).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import halo_probe  # noqa: E402

PLANES, PLANE_BYTES = 256, 16 << 20
WINDOW = 16 << 30
SKEWS = (0, 4 << 10, 1 << 20, 8 << 20)


def time_walk(buf, off, out, mode, skew, launches):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    halo_probe.walk_probe_ex(buf, WINDOW, PLANE_BYTES, PLANES, out, mode, skew, off)      # warm-up, not timed
    ev[0].record()
    for _ in range(launches):
        halo_probe.walk_probe_ex(buf, WINDOW, PLANE_BYTES, PLANES, out, mode, skew, off)
    ev[1].record()
    torch.cuda.synchronize()
    return WINDOW * launches / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r26_walk_store_modes.txt"))
    a = ap.parse_args()
    assert a.gib >= 64 and a.gib % 16 == 0 and a.repeats >= 5
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    nwin = a.gib // 16
    buf = torch.empty(a.gib << 27, dtype=torch.float64, device=dev)
    seed = (torch.randn(1 << 27, dtype=torch.float64, device=dev) * 0.05)
    for i in range(a.gib):
        buf[i << 27:(i + 1) << 27].copy_(seed)
    del seed
    out = torch.empty(WINDOW // PLANES // 8, dtype=torch.float64, device=dev)
    modes = list(range(len(halo_probe.STORE_MODES)))
    say("# %s, %d GiB buffer in one allocation, %d windows of 16 GiB, %d planes of %d MiB per group, %d repeats of %d launches"
        % (torch.cuda.get_device_name(dev), a.gib, nwin, PLANES, PLANE_BYTES >> 20, a.repeats, a.launches))

    # every storing mode writes what the plain store writes (window 0, skews 0 and 4 KiB)
    for skew in (0, 4 << 10):
        want = None
        for m in modes[1:]:
            out.fill_(-1.0)
            halo_probe.walk_probe_ex(buf, WINDOW, PLANE_BYTES, PLANES, out, m, skew, 0)
            torch.cuda.synchronize()
            if want is None:
                want = out.clone()
                assert bool((want >= 0).all())
            else:                                          # mode 5: a chunk's 128 first sums, then its 128 second sums
                got = out if m != 5 else out.view(-1, 2, 128).transpose(1, 2).reshape(-1)
                assert torch.equal(got, want), "store mode %d writes other bytes than the plain store (skew %d)" % (m, skew)
    out.fill_(-1.0)
    halo_probe.walk_probe_ex(buf, WINDOW, PLANE_BYTES, PLANES, out, 0, 0, 0)
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()), "mode 0 stored"
    say("# all storing modes write the plain store's bytes; mode 0 writes nothing")

    rate = {}                                              # (window, mode) -> [TB/s per repeat]
    for w in range(nwin):
        for r in range(a.repeats):
            order = modes[r % len(modes):] + modes[:r % len(modes)]
            for m in order:
                rate.setdefault((w, m), []).append(time_walk(buf, w * WINDOW, out, m, 0, a.launches))
    med = {k: statistics.median(v) for k, v in rate.items()}
    spread = {w: max(rate[(w, 1)]) - min(rate[(w, 1)]) for w in range(nwin)}
    say()
    say("TB/s (median of %d) per 16 GiB window and store mode; 'spread' = max - min of the plain store on that window" % a.repeats)
    say("window  " + "  ".join("%10s" % n for n in halo_probe.STORE_MODES) + "      spread")
    for w in range(nwin):
        say("%6d  " % w + "  ".join("%10.3f" % med[(w, m)] for m in modes) + "  %10.3f" % spread[w])
    say("min/max " + "  ".join("%4.2f/%4.2f " % (min(min(rate[(w, m)]) for w in range(nwin)), max(max(rate[(w, m)]) for w in range(nwin)))
                               for m in modes))

    plain = [med[(w, 1)] for w in range(nwin)]
    lo, hi = min(plain), max(plain)
    slow = [w for w in range(nwin) if plain[w] < (lo + hi) / 2] if hi > 1.02 * lo else list(range(nwin))
    say()
    say("slow windows (plain store): %s" % (slow if hi > 1.02 * lo else "none stands out (plain differs by %.1f %% across windows): all windows taken" % (100 * (hi / lo - 1))))
    winners = []
    for m in modes[2:]:
        above = all(med[(w, m)] - med[(w, 1)] > spread[w] for w in range(nwin))
        half = all(med[(w, m)] - med[(w, 1)] >= 0.5 * (med[(w, 0)] - med[(w, 1)]) for w in slow)
        rec = [(med[(w, m)] - med[(w, 1)]) / (med[(w, 0)] - med[(w, 1)]) if med[(w, 0)] > med[(w, 1)] else float("nan") for w in range(nwin)]
        say("mode %d %-11s above plain by more than its spread on every window: %-5s  recovers >= half of (none - plain) on the slow ones: %-5s"
            "  recovered share per window: %s" % (m, halo_probe.STORE_MODES[m], above, half, " ".join("%5.2f" % x for x in rec)))
        if above and half:
            winners.append(m)
    best = max(modes[2:], key=lambda m: sum(med[(w, m)] for w in range(nwin)))
    say("winner by the rule: %s" % (", ".join("%d (%s)" % (m, halo_probe.STORE_MODES[m]) for m in winners) if winners else "NONE"))
    say("best storing mode by mean rate: %d (%s)" % (best, halo_probe.STORE_MODES[best]))

    say()
    say("skew of the result inside its plane, TB/s (median of %d) per window: plain store, then mode %d (%s)" % (a.repeats, best, halo_probe.STORE_MODES[best]))
    say("window  " + "  ".join("%12s" % ("plain+%dK" % (s >> 10)) for s in SKEWS) + "  " + "  ".join("%12s" % ("m%d+%dK" % (best, s >> 10)) for s in SKEWS))
    combos = [(1, s) for s in SKEWS] + [(best, s) for s in SKEWS]
    skew_w = {}
    for w in range(nwin):
        got = {}
        for r in range(a.repeats):
            for m, s in combos[r % len(combos):] + combos[:r % len(combos)]:
                got.setdefault((m, s), []).append(time_walk(buf, w * WINDOW, out, m, s, a.launches))
        skew_w[w] = got
        say("%6d  " % w + "  ".join("%12.3f" % statistics.median(got[c]) for c in combos))
    for m in (1, best):
        base = [statistics.median(skew_w[w][(m, 0)]) for w in range(nwin)]
        for s in SKEWS[1:]:
            d = [statistics.median(skew_w[w][(m, s)]) - base[w] for w in range(nwin)]
            sp = [max(skew_w[w][(m, 0)]) - min(skew_w[w][(m, 0)]) for w in range(nwin)]
            say("mode %d skew %5d KiB: above skew 0 by more than its spread on every window: %s" % (m, s >> 10, all(x > y for x, y in zip(d, sp))))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
