"""Timing aid: the exact low-res embedding pass ALONE (the scorer's own ev_feat_start / ev_feat_stop events), one shape per
kernel that launch_feat_lr can choose, B images to 1024 x 2048.  Median of --calls calls after --warmup; one JSON line per route.
A/B of two builds: run it once per library (HALO_LIB_PATH) in fresh processes, alternating, and compare the medians.
    python tools/time_lowres_routes.py [--batch 16] [--calls 25] [--warmup 5] [--routes 8px_x6.4,regs_f32]"""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from halo_amd import _lib
from halo_amd.core.active.floating_region import score_maps_lowres

# route: (C, (hf, wf), dtype, embedding offset in elements) -- the kernel each takes follows launch_feat_lr's tests
ROUTES = {"8px_x6.4": (64, (160, 320), torch.float64, 0),       # k_feat_reduce_lr_dmaf<., 8, 8, 8>: the real v3+ head
          "8px_x4": (256, (256, 512), torch.float64, 0),        # k_feat_reduce_lr_dmaf<., 11, 10, 8>: tools/prof_lowres.py's shape
          "4px": (19, (160, 640), torch.float64, 0),            # k_feat_reduce_lr_dmaf<., 8, 12, 4>: 12 pairs per row, past the 8-pixel geometries
          "dma_runtime": (64, (512, 1024), torch.float64, 0),   # k_feat_reduce_lr_dma: x2, taller windows than any fixed geometry
          "regs_offset": (256, (256, 512), torch.float64, 1),   # k_feat_reduce_lr<double>: off 16-byte alignment
          "regs_f32": (256, (256, 512), torch.float32, 0)}      # k_feat_reduce_lr<float>
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--calls", type=int, default=25); ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--routes", default=",".join(ROUTES)); ap.add_argument("--pur", default="radius", choices=("radius", "euc_norm"))
a = ap.parse_args()
dev, L, B = torch.device("cuda:0"), _lib.lib(), a.batch
lg = torch.randn((B, 19, 160, 320), device=dev)
for name in a.routes.split(","):
    C, (hf, wf), dt, off = ROUTES[name]
    buf = torch.empty(B * C * hf * wf + off, dtype=dt, device=dev)
    em = buf[off:].view(B, C, hf, wf)
    em.copy_(torch.randn((1, C, hf, wf), device=dev, dtype=dt) * 0.05)
    ev = tuple(L.halo_event_create() for _ in range(4))
    ms = []
    for i in range(a.warmup + a.calls):
        score_maps_lowres(lg, em, (1024, 2048), "entropy", a.pur, True, None, ksize=3, want_maps=False, mode="exact", events=ev)
        torch.cuda.synchronize(dev)
        v = ctypes.c_float()
        assert L.halo_event_elapsed_ms(ev[2], ev[3], ctypes.byref(v)) == 0
        if i >= a.warmup: ms.append(v.value)
    for e in ev: L.halo_event_destroy(e)
    del em, buf
    print(json.dumps({"route": name, "lib": os.environ.get("HALO_LIB_PATH", "in-tree"), "B": B, "calls": a.calls,
                      "feat_ms_median": round(statistics.median(ms), 4), "feat_ms_min": round(min(ms), 4), "feat_ms_max": round(max(ms), 4)}), flush=True)
