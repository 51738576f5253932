"""The shapes at which halo_hfr.hip's work split has an edge, each the smallest that reaches it, the operand recipe they share, and
the yardstick the device is held to (hfr_ref.py states the reference, the admissibility conditions and the groups).

The split, by constant of halo_hfr.hip (test_hfr_ref_host.py reads them from the source and compares):
    HT = 256        pixels per tile: nblk = ceil(P / HT) tiles per image, the last one with tail = P - (nblk - 1) HT pixels
                    (k_hfr_stats, k_hfr_apply, k_hfr_bwd_out, k_hfr_bwd_out_generic; k_hfr_stats_merge's r % nblk tile size and its
                    r += HT loop over R = B nblk part rows; k_hfr_bwd_small's i += HT loops over B C)
    HSEG = 16       k_hfr_colsum cuts R rows (nblk per image in the forward, B nblk in the backward) at R seg / HSEG
    HDOT = 8        k_hfr_dot cuts a plane at P sp / HDOT
    4 HT = 1024     elements of a plane per blockIdx.y of k_hfr_scale
    HCW = 8         channels per LDS chunk of the generic arm's sums; H_MAX_C = 256 the widest served; C = 64 the register arm

Operands.  From one seed per case: a default-initialised wn_mlp, x = 0.7 N(0, 1) + 0.1, g = N(0, 1), running_mean = N(0, 0.3) and
running_var = U(0.5, 1.5) as tests/test_gpu_hfr.py perturbs them, and, so that a wrong channel index shows, gamma = U(0.5, 1.5)
with one negative entry and beta = N(0, 0.2) instead of ones and zeros.  Two channels are clamped by b2 = -10 (the first chunk and
the last channel); the others get b2 + 1.5: with the default bias alone W2 mr + b2 is a signed sum around zero, about half the
channels clamp by luck and condition 3 of hfr_ref.py cannot hold.  One channel of x is all zero in the last image.  Every image's
last tile is the partial one, so the zero plane and the clamped channel C - 1 sit in it.

Knife edges.  Condition 1 allows no |z| within 4 tau of zero.  A case has up to 4.3 M values of z with a density near 0.4 at zero
and 4 tau near 1e-4: a seed without any such value does not exist at that size (hundreds are expected), and drawing a pixel again
moves the batch statistics by far more than tau, which only brings other values to the edge.  So the recipe nudges: a pixel whose
z_k lies within 8 tau in any of the case's modes moves along W1's row k by the least change of x that takes z_k another 16 tau
away from zero (about 1e-4 in x; the batch statistics move by that over N, far below tau), until no mode has such a value (two
or three rounds).  The margin of 8 against the asserted 4 keeps the outcome the same wherever float64 sums round differently.
Conditions 2 and 3 are per (image, channel) and are met by the choice of seed (find_seed), as is the float32 stock chain's
agreement on every bit.
"""
import functools

import numpy as np
import torch
import torch.nn as nn

import hfr_ref

HT, HCW, HSEG, HDOT, H_MAX_C = 256, 8, 16, 8, 256
SCALE_CHUNK = 4 * HT
ALL_MODES = tuple(hfr_ref.MODES)
TWO_MODES = ("train", "eval")

# name: (B, C, h, w), modes, the edge, what the split is at that shape
CASES = {
    "c64_p257": ((2, 64, 1, 257), ALL_MODES, "one-pixel tail, two tiles, register arm", dict(nblk=2, tail=1)),
    "c64_p511": ((2, 64, 7, 73), TWO_MODES, "255-pixel tail", dict(nblk=2, tail=255)),
    "c64_p768": ((2, 64, 24, 32), TWO_MODES, "exact multiple of HT, the control", dict(nblk=3, tail=256)),
    "c64_p1025": ((2, 64, 25, 41), ALL_MODES, "k_hfr_scale's second y-block holds one element; nblk < HSEG: empty segments",
                  dict(nblk=5, tail=1, scale_blocks=2, last_chunk=1)),
    "c64_p4252_b1": ((1, 64, 4, 1063), TWO_MODES, "nblk = HSEG + 1: uneven segments; B = 1", dict(nblk=17, tail=156, R=17)),
    "c64_p7_b3": ((3, 64, 1, 7), TWO_MODES, "P < HDOT: empty k_hfr_dot splits", dict(nblk=1, tail=7, empty_splits=1)),
    "c64_p1_b3": ((3, 64, 1, 1), TWO_MODES, "P = 1", dict(nblk=1, tail=1, empty_splits=7)),
    "c64_p2043_b33": ((33, 64, 9, 227), TWO_MODES,
                      "more than HT part rows in k_hfr_stats_merge, B C > HT in k_hfr_bwd_small, B > HSEG", dict(nblk=8, tail=251, R=264)),
    "c10_p257": ((2, 10, 1, 257), ALL_MODES, "generic arm, C no multiple of HCW", dict(nblk=2, tail=1)),
    "c3_p1025": ((2, 3, 25, 41), TWO_MODES, "generic arm, C < HCW, five tiles", dict(nblk=5, tail=1, scale_blocks=2, last_chunk=1)),
    "c72_p511": ((2, 72, 7, 73), TWO_MODES, "generic arm above 64, a multiple of HCW", dict(nblk=2, tail=255)),
    "c256_p300": ((2, 256, 12, 25), TWO_MODES, "generic arm at H_MAX_C", dict(nblk=2, tail=44)),
    # the rank route's second case: two ranks of two images each
    "c10_p257_b4": ((4, 10, 1, 257), ("train",), "generic arm, two images per rank", dict(nblk=2, tail=1)),
}
# the first seed from 1 at which every mode of the case meets conditions 2 and 3 and the float32 stock chain agrees on every ReLU
# and clamp bit (find_seed; run on the CPU)
SEEDS = {
    "c64_p257": 1, "c64_p511": 1, "c64_p768": 1, "c64_p1025": 1, "c64_p4252_b1": 1, "c64_p7_b3": 1, "c64_p1_b3": 5,
    "c64_p2043_b33": 1, "c10_p257": 1, "c3_p1025": 1, "c72_p511": 1, "c256_p300": 1, "c10_p257_b4": 1,
}
NUM_BATCHES_TRACKED = 3
REPAIR_MARGIN = 8.0


def case_modes():
    return [(n, m) for n in CASES for m in CASES[n][1]]


def split_facts(B, C, P):
    cdiv = lambda a, b: -(-a // b)
    nblk = cdiv(P, HT)
    bounds = [P * s // HDOT for s in range(HDOT + 1)]
    return dict(nblk=nblk, tail=P - (nblk - 1) * HT, R=B * nblk, scale_blocks=cdiv(P, SCALE_CHUNK),
                last_chunk=P - (cdiv(P, SCALE_CHUNK) - 1) * SCALE_CHUNK, empty_splits=sum(a == b for a, b in zip(bounds, bounds[1:])),
                empty_segments_fwd=sum(nblk * s // HSEG == nblk * (s + 1) // HSEG for s in range(HSEG)),
                arm="register" if C == 64 else "generic")


def marked(C, B):
    """(the clamped channels, the all-zero plane (image, channel))"""
    return ((1, C - 1), (B - 1, C - 2)) if C > 3 else ((0, 2), (B - 1, 1))


def draw(name, seed):
    (B, C, h, w), modes = CASES[name][0], CASES[name][1]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        mlp = nn.Sequential(nn.Linear(C, C), nn.BatchNorm1d(C), nn.ReLU(), nn.Linear(C, C))
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=gen) * 0.7 + 0.1
    g = torch.randn(B, C, h, w, generator=gen)
    running_mean = torch.randn(C, generator=gen) * 0.3
    running_var = torch.rand(C, generator=gen) + 0.5
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.2
    clamped, (zb, zc) = marked(C, B)
    if C > 3:
        gamma[2] = -0.75
    b2 = mlp[3].bias.detach().clone() + 1.5
    b2[list(clamped)] = -10.0
    x[zb, zc] = 0.0
    f32 = lambda t: t.detach().numpy().astype(np.float32).copy()
    case = dict(x=f32(x), g=f32(g), W1=f32(mlp[0].weight), b1=f32(mlp[0].bias), W2=f32(mlp[3].weight), b2=f32(b2), gamma=f32(gamma),
                beta=f32(beta), running_mean=f32(running_mean), running_var=f32(running_var), eps=mlp[1].eps,
                num_batches_tracked=NUM_BATCHES_TRACKED, clamped=clamped, zero=(zb, zc), name=name, seed=seed, nudged=0)
    W1 = case["W1"].astype(np.float64)
    for _ in range(20):
        moved = 0
        for m in modes:
            for r, k, dh in zip(*hfr_ref.knife_edges(case, m, REPAIR_MARGIN)):
                b, p = int(r) // (h * w), int(r) % (h * w)
                d = W1[k].copy()
                if b == zb:
                    d[zc] = 0.0                                                # the all-zero plane stays all zero
                col = case["x"][b, :, p // w, p % w]
                col += (dh * d / (d @ d)).astype(np.float32)
                moved += 1
        case["nudged"] += moved
        if not moved:
            break
    else:
        raise AssertionError("%s: values of z within %g tau of zero after 20 rounds" % (name, REPAIR_MARGIN))
    return case


@functools.lru_cache(maxsize=None)
def build(name):
    return draw(name, SEEDS[name])


SMALL = ("y", "g_x", "g_W1", "g_b1", "g_gamma", "g_beta", "g_W2", "g_b2", "running_mean", "running_var", "var", "row_W1", "row_W2",
         "zero_planes", "batch_stats", "B", "C", "P", "w", "wc", "mr", "allow_g_x")


def evaluate(case, mode):
    """(the reference without its per-pixel intermediates, its admissibility, the stock float32 chain's rho per tensor, the number
    of ReLU and clamp bits on which that chain differs from float64)"""
    from halo_amd.hfr import torch_statement
    ref = hfr_ref.reference(case, mode)
    adm = hfr_ref.admissibility(ref, case)
    stock, _, bits = hfr_ref.run_statement(torch_statement, case, mode)
    relu64, clamp64 = hfr_ref.masks(ref)
    differ = (int((bits[0] != relu64).sum()), int((bits[1] != clamp64).sum()))
    return {k: ref[k] for k in SMALL if k in ref}, adm, hfr_ref.rho(ref, stock), differ


@functools.lru_cache(maxsize=None)
def held(name, mode):
    return evaluate(build(name), mode)


@functools.lru_cache(maxsize=None)
def yardstick():
    """{tensor: (rho*, where)}: the float32 stock chain's worst group over every case and mode"""
    best = {}
    for name, mode in case_modes():
        for T, (r, where) in held(name, mode)[2].items():
            if T not in best or r > best[T][0]:
                best[T] = (r, "%s %s %s" % (name, mode, where))
    return best


def find_seed(name, first=1, last=200):
    """the first seed at which `name` is admissible in all its modes and the stock chain agrees on every bit"""
    for seed in range(first, last):
        case = draw(name, seed)
        ok = True
        for mode in CASES[name][1]:
            _, adm, _, differ = evaluate(case, mode)
            if len(adm["relu"]) or len(adm["clamp"]) or len(adm["cond"]) or any(differ):
                ok = False
                break
        if ok:
            return seed
    raise AssertionError("no admissible seed for %s in [%d, %d)" % (name, first, last))


if __name__ == "__main__":                                                     # PYTHONPATH=<repository root> python tests/hfr_cases.py
    for n in CASES:
        print('"%s": %d,' % (n, find_seed(n)))
