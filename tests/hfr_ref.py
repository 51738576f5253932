"""HFR's weighted normalisation (halo_amd.hfr.torch_statement) stated once in float64 on the CPU, the admissibility conditions of a
test case, and the group-by-group comparison the HFR route tests hold every result to.

The statement.  x (B, C, h, w), P = h w, N = B P rows X = x.permute(0, 2, 3, 1).reshape(N, C):

    h = X W1^T + b1      (mean, var) = the rows' mean and biased variance, or the running statistics
    scale = gamma / sqrt(var + eps)      shift = beta - mean scale      z = h scale + shift      r = relu(z)
    mr_b = mean_p r      w_b = W2 mr_b + b2      wc = clamp(w, min=1e-5)      n_bc = ||x_bc||_2      y = x / max(n, 1e-12) * wc

`reference` evaluates it with torch's float64 operators in this order -- no tiles, no part rows, no per-(image, channel)
coefficients -- and takes every gradient of (y * g).sum() from float64 autograd, so torch's own subgradients (ReLU open where
z > 0, the clamp where w >= 1e-5, clamp_min(n, eps) where n >= eps) are the ones compared.  The running statistics follow
F.batch_norm's update: (1 - f) old + f new with the unbiased variance, f = momentum, or 1 / num_batches_tracked after the increment
when momentum is None.

Admissibility.  A float32 evaluation can only be held to float64 group by group where the two agree on every ReLU bit and every
clamp decision; an input on a knife edge makes a correct kernel and the reference differ by a whole term.  Three conditions, all
computed from float64 alone (u = 2^-24, C the width):

1. No ReLU knife edge: |z| > 4 tau at every (pixel, channel).  tau bounds the float32 error of z = fmaf(h, scale, shift), h a
   C-term fmaf chain from b1.  With Sh = |b1_k| + sum_j |W1_kj| |x_pj| (the chain's abs-sum) and Sz = |scale| Sh + |shift|:
     (a) the chain: each of its C roundings is relative to a partial sum bounded by Sh        |h32 - h| <= C u Sh
     (b) scale rounded to float32 (it is formed in float64 from float64 sums), times |h32| <= Sh        u |scale| Sh
     (c) shift rounded to float32                                                                       u |shift|
     (d) the fmaf's one rounding of a value bounded by Sz                                               u (|scale| Sh + |shift|)
   Sum: u ((C + 2) |scale| Sh + 2 |shift|), terms of order u^2 left to the factor 4.  The code uses the slightly larger
   tau = u ((C + 2) |scale| Sh + 2 Sz) of the issue that asked for these tests; the extra 2 u |scale| Sh is what the stock chain
   needs beyond the device (C + 1 roundings in a GEMM row plus bias, and BatchNorm's separate multiply and add).
2. No clamp knife edge: |w - 1e-5| > 4 dw at every (image, channel).  relu is 1-Lipschitz, so with no ReLU bit flipped the error of
   mr_bk is at most mean_p tau_pk (the device adds in float64; nothing else enters), and W2 carries it into w:
     dw = sum_k |W2_ck| mean_p tau_pk + (C + 2) u Sw,      Sw = |b2_c| + sum_k |W2_ck| mr_bk.
   The second term is u Sw for the device (w is formed in float64 and rounded once); (C + 2) u Sw also covers the stock chain's
   per-pixel float32 Linear, whose abs-sums average to Sw exactly because r >= 0.  This is larger than the issue's `u Sw`, on
   purpose: the stock chain is then covered by the same condition, which test_hfr_ref_host.py checks bit by bit.
3. No ill-conditioned unclamped weight: w >= Sw / 8 wherever w >= 1e-5, so the cancellation in W2 mr + b2 cannot make a plane of y
   small beside the error its terms carry (the yardstick below divides by max|y| of a plane).

The comparison.  rho(T, G) = max_{e in G} |got - want| / scale(T, G):
    y, g_x                        G = one (image, channel) plane, scale = max_G |want|; an all-zero channel of x is such a plane.
                                  g_x has two amendments, both from a finding on the device (NOTES.md, HFR testing): each
                                  element's error counts beyond 3 u (|g| e1 + |x| |e2|), the three float32 roundings (e1, e2,
                                  g e1) of the normalize branch g e1 + x e2, whose terms cancel where g is parallel to x; and at
                                  P = 1, where a plane is a single entry of the signed sum W1^T g_h, G = one image
    g_W1, g_W2                    G = one row, scale = max(max_G |want|, u * the row's abs-sum): max_j sum_p |g_h_pc| |x_pj|
                                  for g_W1, max_k sum_b |g_w_bc| mr_bk for g_W2
    g_b1, g_b2, g_gamma, g_beta   one group, scale = max |want|; under batch statistics g_b1 (zero up to rounding: the
                                  BatchNorm removes b1) is held to max |g_W1|
    running_mean                  per channel, scale = max(|want|, sqrt(var_c))
    running_var                   per channel, scale = |want|
A group whose scale is zero (y of an all-zero channel, g_W2's row of a clamped channel) must be exact: rho is 0 or inf there.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
CLAMP, NEPS = 1e-5, 1e-12
MODES = {
    # name: (training, momentum, affine, track_running_stats)
    "train": (True, 0.1, True, True),
    "train_cumulative": (True, None, True, True),
    "eval": (False, 0.1, True, True),
    "train_no_affine": (True, 0.1, False, True),
    "eval_no_tracking": (False, 0.1, True, False),
}
PARAMS = ("W1", "b1", "gamma", "beta", "W2", "b2")
TENSORS = ("y", "g_x", "g_W1", "g_b1", "g_gamma", "g_beta", "g_W2", "g_b2", "running_mean", "running_var")
FAULTS = ("stats_skip_last_pixel", "mean_r_skip_last_pixel", "tail_counts_over_full_tile", "coef_of_image0_for_image1",
          "g_W1_drops_last_part_row", "clamped_y_times_2", "g_W2_row40_zeroed")


def batch_stats(mode):
    training, _, _, track = MODES[mode]
    return training or not track


def updates(mode):
    training, _, _, track = MODES[mode]
    return training and track


def reference(case, mode, fault=None, tile=256):
    """every result and intermediate of the statement in float64 (numpy arrays in a dict).  `fault` names one deliberately wrong
    variant (FAULTS) for the rejection test: the same float64 evaluation with that one slip in it."""
    training, momentum, affine, track = MODES[mode]
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))
    x = t(case["x"]).requires_grad_(True)
    g = t(case["g"])
    W1, b1, W2, b2 = (t(case[k]).requires_grad_(True) for k in ("W1", "b1", "W2", "b2"))
    B, C, hh, ww = x.shape
    P, N, eps = hh * ww, B * hh * ww, float(case["eps"])
    gamma = t(case["gamma"]).requires_grad_(True) if affine else None
    beta = t(case["beta"]).requires_grad_(True) if affine else None
    X = x.permute(0, 2, 3, 1).reshape(N, C)
    h = F.linear(X, W1, b1)
    h.retain_grad()
    out = {}
    if batch_stats(mode):
        rows = h
        if fault == "stats_skip_last_pixel":
            rows = h.view(B, P, C)[:, :P - 1].reshape(-1, C)
        mean = rows.mean(0)
        var = ((rows - mean) ** 2).mean(0)
    else:
        mean, var = t(case["running_mean"]), t(case["running_var"])
    if updates(mode):
        f = momentum if momentum is not None else 1.0 / (int(case["num_batches_tracked"]) + 1)
        n_rows = rows.shape[0]
        out["running_mean"] = ((1 - f) * t(case["running_mean"]) + f * mean).detach().numpy()
        out["running_var"] = ((1 - f) * t(case["running_var"]) + f * var * n_rows / (n_rows - 1)).detach().numpy()
    scale = (gamma if affine else 1.0) / torch.sqrt(var + eps)
    shift = (beta if affine else 0.0) - mean * scale
    z = h * scale + shift
    r = torch.relu(z)
    mr = r.view(B, P, C).mean(1)
    if fault == "mean_r_skip_last_pixel":
        mr = r.view(B, P, C)[:, :P - 1].sum(1) / P
    mr.retain_grad()
    w = F.linear(mr, W2, b2)
    w.retain_grad()
    wc = w.clamp(min=CLAMP)
    y = F.normalize(x.reshape(B, C, P), dim=-1, eps=NEPS).reshape(B, C, hh, ww) * wc.view(B, C, 1, 1)
    (y * g).sum().backward()                                                   # also leaves h.grad, mr.grad, w.grad
    npy = lambda v: v.detach().numpy().copy()
    out.update(y=npy(y), g_x=npy(x.grad), g_W1=npy(W1.grad), g_b1=npy(b1.grad), g_W2=npy(W2.grad), g_b2=npy(b2.grad))
    if affine:
        out.update(g_gamma=npy(gamma.grad), g_beta=npy(beta.grad))
    xa = np.abs(np.asarray(case["x"], np.float64))
    Xa = xa.transpose(0, 2, 3, 1).reshape(N, C)
    g_h, g_w = npy(h.grad), npy(w.grad)
    nrm = np.sqrt((np.asarray(case["x"], np.float64).reshape(B, C, P) ** 2).sum(-1))
    sc, sf = npy(scale) * np.ones(C), npy(shift) * np.ones(C)
    Sh = np.abs(npy(b1))[None, :] + Xa @ np.abs(npy(W1)).T
    Sz = np.abs(sc)[None, :] * Sh + np.abs(sf)[None, :]
    Sw = np.abs(npy(b2))[None, :] + npy(mr) @ np.abs(npy(W2)).T
    out.update(h=npy(h), z=npy(z), mean=npy(mean), var=npy(var), scale=sc, shift=sf, mr=npy(mr), w=npy(w), wc=npy(wc), n=nrm,
               Sh=Sh, Sz=Sz, Sw=Sw, g_h=g_h, g_w=g_w, g_mr=npy(mr.grad),
               row_W1=np.max(np.abs(g_h).T @ Xa, axis=1), row_W2=np.max(np.abs(g_w).T @ npy(mr), axis=1),
               zero_planes=xa.reshape(B, C, P).max(-1) == 0, batch_stats=batch_stats(mode), B=B, C=C, P=P)
    # the normalize branch of g_x is g e1 + x e2, e1 = wc / nc, e2 = -[n >= eps] wc A / (nc^2 n), A = sum_p g x, nc = max(n, eps)
    nc, wc64 = np.maximum(nrm, NEPS), out["wc"]
    A = (np.asarray(case["g"], np.float64) * np.asarray(case["x"], np.float64)).reshape(B, C, P).sum(-1)
    e2 = np.where(nrm >= NEPS, wc64 * np.abs(A) / np.where(nrm >= NEPS, nc * nc * nrm, 1.0), 0.0)
    out["allow_g_x"] = 3.0 * U * (np.abs(np.asarray(case["g"], np.float64)) * (wc64 / nc)[:, :, None, None] + xa * e2[:, :, None, None])
    if fault in FAULTS[2:]:
        _late_fault(out, case, fault, tile)
    return out


def _late_fault(o, case, fault, tile):
    """the slips that sit behind the forward's sums: each is the correct float64 result plus what the slip adds, itself float64"""
    B, C, P = o["B"], o["C"], o["P"]
    x = np.asarray(case["x"], np.float64)
    X = x.transpose(0, 2, 3, 1).reshape(B, P, C)
    g = np.asarray(case["g"], np.float64)
    W1 = np.asarray(case["W1"], np.float64)
    open_ = (o["z"] > 0).reshape(B, P, C)
    a = o["scale"]                                                           # d z / d h
    if fault == "tail_counts_over_full_tile":
        # the pixels a tail tile does not have hold x = 0, so h = b1 and z = b1 scale + shift there; counting them adds
        # pad [z(b1) > 0] to #(z > 0) of every image, and with it g_r pad to sum g_z: g_h moves by -a d / N at every pixel
        assert o["batch_stats"]
        pad = (-P) % tile
        zb = np.asarray(case["b1"], np.float64) * o["scale"] + o["shift"]
        d = (o["g_mr"] / P * (pad * (zb > 0))[None, :]).sum(0)
        dgh = -a * d / (B * P)
        o["g_beta"] = o["g_beta"] + d
        o["g_b1"] = o["g_b1"] + dgh * (B * P)
        o["g_W1"] = o["g_W1"] + np.outer(dgh, X.sum((0, 1)))
        o["g_x"] = o["g_x"] + (dgh @ W1)[None, :, None, None]
    elif fault == "coef_of_image0_for_image1":
        # image 1 takes image 0's c1 = a g_r (the ReLU branch of g_h) and its e1 = wc / nc, e2 = -wc A / (nc^2 n)
        nc = np.maximum(o["n"], NEPS)
        A = (g.reshape(B, C, P) * x.reshape(B, C, P)).sum(-1)
        e1 = o["wc"] / nc
        e2 = np.where(o["n"] >= NEPS, -o["wc"] * A / np.where(o["n"] >= NEPS, nc * nc * o["n"], 1.0), 0.0)
        c1 = a[None, :] * o["g_mr"] / P
        dgh = open_[1] * (c1[0] - c1[1])[None, :]                             # (P, C)
        o["g_b1"] = o["g_b1"] + dgh.sum(0)
        o["g_W1"] = o["g_W1"] + dgh.T @ X[1]
        gx = o["g_x"].copy().reshape(B, C, P)
        gx[1] += (dgh @ W1).T + g.reshape(B, C, P)[1] * (e1[0] - e1[1])[:, None] + x.reshape(B, C, P)[1] * (e2[0] - e2[1])[:, None]
        o["g_x"] = gx.reshape(o["g_x"].shape)
    elif fault == "g_W1_drops_last_part_row":
        p0 = ((P - 1) // tile) * tile                                        # the last image's last tile
        gh = o["g_h"].reshape(B, P, C)[B - 1, p0:]
        o["g_W1"] = o["g_W1"] - gh.T @ X[B - 1, p0:]
    elif fault == "clamped_y_times_2":
        c = int(case["clamped"][0])
        o["y"] = o["y"].copy()
        o["y"][:, c] *= 2.0
    elif fault == "g_W2_row40_zeroed":
        o["g_W2"] = o["g_W2"].copy()
        o["g_W2"][40] = 0.0


def knife_edges(case, mode, margin):
    """condition 1 alone, forward only, for the case generator: (rows, channels, dh) of every |z| <= margin tau, dh the change of
    h that takes z to 2 margin tau further from zero on its own side"""
    training, _, affine, _ = MODES[mode]
    f8 = lambda k: np.asarray(case[k], np.float64)
    x = f8("x")
    B, C, hh, ww = x.shape
    X = x.transpose(0, 2, 3, 1).reshape(-1, C)
    h = X @ f8("W1").T + f8("b1")
    mean, var = (h.mean(0), h.var(0)) if batch_stats(mode) else (f8("running_mean"), f8("running_var"))
    scale = (f8("gamma") if affine else 1.0) / np.sqrt(var + float(case["eps"]))
    shift = (f8("beta") if affine else 0.0) - mean * scale
    Sh = np.abs(f8("b1"))[None, :] + np.abs(X) @ np.abs(f8("W1")).T
    t = U * ((C + 2) * np.abs(scale) * Sh + 2.0 * (np.abs(scale) * Sh + np.abs(shift)))
    z = h * scale + shift
    rows, chans = np.nonzero(np.abs(z) <= margin * t)
    side = np.where(z[rows, chans] >= 0, 1.0, -1.0)
    return rows, chans, side * 2.0 * margin * t[rows, chans] / (scale * np.ones(C))[chans]


def tau(ref):
    return U * ((ref["C"] + 2) * np.abs(ref["scale"])[None, :] * ref["Sh"] + 2.0 * ref["Sz"])


def admissibility(ref, case, margin=4.0):
    """the three conditions: dict of the violating index arrays (all empty for an admissible case) and the smallest margins seen"""
    B, C, P = ref["B"], ref["C"], ref["P"]
    t = tau(ref)
    relu_bad = np.argwhere(np.abs(ref["z"]) <= margin * t)                   # (row, channel)
    dw = t.reshape(B, P, C).mean(1) @ np.abs(np.asarray(case["W2"], np.float64)).T + (C + 2) * U * ref["Sw"]
    clamp_bad = np.argwhere(np.abs(ref["w"] - CLAMP) <= margin * dw)
    live = ref["w"] >= CLAMP
    cond_bad = np.argwhere(live & (ref["w"] < ref["Sw"] / 8.0))
    return dict(relu=relu_bad, clamp=clamp_bad, cond=cond_bad, min_z_over_tau=float((np.abs(ref["z"]) / t).min()),
                min_clamp_over_dw=float((np.abs(ref["w"] - CLAMP) / dw).min()),
                min_w_over_Sw=float((ref["w"] / ref["Sw"])[live].min()) if live.any() else float("inf"))


def _ratio(err, scale):
    """err / scale per group; a zero scale admits a zero error only"""
    err, scale = np.asarray(err, np.float64), np.asarray(scale, np.float64)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))


def rho(ref, got):
    """{tensor: (rho of its worst group, that group's label)} for every tensor `got` holds (numpy, any float type)"""
    B, C, P = ref["B"], ref["C"], ref["P"]
    res = {}

    def put(T, ratios, label):
        ratios = np.asarray(ratios).reshape(-1)
        i = int(np.argmax(ratios))
        res[T] = (float(ratios[i]), label(i))

    for T in TENSORS:
        if got.get(T) is None:
            continue
        want = ref[T]
        have = np.asarray(got[T], np.float64)
        assert have.shape == want.shape, (T, have.shape, want.shape)
        err = np.abs(have - want)
        if T == "g_x":
            err = np.maximum(err - ref["allow_g_x"], 0.0)
        if T == "g_x" and P == 1:
            put(T, _ratio(err.reshape(B, C).max(-1), np.abs(want).reshape(B, C).max(-1)), lambda i: "image %d" % i)
        elif T in ("y", "g_x"):
            e, s = err.reshape(B * C, P).max(-1), np.abs(want).reshape(B * C, P).max(-1)
            put(T, _ratio(e, s), lambda i: "image %d channel %d" % (i // C, i % C))
        elif T in ("g_W1", "g_W2"):
            s = np.maximum(np.abs(want).max(-1), U * ref["row_" + T[2:]])
            put(T, _ratio(err.max(-1), s), lambda i: "row %d" % i)
        elif T == "running_mean":
            put(T, _ratio(err, np.maximum(np.abs(want), np.sqrt(ref["var"]))), lambda i: "channel %d" % i)
        elif T == "running_var":
            put(T, _ratio(err, np.abs(want)), lambda i: "channel %d" % i)
        else:
            s = np.abs(ref["g_W1"]).max() if (T == "g_b1" and ref["batch_stats"]) else np.abs(want).max()
            put(T, _ratio(err.max(), s), lambda i: "whole tensor")
    return res


def masks(ref):
    return ref["z"] > 0, ref["w"] >= CLAMP


# ---------------------------------------------------------------- the stock chain, any dtype and device
def make_module(case, mode, dtype=torch.float32, device="cpu"):
    import torch.nn as nn
    training, momentum, affine, track = MODES[mode]
    C = int(np.asarray(case["W1"]).shape[0])
    mlp = nn.Sequential(nn.Linear(C, C), nn.BatchNorm1d(C, eps=float(case["eps"]), momentum=momentum, affine=affine,
                                                        track_running_stats=track), nn.ReLU(), nn.Linear(C, C))
    t = lambda k: torch.from_numpy(np.asarray(case[k]))
    with torch.no_grad():
        mlp[0].weight.copy_(t("W1")), mlp[0].bias.copy_(t("b1")), mlp[3].weight.copy_(t("W2")), mlp[3].bias.copy_(t("b2"))
        if affine:
            mlp[1].weight.copy_(t("gamma")), mlp[1].bias.copy_(t("beta"))
        if track:
            mlp[1].running_mean.copy_(t("running_mean")), mlp[1].running_var.copy_(t("running_var"))
            mlp[1].num_batches_tracked.fill_(int(case["num_batches_tracked"]))
    return mlp.train(training).to(device=device, dtype=dtype)


def params_of(mlp):
    lin1, bn, _, lin2 = mlp
    return [lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias]


def run_statement(fn, case, mode, dtype=torch.float32, device="cpu", mlp=None):
    """fn(x, wn_mlp) with autograd on a fresh module: ({tensor: numpy}, the module, the stock chain's (z > 0, w >= 1e-5) bits when
    the module's own layers ran)"""
    mlp = make_module(case, mode, dtype, device) if mlp is None else mlp
    seen = {}
    hooks = [mlp[1].register_forward_hook(lambda m, i, o: seen.__setitem__("z", o.detach())),
             mlp[3].register_forward_hook(lambda m, i, o: seen.__setitem__("o", o.detach()))]
    x = torch.from_numpy(np.asarray(case["x"])).to(device=device, dtype=dtype).requires_grad_(True)
    g = torch.from_numpy(np.asarray(case["g"])).to(device=device, dtype=dtype)
    y = fn(x, mlp)
    live = [(n, p) for n, p in zip(PARAMS, params_of(mlp)) if p is not None]
    grads = torch.autograd.grad((y * g).sum(), [x] + [p for _, p in live])
    for hk in hooks:
        hk.remove()
    npy = lambda v: v.detach().double().cpu().numpy()
    got = {"y": npy(y), "g_x": npy(grads[0])}
    got.update({"g_" + n: npy(v) for (n, _), v in zip(live, grads[1:])})
    if updates(mode):
        got.update(running_mean=npy(mlp[1].running_mean), running_var=npy(mlp[1].running_var))
    bits = None
    if "z" in seen:
        B, C, hh, ww = x.shape
        bits = ((seen["z"] > 0).cpu().numpy(), (seen["o"].view(B, hh * ww, C).mean(dim=1) >= CLAMP).cpu().numpy())
    return got, mlp, bits
