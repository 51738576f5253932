"""HFR weighted normalisation on the device (halo_hfr.hip through halo_amd.hfr / halo_amd.hooks) against the reference's own head
(tests/golden/hfr.npz, tests/golden/make_hfr_fixtures.py, float64 evaluation) and the torch statement run in float64 on the
device: y within 2e-6 * max|y|, every gradient within 2e-5 * its max|g|, running statistics within 2e-6 relative."""
import multiprocessing as mp
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIX = os.path.join(GOLDEN, "hfr.npz")
PARAMS = ("W1", "b1", "gamma", "beta", "W2", "b2")
ROWS = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from halo_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def case(name):
    z = np.load(FIX)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


def cases():
    z = np.load(FIX)
    return sorted({k.split("/")[0] for k in z.files})


def make_mlp(C, norm=nn.BatchNorm1d, momentum=0.1):
    return nn.Sequential(nn.Linear(C, C), norm(C, momentum=momentum), nn.ReLU(), nn.Linear(C, C))


def params_of(mlp):
    lin1, bn, _, lin2 = mlp
    return [lin1.weight, lin1.bias, bn.weight, bn.bias, lin2.weight, lin2.bias]


def mlp_from_case(d, device, dtype=torch.float32):
    C, B, h, w, training, mom_none, nbt = (int(v) for v in d["meta"])
    mlp = make_mlp(C, momentum=None if mom_none < 0 else float(d["momentum"]))
    with torch.no_grad():
        for p, t in zip(PARAMS, params_of(mlp)):
            t.copy_(torch.from_numpy(d[p].astype(np.float32)))
        mlp[1].running_mean.copy_(torch.from_numpy(d["running_mean_in"]))
        mlp[1].running_var.copy_(torch.from_numpy(d["running_var_in"]))
        mlp[1].num_batches_tracked.fill_(nbt)
    mlp.train(bool(training))
    return mlp.to(device=device, dtype=dtype)


def near(got, want, rel, scale=None):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    assert got.shape == want.shape
    err, scale = np.abs(got - want).max(), max(np.abs(want).max(), scale or 0.0)
    assert err <= rel * scale + 1e-30, "max err %.3e vs bar %.3e" % (err, rel * scale)


def near_dx(got, want, x):
    """d x within 2e-5 of its max, an all-zero channel (the eps branch of F.normalize: g / eps) held to its own max"""
    zero = torch.as_tensor(np.abs(np.asarray(x)).reshape(x.shape[0], x.shape[1], -1).max(-1) == 0)
    got = got.detach().cpu()
    want = torch.as_tensor(np.asarray(want))
    for sel in (zero, ~zero):
        if bool(sel.any()):
            near(got[sel], want[sel], 2e-5)


def grad_scale(d, p):
    """under batch statistics d b1 = sum_p g_h is zero up to rounding (the BatchNorm removes b1); it is held to the scale
    of d W1 = sum_p g_h x^T instead of its own"""
    return float(np.abs(d["f64/dW1"]).max()) if p == "b1" else None


def run_fused(x, mlp, g):
    from halo_amd.hfr import weighted_normalize, fallback_reason
    assert fallback_reason(x, mlp) is None
    x = x.detach().clone().requires_grad_(True)
    y = weighted_normalize(x, mlp)
    grads = torch.autograd.grad((y * g).sum(), [x] + params_of(mlp))
    return y.detach(), grads[0], grads[1:]


@pytest.mark.parametrize("name", cases())
def test_fixture(dev, name):
    d = case(name)
    mlp = mlp_from_case(d, dev)
    x = torch.from_numpy(d["x"]).to(dev)
    g = torch.from_numpy(d["g"]).to(dev)
    y, dx, grads = run_fused(x, mlp, g)
    near(y, d["f64/y"], 2e-6)
    near_dx(dx, d["f64/dx"], d["x"])
    for p, gp in zip(PARAMS, grads):
        near(gp[:ROWS] if p in ("W1", "W2") else gp, d["f64/d" + p], 2e-5, scale=grad_scale(d, p))
    near(mlp[1].running_mean, d["f64/running_mean"], 2e-6)
    near(mlp[1].running_var, d["f64/running_var"], 2e-6)
    assert int(mlp[1].num_batches_tracked) == int(d["meta"][6]) + (1 if d["meta"][4] else 0)


def torch_reference(x, mlp, g):
    from halo_amd.hfr import torch_statement
    x = x.detach().clone().requires_grad_(True)
    y = torch_statement(x, mlp)
    grads = torch.autograd.grad((y * g).sum(), [x] + params_of(mlp))
    return y.detach(), grads[0], grads[1:]


@pytest.mark.parametrize("training", [True, False])
def test_training_shape_and_bits(dev, training):
    torch.manual_seed(3)
    B, C, h, w = 2, 64, 160, 320
    x = torch.randn(B, C, h, w, device=dev) * 0.7 + 0.1
    g = torch.randn(B, C, h, w, device=dev)
    mlp = make_mlp(C).to(dev).train(training)
    with torch.no_grad():
        mlp[1].running_mean.normal_(0.0, 0.3)
        mlp[1].running_var.uniform_(0.5, 1.5)
        mlp[3].bias[:3] = -10.0                                   # clamp active
    ref = make_mlp(C).to(dev).train(training)
    ref.load_state_dict(mlp.state_dict())
    ref = ref.double()
    y, dx, grads = run_fused(x, mlp, g)
    ry, rdx, rgrads = torch_reference(x.double(), ref, g.double())
    near(y, ry, 2e-6)
    near(dx, rdx, 2e-5)
    for gp, rg, p in zip(grads, rgrads, PARAMS):
        near(gp, rg, 2e-5, scale=float(rgrads[0].abs().max()) if p == "b1" else None)
    near(mlp[1].running_mean, ref[1].running_mean, 2e-6)
    near(mlp[1].running_var, ref[1].running_var, 2e-6)
    # two calls on the same inputs and parameters (fresh copies of the module) return identical bits
    mlp2 = make_mlp(C).to(dev).train(training)
    mlp2.load_state_dict(mlp.state_dict())
    mlp3 = make_mlp(C).to(dev).train(training)
    mlp3.load_state_dict(mlp.state_dict())
    y2, dx2, g2 = run_fused(x, mlp2, g)
    y3, dx3, g3 = run_fused(x, mlp3, g)
    assert torch.equal(y2, y3) and torch.equal(dx2, dx3)
    assert all(torch.equal(a, b) for a, b in zip(g2, g3))
    assert torch.equal(mlp2[1].running_mean, mlp3[1].running_mean) and torch.equal(mlp2[1].running_var, mlp3[1].running_var)


def _both(x, mlp_a, mlp_b, fn_a, fn_b):
    """(result or exception) of fn_a(x, mlp_a) and fn_b(x, mlp_b)"""
    out = []
    for fn, m in ((fn_a, mlp_a), (fn_b, mlp_b)):
        try:
            out.append(fn(x, m))
        except Exception as exc:          # noqa: BLE001 -- the exception itself is compared
            out.append(exc)
    return out


@pytest.mark.parametrize("kind", ["float64", "autocast", "wide", "structure", "single_row"])
def test_fallbacks(dev, kind):
    from halo_amd.hfr import weighted_normalize, torch_statement, fallback_reason
    torch.manual_seed(5)
    C, B, h, w, dtype = 16, 2, 5, 7, torch.float32
    if kind == "float64":
        dtype = torch.float64
    if kind == "wide":
        C = 260
    if kind == "single_row":
        B, h, w = 1, 1, 1
    mlp = make_mlp(C)
    if kind == "structure":
        mlp = nn.Sequential(nn.Linear(C, C), nn.BatchNorm1d(C), nn.ReLU(), nn.Dropout(0.0), nn.Linear(C, C))
    mlp = mlp.to(device=dev, dtype=dtype).train()
    ref = make_mlp(C) if kind != "structure" else nn.Sequential(nn.Linear(C, C), nn.BatchNorm1d(C), nn.ReLU(), nn.Dropout(0.0), nn.Linear(C, C))
    ref = ref.to(device=dev, dtype=dtype).train()
    ref.load_state_dict(mlp.state_dict())
    x = torch.randn(B, C, h, w, device=dev, dtype=dtype)
    if kind == "autocast":
        with torch.autocast("cuda", dtype=torch.float16):
            assert fallback_reason(x, mlp) is not None
            got, want = _both(x, mlp, ref, weighted_normalize, torch_statement)
    else:
        assert fallback_reason(x, mlp) is not None
        got, want = _both(x, mlp, ref, weighted_normalize, torch_statement)
    if isinstance(want, Exception):
        assert type(got) is type(want) and str(got) == str(want)
    else:
        assert got.dtype == want.dtype and torch.equal(got, want)
        assert torch.equal(mlp[1].running_mean, ref[1].running_mean)


class _Head(nn.Module):
    """a stand-in v3+ hyperbolic head with the reference's attribute names (small layers)"""

    def __init__(self, C=64, K=5):
        super().__init__()
        from halo_amd.core.utils.hyperbolic import HyperMapper, HyperMLR
        self.parallel_branches = nn.ModuleList([nn.Conv2d(8, 8, 1), nn.Conv2d(8, 8, 3, padding=1)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(8, 8, 1))
        self.bottleneck = nn.Conv2d(24, 16, 1)
        self.shortcut = nn.Conv2d(4, 4, 1)
        self.decoder = nn.Conv2d(20, 16, 3, padding=1)
        self.conv_reduce = nn.Conv2d(16, C, 1)
        self.mapper = HyperMapper(c=1.0)
        self.conv_seg = HyperMLR(C, K, c=1.0)
        self.wn_mlp = make_mlp(C)


def test_hooked_head(dev):
    from halo_amd.core.models.classifier import v3plus_hyper_forward
    from halo_amd.hooks import use_fused_feature_reweighting, fused_v3plus_hyper_forward

    class Plain(_Head):
        forward = v3plus_hyper_forward

    class Fused(_Head):
        forward = v3plus_hyper_forward

    assert use_fused_feature_reweighting(Fused) is Fused
    assert Fused.forward is fused_v3plus_hyper_forward and Fused._unfused_forward is v3plus_hyper_forward
    assert Plain.forward is v3plus_hyper_forward
    torch.manual_seed(11)
    a = Plain().to(dev).train()
    b = Fused().to(dev).train()
    b.load_state_dict(a.state_dict())
    a64 = Plain().to(dev).double().train()
    a64.load_state_dict(a.state_dict())
    feats = {"low": torch.randn(2, 4, 24, 40, device=dev), "out": torch.randn(2, 8, 12, 20, device=dev)}
    outs = {}
    for tag, head in (("fused", b), ("plain", a)):
        out, embed = head(feats)
        loss = out.square().mean() + embed.sum()
        grads = torch.autograd.grad(loss, list(head.parameters()))
        outs[tag] = (out.detach(), embed.detach(), grads)
    (fo, fe, fg), (po, pe, pg) = outs["fused"], outs["plain"]
    near(fe, pe, 2e-5)
    near(fo, po, 2e-5)
    # both heads run in float32 and the unhooked one's wn_mlp gradients carry the stock chain's own rounding (the BatchNorm
    # backward amplifies it); the fused path is held to 2e-5 against float64 above, so here 5e-4 of max|g| for every parameter
    names = [n for n, _ in a.named_parameters()]
    w1 = names.index("wn_mlp.0.weight")
    for n, x1, x2 in zip(names, fg, pg):
        near(x1, x2, 5e-4, scale=float(pg[w1].abs().max()) if n == "wn_mlp.0.bias" else None)   # d b1: see grad_scale


# ---------------------------------------------------------------- SyncBatchNorm at world 2 over gloo
def _rank_main(rank, world, store, inputs, out_path):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world)
    try:
        from halo_amd.hfr import weighted_normalize
        d = torch.load(inputs)
        dev = torch.device("cuda:0")
        mlp = make_mlp(d["C"], norm=nn.SyncBatchNorm)
        mlp.load_state_dict(d["state"])
        mlp = mlp.to(dev).train()
        half = d["x"].shape[0] // world
        x = d["x"][rank * half:(rank + 1) * half].to(dev).requires_grad_(True)
        g = d["g"][rank * half:(rank + 1) * half].to(dev)
        y = weighted_normalize(x, mlp)
        grads = torch.autograd.grad((y * g).sum(), [x] + params_of(mlp))
        torch.save({"y": y.detach().cpu(), "dx": grads[0].cpu(), "grads": [t.cpu() for t in grads[1:]],
                    "rm": mlp[1].running_mean.cpu(), "rv": mlp[1].running_var.cpu()}, out_path)
    finally:
        dist.destroy_process_group()


def test_sync_batchnorm_world2(dev):
    torch.manual_seed(21)
    C, B, h, w = 64, 4, 20, 40
    x = torch.randn(B, C, h, w) * 0.8
    g = torch.randn(B, C, h, w)
    mlp = make_mlp(C)
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "inputs.pt")
        torch.save({"C": C, "x": x, "g": g, "state": mlp.state_dict()}, inputs)
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_rank_main, args=(r, 2, os.path.join(tmp, "store"), inputs, os.path.join(tmp, "r%d.pt" % r)))
                 for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=240)
        for p in procs:
            if p.is_alive():
                p.kill()
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        res = [torch.load(os.path.join(tmp, "r%d.pt" % r)) for r in range(2)]
    full = make_mlp(C).to(dev).train()
    full.load_state_dict(mlp.state_dict())
    y, dx, grads = run_fused(x.to(dev), full, g.to(dev))
    for r in range(2):
        near(res[r]["y"], y[2 * r:2 * r + 2], 1e-6)
        near(res[r]["dx"], dx[2 * r:2 * r + 2], 1e-5)
    for i in range(6):
        near(res[0]["grads"][i] + res[1]["grads"][i], grads[i], 1e-5, scale=float(grads[0].abs().max()) if i == 1 else None)
    assert torch.equal(res[0]["rm"], res[1]["rm"]) and torch.equal(res[0]["rv"], res[1]["rv"])
    near(res[0]["rm"], full[1].running_mean, 1e-6)
    near(res[0]["rv"], full[1].running_var, 1e-6)
