"""CPU checks of the validation metric (halo_amd.metrics, halo_amd.hooks.use_device_metrics): the fixture generator is pinned
to a torch-CPU statement of the chain, the accumulator's epoch-end arithmetic to the reference's formula, the hook's hand-over
and the reduction over two gloo ranks.  The kernels themselves are held to the fixture in tests/test_gpu_eval.py."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_inputs as ei  # noqa: E402

FIX = os.path.join(GOLDEN, "eval.npz")


def small_cases():
    z = np.load(FIX)
    return sorted({k.split("/")[0] for k in z.files if not k.startswith("full_")})


@pytest.mark.parametrize("name", small_cases())
def test_fixture_equals_torch_cpu_chain(name):
    z = np.load(FIX)
    K, flip = (int(v) for v in z[name + "/meta"])
    label = z[name + "/label"]
    pred = ei.torch_chain_pred(torch.from_numpy(z[name + "/logits"]), label.shape[-2:], bool(flip)).numpy()
    assert np.array_equal(pred, z[name + "/pred"])
    ref = z[name + "/ref"]
    assert ref.dtype == np.float32 and ref.shape == (label.shape[0], 3, K)
    for i in range(label.shape[0]):
        assert np.array_equal(ei.counts_from_pred(pred[i], label[i], K), ref[i].astype(np.int64))


def test_fixture_covers_the_edge_cases():
    z = np.load(FIX)
    for name in small_cases():
        K, flip = (int(v) for v in z[name + "/meta"])
        lg, label, pred = z[name + "/logits"], z[name + "/label"], z[name + "/pred"]
        views = 2 if flip else 1
        assert pred[0, 0, 0] == 0                                    # all classes tied
        assert np.isnan(lg[2 * views]).any() and pred[2, 31, 63] == 0  # NaN logit next to the centre pixel -> class 0
        if K > 5:
            assert (pred[1] == 3).sum() > 0.8 * pred[1].size and not (pred[1] == 5).any()   # identical planes: the lower wins
        lab = label.astype(np.int64)
        assert (lab == 255).any() and ((lab >= K) & (lab < 255)).any()
        assert (lab == -1).any() == (label.dtype != np.uint8)


@pytest.mark.parametrize("name", sorted(ei.FULLSIZE))
def test_fullsize_fixture_equals_torch_cpu_chain(name):
    z = np.load(FIX)
    lg, label = ei.fullsize(name)
    pred = ei.torch_chain_pred(torch.from_numpy(lg), label.shape, True)[0].numpy()
    assert ei.digest(pred) == str(z["full_" + name + "/pred_sha256"])
    assert np.array_equal(ei.counts_from_pred(pred, label, 19), z["full_" + name + "/ref"].astype(np.int64))


# ---------------------------------------------------------------- the contract chain (oracle/) and the ragged inputs
@pytest.mark.parametrize("name", small_cases())
def test_contract_chain_equals_the_reference_maps(name):
    """eval.npz's `pred` is the reference's own arg-max map, so this makes the oracle's chain the reference's chain."""
    z = np.load(FIX)
    _, flip = (int(v) for v in z[name + "/meta"])
    label = z[name + "/label"]
    assert np.array_equal(ei.contract_pred(z[name + "/logits"], label.shape[-2:], bool(flip)), z[name + "/pred"])


@pytest.mark.parametrize("name", sorted(ei.FULLSIZE))
def test_contract_chain_reproduces_the_fullsize_digests(name):
    z = np.load(FIX)
    lg, label = ei.fullsize(name)
    assert ei.digest(ei.contract_pred(lg, label.shape, True)[0]) == str(z["full_" + name + "/pred_sha256"])


@pytest.mark.parametrize("name", sorted(ei.RAGGED))
def test_contract_chain_differs_from_torch_only_within_atens_scalar_tails(name):
    """Off multiples of 16 pixels torch's CPU softmax ends each thread's chunk with a scalar exp (tests/test_aten_exact.py:
    fewer than 16 pixels per thread and softmaxed view, plus one vector for the chunk boundaries), so the live torch chain may
    leave contract_pred there and nowhere else.  Observed: 0 pixels on every case but k19_identity_5x7, where the identity
    resize spreads the NaN logit over four pixels (weight 0 times NaN) and torch's scalar tail orders a NaN maximum
    differently: 2 of image 0's 35 pixels."""
    K, views, lg, label, pred = ei.ragged_case(name)
    live = ei.torch_chain_pred(torch.from_numpy(lg.copy()), label.shape[-2:], views == 2).numpy()
    differ = (live != pred).reshape(pred.shape[0], -1).sum(1)
    print(name, "pixels where torch's chain leaves the contract chain, per image:", differ.tolist())
    assert int(differ.max()) <= views * 16 * (torch.get_num_threads() + 1)


def test_ragged_inputs_reach_the_arms_they_are_meant_for():
    from oracle import halo_oracle as ho
    dtypes = {}
    for name in sorted(ei.RAGGED):
        _, K, (h, w), (H, W), views, B, dtype = ei.RAGGED[name]
        K_, views_, lg, label, pred = ei.ragged_case(name)
        assert (K_, views_) == (K, views) and lg.shape == (B * views, K, h, w) and label.shape == pred.shape == (B, H, W)
        assert label.dtype == dtype and pred.dtype == np.int64 and pred.min() >= 0 and pred.max() < K
        dtypes.setdefault("generic" if K not in (16, 19) else "k%d" % K, set()).add(np.dtype(dtype).name)
        lab = label.astype(np.int64)
        assert (lab == 255).any() and (dtype == np.uint8 or (lab == -1).any())
        assert ((lab >= K) & (lab != 255)).any() or (K > 255 and dtype == np.uint8)
        last = lab.reshape(B, -1)[:, -1]                                      # tail lanes recompute the last pixel: it must be one that
        assert ((last >= 0) & (last < K) & (last != 255)).all()              # counts, or a lost lane mask would add nothing
        counts = sum(ei.counts_from_pred(pred[i], label[i], K) for i in range(B))
        assert counts[0].sum() > 0                                           # some agreement: the intersection row is not empty
        one_cell = h * w == 1
        if one_cell:
            assert (pred == 3).all()                                         # one logit vector: identical planes 3 and 5, the lower wins
        elif K > 1:
            assert len(np.unique(pred)) >= 2
        if not one_cell:
            assert pred[ei.RAGGED_TIE_IMAGE % B, 0, 0] == 0                  # all classes tied in both views
            i = ei.RAGGED_NAN_IMAGE % B
            nan = np.isnan(ho.bilinear(lg[views * i, min(1, K - 1)], (H, W)))
            assert nan.any() and (pred[i][nan] == 0).all()                   # NaN logit -> NaN softmax -> class 0
        if K > 5:
            planes = pred[ei.RAGGED_PLANES_IMAGE % B]
            assert not (planes == 5).any()                                   # identical planes: never the higher index
            if B > 1:                                                        # an image of its own: the planes win most of it
                assert (planes == 3).sum() > 0.5 * planes.size               # (74 % where the identity size does no smoothing)
        if K == 86:
            # 3 K = 258 words: clear_hist / store_hist's second trip carries words 256 and 257, the targets of classes 84 and 85
            assert counts[2, 84] > 0 and counts[2, 85] > 0
        if K == 1024:
            # the later trips carry every intersection word of a class >= 256 and all output and target words
            assert (pred >= 256).any() and (lab[lab < K] >= 256).any() and counts[0, 256:].sum() > 0
    assert all(v == {"int64", "int32", "uint8"} for v in dtypes.values()) and set(dtypes) == {"k19", "k16", "generic"}


def test_counts_from_pred_with_an_ignore_index_among_the_classes_is_three_histc():
    """intersectionAndUnionGPU (core/utils/misc.py:35-47) written out, with ignore_index = 7 < K: the label's 7s overwrite
    the prediction and are then counted as class 7 in all three rows."""
    K, ignore_index = 19, 7
    _, _, _, label, pred = ei.ragged_case("k19_37x53")
    for i in range(label.shape[0]):
        output = torch.from_numpy(pred[i].copy()).view(-1)
        target = torch.from_numpy(label[i].astype(np.int64)).view(-1)
        assert (target == ignore_index).any() and ((output == ignore_index) & (target != ignore_index)).any()
        output[target == ignore_index] = ignore_index                      # in place, before anything is counted

        def histc(v):
            return torch.histc(v.float(), bins=K, min=0, max=K - 1)

        inter, out, tgt = histc(output[output == target]), histc(output), histc(target)
        want = torch.stack([inter, out + tgt - inter, tgt]).numpy()
        got = ei.counts_from_pred(pred[i], label[i], K, ignore_index=ignore_index)
        assert np.array_equal(got, want.astype(np.int64))
        assert not np.array_equal(got, ei.counts_from_pred(pred[i], label[i], K))


def reference_epoch_end(inter, union, target):
    """train_learners.py:138-151 on gathered float32 per-image arrays (N, K)"""
    inter, union, target = inter.sum(axis=0), union.sum(axis=0), target.sum(axis=0)
    iou_class = inter / (union + 1e-10)
    accuracy_class = inter / (target + 1e-10)
    return (iou_class.mean() * 100, accuracy_class.mean() * 100, inter.sum() / (target.sum() + 1e-10) * 100)


def random_counts(n, K, seed):
    """per-image (n, 3, K) int64 counts; class K-1 absent from prediction and label everywhere"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 50000, (n, K))
    tgt = rng.integers(0, 50000, (n, K))
    inter = np.minimum(out, tgt) // rng.integers(1, 4, (n, K))
    out[:, -1] = tgt[:, -1] = inter[:, -1] = 0
    return np.stack([inter, out + tgt - inter, tgt], axis=1).astype(np.int64)


def test_accumulator_metrics_and_reduce_equal_reference_formula():
    from halo_amd.metrics import ConfusionAccumulator
    c = random_counts(12, 19, 0)
    f = c.astype(np.float32)
    want = reference_epoch_end(f[:, 0], f[:, 1], f[:, 2])
    acc = ConfusionAccumulator(19, "cpu").add_counts(torch.from_numpy(c))
    m = acc.metrics()
    for k, v in zip(("mIoU", "mAcc", "aAcc"), want):
        assert abs(m[k] - float(v)) <= 1e-6 * abs(float(v))
    assert m["iou_class"][-1] == 0.0 and m["accuracy_class"][-1] == 0.0
    assert np.array_equal(acc.counts().numpy(), c.sum(0))
    # Lightning's all_gather: (world, 3, K) for several processes, the tensor itself for one
    other = torch.from_numpy(random_counts(5, 19, 1).sum(0))
    got = acc.reduce(lambda t: torch.stack([t, other]))
    assert np.array_equal(got.numpy(), c.sum(0) + other.numpy())
    acc.reset().add_counts(other)
    assert np.array_equal(acc.reduce(lambda t: t).numpy(), other.numpy())
    assert not acc.reset().counts().any()


class StandInLearner(object):
    """The attributes BaseLearner's validation methods use; its own validation_step records its calls."""

    def __init__(self):
        self.cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=19), INPUT=types.SimpleNamespace(IGNORE_LABEL=255))
        self.device = torch.device("cpu")
        self.calls, self.logged = [], {}
        self.intersections = self.unions = self.targets = np.array([])

    def validation_step(self, batch, batch_idx):
        self.calls.append(batch_idx)
        c = random_counts(1, 19, batch_idx).astype(np.float32)
        for attr, row in zip(("intersections", "unions", "targets"), (c[:, 0], c[:, 1], c[:, 2])):
            have = getattr(self, attr)
            setattr(self, attr, row if have.size == 0 else np.concatenate((have, row), axis=0))

    def on_validation_epoch_end(self):
        raise AssertionError("replaced by the hook")

    def all_gather(self, t):
        return t

    def log(self, name, value, **kw):
        self.logged[name] = (value, kw)


def test_use_device_metrics_hands_batch_2_to_the_reference_and_folds_its_arrays():
    from halo_amd.hooks import use_device_metrics

    class Learner(StandInLearner):
        pass

    use_device_metrics(Learner)
    assert Learner._reference_validation_step is StandInLearner.__dict__["validation_step"]
    assert Learner._reference_on_validation_epoch_end is StandInLearner.__dict__["on_validation_epoch_end"]
    me = Learner()
    batch = {"img": torch.zeros((2, 3, 8, 16)), "label": torch.zeros((2, 8, 16), dtype=torch.int64), "name": ["a", "b"]}
    me.validation_step(batch, 3)
    me.validation_step(batch, 4)
    assert me.calls == [3, 4]
    want = reference_epoch_end(me.intersections, me.unions, me.targets)
    me.on_validation_epoch_end()
    for k, v in zip(("mIoU", "mAcc", "aAcc"), want):
        value, kw = me.logged[k]
        assert abs(value - float(v)) <= 1e-6 * abs(float(v))
        assert kw == dict(on_step=False, on_epoch=True, sync_dist=True, prog_bar=True)
    assert me.intersections.size == 0 and not me._device_metrics.counts().any()


def _gloo_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from halo_amd.metrics import ConfusionAccumulator
    acc = ConfusionAccumulator(19, "cpu").add_counts(torch.from_numpy(random_counts(3, 19, 10 + rank)))
    got = acc.reduce(dist.group.WORLD)
    np.save(os.path.join(outdir, "rank%d.npy" % rank), got.numpy())
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_reduce_over_two_gloo_ranks_sums_the_counts(tmp_path):
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    want = random_counts(3, 19, 10).sum(0) + random_counts(3, 19, 11).sum(0)
    for r in range(2):
        assert np.array_equal(np.load(tmp_path / ("rank%d.npy" % r)), want)
