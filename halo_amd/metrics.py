"""Validation mIoU on the device (core/train_learners.py:57-165, core/utils/misc.py:35-47).

The reference's validation pass upsamples the head's logits of [x, flip(x)] to label size, takes the softmax, averages the map
with the flipped one, takes the arg-max and histograms prediction, label and agreement with torch.histc on the host, one image
at a time.  Here that chain is one HIP launch per batch (halo_eval.hip); the full-resolution maps never exist and the counts
stay on the device as exact int64, rows [intersection, union, target]:

    flip_tta_confusion(logits, label, K)          the fused chain: (B, 3, K) counts [+ the arg-max map]
    intersection_and_union_gpu(output, target, K) drop-in for core.utils.misc.intersectionAndUnionGPU
    ConfusionAccumulator(K, device)               an epoch's sum, its reduction over ranks and mIoU / mAcc / aAcc

There is no CPU route: every entry point that counts needs ROCm tensors (the accumulator's reduce / metrics also run on CPU
counts).
"""
import torch

from . import _lib

INTERSECTION, UNION, TARGET = 0, 1, 2          # rows of a count tensor


def _workspace(B, K, H, W, dev):
    n = _lib.lib().halo_eval_workspace_bytes(B, K, H, W)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def _counts_buffer(out, B, K, dev):
    if out is None:
        return torch.zeros((B, 3, K), dtype=torch.int64, device=dev)
    if out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != B * 3 * K or out.device != dev:
        raise ValueError("halo_amd.metrics: out must be a contiguous int64 tensor of %d x 3 x %d elements on %s" % (B, K, dev))
    return out


def _label_batch(label):
    if label.dim() == 2:
        label = label.unsqueeze(0)
    if label.dim() != 3:
        raise ValueError("halo_amd.metrics: label must be (H, W) or (B, H, W), got %s" % (tuple(label.shape),))
    return label.contiguous()


def flip_tta_confusion(logits, label, num_classes, ignore_index=255, flip=True, out=None, pred_out=None):
    """Counts of BaseLearner.inference + validation_step + intersectionAndUnionGPU for B images in one launch.

    logits: float32 (B*views, K, h, w) on the device, the head's low-resolution output; with flip=True (views = 2) rows 2i and
    2i+1 are image i and its horizontally flipped copy (what the head returns for cat([x, flip(x, [3])]) at B = 1).
    label: (B, H, W) or (H, W), int64 / int32 / uint8; the logits are upsampled to its size.
    Returns int64 (B, 3, K) counts, rows [intersection, union, target].  With `out` the counts are ADDED into it (so an epoch's
    sum can stay on the device without a host sync).  pred_out: optional int64 (B, H, W) receiving the arg-max map before the
    ignore write (what Test.test_step saves)."""
    K = int(num_classes)
    views = 2 if flip else 1
    label = _label_batch(label)
    B, H, W = label.shape
    if logits.dim() != 4 or logits.shape[0] != views * B or logits.shape[1] != K:
        raise ValueError("halo_amd.metrics: logits must be (%d, %d, h, w) for %d image(s), got %s" % (views * B, K, B, tuple(logits.shape)))
    if logits.dtype != torch.float32:
        raise TypeError("halo_amd.metrics: logits must be float32, got %s" % logits.dtype)
    dev = _lib.require_device(logits, label, out, pred_out)
    logits = logits.contiguous()
    h, w = logits.shape[2], logits.shape[3]
    counts = _counts_buffer(out, B, K, dev)
    if pred_out is not None and (pred_out.dtype != torch.int64 or not pred_out.is_contiguous() or pred_out.numel() != B * H * W):
        raise ValueError("halo_amd.metrics: pred_out must be a contiguous int64 tensor of %d x %d x %d elements" % (B, H, W))
    L = _lib.lib()
    ws, nws = _workspace(B, K, H, W, dev)
    _lib.check(L.halo_eval_confusion(_lib.ptr(logits), K * h * w, views, K, h, w, _lib.ptr(label), _lib.int_code(label), H, W, B,
                                     int(ignore_index), _lib.ptr(counts), _lib.ptr(pred_out), _lib.ptr(ws), nws, _lib.stream_ptr(dev)),
               "halo_eval_confusion")
    return counts


def confusion_from_pred(pred, label, num_classes, ignore_index=255, out=None):
    """Counts (B, 3, K) of a prediction map already on the device: pred and label (B, H, W) or (H, W), int64 / int32 / uint8.
    The counts are ADDED into `out` when given."""
    K = int(num_classes)
    pred, label = _label_batch(pred), _label_batch(label)
    if pred.shape != label.shape:
        raise ValueError("halo_amd.metrics: pred %s and label %s differ in shape" % (tuple(pred.shape), tuple(label.shape)))
    B, H, W = label.shape
    dev = _lib.require_device(pred, label, out)
    counts = _counts_buffer(out, B, K, dev)
    L = _lib.lib()
    ws, nws = _workspace(B, K, H, W, dev)
    _lib.check(L.halo_confusion_from_pred(_lib.ptr(pred), _lib.int_code(pred), _lib.ptr(label), _lib.int_code(label), K, H, W, B,
                                          int(ignore_index), _lib.ptr(counts), _lib.ptr(ws), nws, _lib.stream_ptr(dev)),
               "halo_confusion_from_pred")
    return counts


def intersection_and_union_gpu(output, target, K, ignore_index=255):
    """core.utils.misc.intersectionAndUnionGPU on the device: float32 (K,) intersection, union and target areas on output's
    device, equal to the reference's values (its float32 histc is exact below 2^24 per bin).

    The one deviation: the reference writes ignore_index into `output` in place where the target is ignored; this function
    leaves `output` as it is."""
    assert output.dim() in (1, 2, 3)
    assert output.shape == target.shape
    n = output.numel()
    counts = confusion_from_pred(output.reshape(1, 1, n), target.reshape(1, 1, n), K, ignore_index)[0].to(torch.float32)
    return counts[INTERSECTION], counts[UNION], counts[TARGET]


def _is_process_group(obj):
    import torch.distributed as dist
    return dist.is_available() and isinstance(obj, dist.ProcessGroup)


class ConfusionAccumulator(object):
    """An epoch's validation counts, int64 (3, K) on `device`, rows [intersection, union, target].

        acc = ConfusionAccumulator(19, "cuda:0")
        acc.add_logits(head_out, label)          # per validation step (no host sync)
        acc.reduce(self.all_gather)              # at epoch end: sum over ranks (Lightning's all_gather or a process group)
        acc.metrics()["mIoU"]; acc.reset()
    """

    def __init__(self, K, device, ignore_index=255):
        self.K = int(K)
        self.device = torch.device(device)
        self.ignore_index = int(ignore_index)
        self._counts = torch.zeros((3, self.K), dtype=torch.int64, device=self.device)

    def add_logits(self, logits, label, flip=True, pred_out=None):
        """Count B images from the head's low-resolution logits (flip_tta_confusion's layout)."""
        B = 1 if label.dim() == 2 else label.shape[0]
        if B == 1:
            flip_tta_confusion(logits, label, self.K, self.ignore_index, flip=flip, out=self._counts, pred_out=pred_out)
        else:
            self._counts += flip_tta_confusion(logits, label, self.K, self.ignore_index, flip=flip, pred_out=pred_out).sum(0)
        return self

    def add_pred(self, pred, label):
        """Count prediction maps (B, H, W) or (H, W) against their labels."""
        B = 1 if label.dim() <= 2 else label.shape[0]
        if B == 1:
            confusion_from_pred(pred, label, self.K, self.ignore_index, out=self._counts)
        else:
            self._counts += confusion_from_pred(pred, label, self.K, self.ignore_index).sum(0)
        return self

    def add_counts(self, counts):
        """Add counts of the same layout ((3, K) or (N, 3, K)) from elsewhere, e.g. the reference's per-image float arrays."""
        c = torch.as_tensor(counts)
        if c.dim() == 3:
            c = c.sum(0)
        self._counts += c.to(device=self.device, dtype=torch.int64)
        return self

    def counts(self):
        """A copy of the int64 (3, K) counts."""
        return self._counts.clone()

    def reduce(self, all_gather=None):
        """Sum the counts over ranks and keep the sum (call once per epoch).  `all_gather`: Lightning's `self.all_gather`
        (returns (world, 3, K), or (3, K) on one process), a torch.distributed process group, or None (one process)."""
        if all_gather is None:
            return self.counts()
        if _is_process_group(all_gather):
            import torch.distributed as dist
            c = self._counts
            if c.is_cuda and dist.get_backend(all_gather) == "gloo":
                c = c.cpu()
            dist.all_reduce(c, op=dist.ReduceOp.SUM, group=all_gather)
            self._counts = c.to(self.device)
        else:
            g = torch.as_tensor(all_gather(self._counts))
            self._counts = (g.sum(0) if g.dim() == 3 else g).to(device=self.device, dtype=torch.int64)
        return self.counts()

    def metrics(self):
        """mIoU / mAcc / aAcc (percent) and the per-class arrays, with the reference's formulas (train_learners.py:145-151):
        +1e-10 in every denominator, so a class absent from both prediction and label counts 0 in the means.  Computed in
        float64 from the exact counts (the reference sums float32 arrays: the two differ by at most ~1e-6 relative)."""
        c = self._counts.detach().cpu().to(torch.float64).numpy()
        inter, union, target = c[INTERSECTION], c[UNION], c[TARGET]
        iou_class = inter / (union + 1e-10)
        accuracy_class = inter / (target + 1e-10)
        return {"mIoU": float(iou_class.mean() * 100), "mAcc": float(accuracy_class.mean() * 100),
                "aAcc": float(inter.sum() / (target.sum() + 1e-10) * 100),
                "iou_class": iou_class, "accuracy_class": accuracy_class,
                "intersection": inter, "union": union, "target": target}

    def reset(self):
        self._counts.zero_()
        return self


__all__ = ["flip_tta_confusion", "confusion_from_pred", "intersection_and_union_gpu", "ConfusionAccumulator"]
