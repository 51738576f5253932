"""Lightning-side hook for the sharded acquisition round.

The reference enters the round on rank 0 only while the other DDP ranks stall
(core/train_learners.py:307-326):

    def on_train_batch_start(self, batch, batch_idx):
        if self.local_rank == 0 and batch_idx in self.active_iters and not self.debug:
            <save checkpoint>; RegionSelection(cfg, feature_extractor, classifier, active_loader, active_round)
            self.log('active_round', ...); self.active_round += 1
        return batch, batch_idx

`sharded_on_train_batch_start` is that method with the rank gate removed from the selection:
every rank scores its contiguous block of the pool (halo_amd.pool.region_selection_sharded), the
pick tables are all-gathered, and all ranks leave together.  The checkpoint is still written by
rank 0 only.  Bind it with `use_sharded_rounds(SourceFreeLearner)` (or assign the method on any
learner class with the same attributes); nothing else in the learner changes.  Optional attributes
of the learner: `acquisition_group` (process group), `acquisition_driver` (test stand-in) and
`acquisition_global_budget` (None = reference behaviour; an integer G switches the round to the
pool-wide budget of halo_amd.pool.region_selection_sharded).  Contract of a custom `acquisition_driver`:
`driver(cfg, feature_extractor, classifier, loader, round_number) -> [(picks (n, 3), count)]` in loader
order; with a global budget it is additionally passed the keyword `write_files=False` and must then write
NO file (the files follow from the kept picks) -- a driver without that keyword is refused.  No Lightning import
is needed here: the method only touches attributes the reference's learner already has.
"""
import os

import numpy as np
import torch

from .pool import region_selection_sharded


def sharded_on_train_batch_start(self, batch, batch_idx):
    if batch_idx in self.active_iters and not self.debug:
        if self.local_rank == 0:
            name = "model_before_round_{}.ckpt".format(self.active_round)
            print("\nSaving checkpoint: {}".format(name))
            self.trainer.save_checkpoint(os.path.join(self.cfg.SAVE_DIR, name))
            print(f"\n>>>>>>>>>>>>>>>> Active Round {self.active_round} (sharded) >>>>>>>>>>>>>>>>")
        self.last_round_tables = region_selection_sharded(self.cfg, self.feature_extractor, self.classifier,
                                                          self.active_loader, self.active_round,
                                                          group=getattr(self, "acquisition_group", None),
                                                          driver=getattr(self, "acquisition_driver", None),
                                                          # None (default) = the reference's per-image budget; an integer G =
                                                          # spend G regions over the whole pool this round (opt-in)
                                                          global_budget=getattr(self, "acquisition_global_budget", None))
        if self.local_rank == 0:
            self.log("active_round", self.active_round, on_step=True, on_epoch=False)
        self.active_round += 1          # on every rank: all of them ran the round
    return batch, batch_idx


def use_sharded_rounds(learner_cls):
    """Replace the learner's rank-0-only acquisition hook with the sharded one.  Returns the class."""
    learner_cls._reference_on_train_batch_start = learner_cls.__dict__.get("on_train_batch_start")
    learner_cls.on_train_batch_start = sharded_on_train_batch_start
    return learner_cls


# ---------------------------------------------------------------- validation metric on the device
# BaseLearner.validation_step / on_validation_epoch_end (core/train_learners.py:108-165) upsample both views of every validation
# image to (2, K, 1024, 2048), average, take the arg-max and histogram it on the host.  `use_device_metrics(learner_cls)` binds
# the two methods below instead: the head's low-resolution logits go straight to halo_amd.metrics (one HIP launch per image, the
# counts stay on the device), and the epoch end reduces those counts through `self.all_gather`.  The printed lines and the
# three `self.log` calls are the reference's.  A step the fused path does not cover -- more than one image, or a head output that
# is not float32 (2, K, h, w) on the device -- runs the reference's own step (kept as `_reference_validation_step`), whose
# per-image arrays the epoch end folds in.

def _metrics_accumulator(self, device=None):
    from .metrics import ConfusionAccumulator
    acc = getattr(self, "_device_metrics", None)
    if acc is None or (device is not None and acc.device != torch.device(device)):
        if device is None:                               # LightningModule.device; the counts of the epoch end live there
            device = getattr(self, "device", None)
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device())
        acc = ConfusionAccumulator(self.cfg.MODEL.NUM_CLASSES, device, self.cfg.INPUT.IGNORE_LABEL)
        self._device_metrics = acc
    return acc


def device_validation_step(self, batch, batch_idx):
    x, y = batch["img"], batch["label"]
    K = self.cfg.MODEL.NUM_CLASSES
    if x.shape[0] != 1 or y.shape[0] != 1:
        return self._reference_validation_step(batch, batch_idx)
    with torch.no_grad():
        image = torch.cat([x, torch.flip(x, [3])], 0)          # BaseLearner.inference(x, y, flip=True)
        output, _ = self.classifier(self.feature_extractor(image))
    if not (torch.is_tensor(output) and output.is_cuda and output.dtype == torch.float32 and output.dim() == 4
            and output.shape[0] == 2 and output.shape[1] == K):
        return self._reference_validation_step(batch, batch_idx)
    _metrics_accumulator(self, output.device).add_logits(output, y.reshape(y.shape[-2:]), flip=True)


def device_on_validation_epoch_end(self):
    acc = _metrics_accumulator(self)
    rows = [getattr(self, n, None) for n in ("intersections", "unions", "targets")]
    if all(r is not None and np.size(r) > 0 for r in rows):                 # steps the reference's own method counted
        acc.add_counts(np.stack([np.asarray(r, dtype=np.float64).reshape(-1, acc.K).sum(0) for r in rows]).round().astype(np.int64))
    acc.reduce(self.all_gather)
    m = acc.metrics()
    mIoU, mAcc, aAcc = m["mIoU"], m["mAcc"], m["aAcc"]

    print('\nmIoU: {:.2f}'.format(mIoU))
    print('mAcc: {:.2f}'.format(mAcc))
    print('aAcc: {:.2f}\n'.format(aAcc))

    self.log('mIoU', mIoU, on_step=False, on_epoch=True, sync_dist=True, prog_bar=True)
    self.log('mAcc', mAcc, on_step=False, on_epoch=True, sync_dist=True, prog_bar=True)
    self.log('aAcc', aAcc, on_step=False, on_epoch=True, sync_dist=True, prog_bar=True)

    acc.reset()
    self.intersections = np.array([])
    self.unions = np.array([])
    self.targets = np.array([])


def use_device_metrics(learner_cls):
    """Replace the learner's validation step and epoch end with the device-side metric.  Returns the class."""
    learner_cls._reference_validation_step = _inherited(learner_cls, "validation_step")
    learner_cls._reference_on_validation_epoch_end = _inherited(learner_cls, "on_validation_epoch_end")
    learner_cls.validation_step = device_validation_step
    learner_cls.on_validation_epoch_end = device_on_validation_epoch_end
    return learner_cls


def _inherited(cls, name):
    for klass in cls.__mro__:
        if name in klass.__dict__:
            return klass.__dict__[name]
    return None
