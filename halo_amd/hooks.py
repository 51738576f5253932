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
import torch.nn.functional as F

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


# ---------------------------------------------------------------- training criterion from low-resolution logits
# Every learner's training_step (core/train_learners.py:224-243, 328-368, 404-463, 505-563) asks the head for logits at the input
# size, then runs torch.softmax, CrossEntropyLoss and NegativeLearningLoss on the full-resolution maps.  `use_fused_training_losses
# (learner_cls)` binds a training_step that calls the head WITHOUT `size` and hands its low-resolution logits to
# halo_amd.training.upsampled_losses (one forward and one backward launch per image batch, no full-resolution map).  The step keeps
# the reference's protocol: the accumulator, the labelled-pixel gate (answered by the kernel's count), the loss weights, every
# self.log name and keyword, manual_backward and the optimiser / scheduler steps.  LocalConsistentLoss keeps its full-resolution
# input (F.interpolate of the source logits, built only when CONSISTENT_LOSS > 0).  A head output that is not a tuple whose first
# element is float32 (B, K, h, w) on the device (the non-hyper DeepLab-v2 head returns a bare tensor) runs the reference's own
# step, kept as `_reference_training_step`; the forward already run for that probe is then repeated by that step.

_PROTOCOLS = ("FullySupervisedLearner", "SourceTargetLearner", "SourceFreeLearner", "SourceLearner")


def _training_protocol(cls):
    """the reference learner whose training_step the class inherits: the first of _PROTOCOLS in its MRO (None if none)"""
    for klass in cls.__mro__:
        if klass.__name__ in _PROTOCOLS:
            return klass.__name__
    return None


def _head_logits(self, x):
    """the head's low-resolution logits for x, or None when the output is not served"""
    out = self.classifier(self.feature_extractor(x))
    if not isinstance(out, (tuple, list)) or len(out) == 0:
        return None
    lg = out[0]
    if not (torch.is_tensor(lg) and lg.is_cuda and lg.dtype == torch.float32 and lg.dim() == 4
            and lg.shape[1] == self.cfg.MODEL.NUM_CLASSES and lg.shape[0] == x.shape[0]):
        return None
    return lg


def _criterion_args(self):
    neg = getattr(self, "negative_criterion", None)
    return {"ignore_index": int(self.criterion.ignore_index), "negative_threshold": float(getattr(neg, "threshold", 0.05))}


def _log(self, name, value):
    self.log(name, value.item(), on_step=True, on_epoch=False, sync_dist=True, prog_bar=True)


def _finish_step(self, optimizers, loss, batch_idx):
    self.log('loss', loss.item(), on_step=True, on_epoch=False, sync_dist=True, prog_bar=True)
    self.log_metrics(batch_idx)
    self.manual_backward(loss)
    for opt in optimizers:
        opt.step()
    for sched in self.lr_schedulers():
        sched.step()


def fused_training_step(self, batch, batch_idx):
    from .core.models.classifier import device_resize
    from .training import upsampled_losses
    proto = _training_protocol(type(self))
    if proto is None:
        raise TypeError("fused_training_step: %s derives from none of %s" % (type(self).__name__, ", ".join(_PROTOCOLS)))
    kw = _criterion_args(self)
    optimizers = self.optimizers()
    for opt in optimizers:
        opt.zero_grad()

    if proto == "SourceLearner":
        src_input, src_label = batch['img'], batch['label']
        src_lg = _head_logits(self, src_input)
        if src_lg is None:
            return self._reference_training_step(batch, batch_idx)
        loss = upsampled_losses(src_lg, src_label, size=src_input.shape[-2:], negative=False, **kw).ce
        self.log('loss', loss.item(), on_step=True, on_epoch=False, sync_dist=True, prog_bar=True)
        self.log_metrics(batch_idx)
        self.manual_backward(loss)
        for opt in optimizers:
            opt.step()
        for sched in self.lr_schedulers():
            sched.step()
        return loss

    neg_w = self.cfg.SOLVER.NEGATIVE_LOSS
    if proto == "SourceFreeLearner":
        tgt_input, tgt_mask = batch['img'], batch['mask']
        tgt_lg = _head_logits(self, tgt_input)
        if tgt_lg is None:
            return self._reference_training_step(batch, batch_idx)
        tgt = upsampled_losses(tgt_lg, tgt_mask, size=tgt_input.shape[-2:], negative=neg_w > 0, **kw)
        loss = torch.Tensor([0]).cuda()
        if int(tgt.n_labelled) != 0:                 # torch.sum(tgt_mask != 255) != 0; a label outside [0, K) raised above
            loss_sup = tgt.ce
            loss += loss_sup
            _log(self, 'loss_sup', loss_sup)
        if neg_w > 0:
            negative_loss = tgt.nl * neg_w
            loss += negative_loss
            _log(self, 'negative_loss', negative_loss)
        _finish_step(self, optimizers, loss, batch_idx)
        return None

    # SourceTargetLearner / FullySupervisedLearner: a source batch and a target batch
    src_input, src_label = batch[0]['img'], batch[0]['label']
    src_lg = _head_logits(self, src_input)
    if src_lg is None:
        return self._reference_training_step(batch, batch_idx)
    supervised = proto == "FullySupervisedLearner"
    tgt_input, tgt_label = batch[1]['img'], batch[1]['label' if supervised else 'mask']
    tgt_lg = _head_logits(self, tgt_input)
    if tgt_lg is None:
        return self._reference_training_step(batch, batch_idx)
    src = upsampled_losses(src_lg, src_label, size=src_input.shape[-2:], negative=False, **kw)
    tgt = upsampled_losses(tgt_lg, tgt_label, size=tgt_input.shape[-2:], negative=neg_w > 0, **kw)
    loss = torch.Tensor([0]).cuda()
    loss_sup = src.ce
    loss += loss_sup
    _log(self, 'loss_sup', loss_sup)
    if supervised or int(tgt.n_labelled) != 0:
        loss_sup_tgt = tgt.ce
        loss += loss_sup_tgt
        _log(self, 'loss_sup_tgt', loss_sup_tgt)
    if self.cfg.SOLVER.CONSISTENT_LOSS > 0:
        resize = device_resize(self)                  # use_device_resize(learner_cls): the HIP resize with its atomic-free backward
        if resize is None:
            src_out = F.interpolate(src_lg, size=src_input.shape[-2:], mode="bilinear", align_corners=True)
        else:
            src_out = resize(src_lg, src_input.shape[-2:])
        consistency_loss = self.local_consistent_loss(src_out, src_label) * self.cfg.SOLVER.CONSISTENT_LOSS
        loss += consistency_loss
        _log(self, 'consistency_loss', consistency_loss)
    if neg_w > 0:
        negative_loss = tgt.nl * neg_w
        loss += negative_loss
        _log(self, 'negative_loss', negative_loss)
    _finish_step(self, optimizers, loss, batch_idx)
    return None


def use_fused_training_losses(learner_cls):
    """Replace the learner's training_step with fused_training_step.  Returns the class.  The class must derive from one of
    the reference's SourceLearner, SourceFreeLearner, SourceTargetLearner or FullySupervisedLearner (by name)."""
    if _training_protocol(learner_cls) is None:
        raise TypeError("use_fused_training_losses: %s derives from none of %s" % (learner_cls.__name__, ", ".join(_PROTOCOLS)))
    learner_cls._reference_training_step = _inherited(learner_cls, "training_step")
    learner_cls.training_step = fused_training_step
    return learner_cls


# ---------------------------------------------------------------- the optimiser step in one HIP pass per param group
# configure_optimizers (core/train_learners.py:167-208) builds two geoopt RiemannianSGD instances with MODEL.HYPER (two
# torch.optim.SGD without) and their schedulers; the learners' steps then call opt.step() on each.  geoopt's step is a Python loop
# of eight tensor statements per parameter.  `use_fused_optimizer_step(learner_cls)` binds a configure_optimizers that calls the
# inherited one and passes every optimiser it returns through halo_amd.optim.fuse_step: the same objects, so the schedulers --
# returned untouched -- and Lightning's bookkeeping keep pointing at them.  What fuse_step does not serve keeps its stock step.

def _fuse_configured(configured):
    """fuse_step on every optimiser of a configure_optimizers result, in any of the shapes Lightning accepts: one optimiser, a
    list / tuple of them, the (optimisers, schedulers) pair, a dict or dicts with an "optimizer" key"""
    from .optim import fuse_step
    if isinstance(configured, torch.optim.Optimizer):
        return fuse_step(configured)
    if isinstance(configured, dict):
        if isinstance(configured.get("optimizer"), torch.optim.Optimizer):
            fuse_step(configured["optimizer"])
        return configured
    if isinstance(configured, (list, tuple)):
        if len(configured) == 2 and isinstance(configured[0], (list, tuple)):
            _fuse_configured(configured[0])                          # (optimisers, schedulers): the schedulers stay as they are
        else:
            for item in configured:
                _fuse_configured(item)
    return configured


def fused_configure_optimizers(self):
    return _fuse_configured(type(self)._unfused_configure_optimizers(self))


def use_fused_optimizer_step(learner_cls):
    """Bind fused_configure_optimizers on a learner class: the inherited configure_optimizers runs as before and every optimiser
    it returns is converted by halo_amd.optim.fuse_step.  Returns the class; the method it replaced is kept as
    `_unfused_configure_optimizers`.  Idempotent."""
    if not isinstance(learner_cls, type) or _inherited(learner_cls, "configure_optimizers") is None:
        raise TypeError("use_fused_optimizer_step: %r is not a class with a configure_optimizers method" % (learner_cls,))
    if _inherited(learner_cls, "configure_optimizers") is fused_configure_optimizers:      # bound here or on a base already
        return learner_cls
    learner_cls._unfused_configure_optimizers = _inherited(learner_cls, "configure_optimizers")
    learner_cls.configure_optimizers = fused_configure_optimizers
    return learner_cls


# ---------------------------------------------------------------- HFR weighted normalisation of the v3+ head
# With cfg.MODEL.HFR the DeepLab-v3+ hyperbolic head runs the `wn_mlp` weighted normalisation between conv_reduce and
# mapper.expmap (core/models/classifier.py:529-550), as torch statements.  `use_fused_feature_reweighting(head_cls)` binds
# `fused_v3plus_hyper_forward`: halo_amd.core.models.classifier.v3plus_hyper_forward with that statement replaced by
# halo_amd.hfr.weighted_normalize (halo_hfr.hip, which keeps the torch statement outside its envelope).  The previous forward is
# kept as `_unfused_forward`.  Neither install() nor the existing forward changes.

def fused_v3plus_hyper_forward(self, x, size=None):
    from .core.models.classifier import _tail_modules, pooled_aspp_pyramid, broadcast_or_resize, device_resize, folded_pooling, hyper_head_tail, v3plus_decoder
    from .hfr import weighted_normalize
    low, top = x["low"], x["out"]
    pyramid, pooled = pooled_aspp_pyramid(self, top)
    resize = device_resize(self)
    if folded_pooling(self, pooled):
        dec = v3plus_decoder(self, pyramid, low, resize, pooled=pooled)
    else:
        if resize is None:
            pyramid.append(F.interpolate(pooled, size=top.shape[2:], mode="bilinear", align_corners=True))
        else:
            pyramid.append(broadcast_or_resize(pooled, top.shape[2:], resize))
        dec = v3plus_decoder(self, pyramid, low, resize)
    dec = self.conv_reduce(dec)
    if getattr(self, "wn_mlp", None) is not None:
        dec = weighted_normalize(dec, self.wn_mlp)
    mapper, seg = _tail_modules(self)
    return hyper_head_tail(dec, mapper, seg, size=size, resize_embed=False, resize=resize)


def use_fused_feature_reweighting(head_cls):
    """Bind fused_v3plus_hyper_forward on a DeepLab-v3+ hyperbolic head class (the reference's DepthwiseSeparableASPP_Hyper or
    halo_amd's drop-in).  Returns the class; the forward it replaced is kept as `_unfused_forward`.  A class that carries
    v3plus_forward (use_v3plus_forward: the Euclidean head, which has no conv_seg) keeps that forward and gets a class mark that it
    reads: its wn_mlp statement then runs halo_amd.hfr.weighted_normalize."""
    from .core.models.classifier import v3plus_forward
    if isinstance(head_cls, type) and _inherited(head_cls, "forward") is v3plus_forward:
        head_cls._halo_fused_feature_reweighting = True
        return head_cls
    if head_cls.__dict__.get("forward") is fused_v3plus_hyper_forward:
        return head_cls
    head_cls._unfused_forward = _inherited(head_cls, "forward")
    head_cls.forward = fused_v3plus_hyper_forward
    return head_cls


# ---------------------------------------------------------------- resizes of the training paths on the device operator
# Under training every align_corners resize of the package's forwards is an F.interpolate, whose device backward scatters float
# atomic adds: the one source of run-to-run differences in a step's gradients.  `use_device_resize(cls)` marks a head class (one that
# carries v2_hyper_forward, v3plus_hyper_forward, fused_v3plus_hyper_forward or v3plus_forward) or a learner class (fused_training_step's
# LocalConsistentLoss input): marked classes resize through halo_amd.resize.resize_or_interpolate -- halo_bilinear_upsample forward,
# its gather adjoint backward -- and broadcast the v3+ head's 1 x 1 global-pooling branch.  Nothing changes for an unmarked class.

def _package_forwards():
    """the v2 forward, then the v3+ ones"""
    from .core.models.classifier import v2_hyper_forward, v3plus_forward, v3plus_hyper_forward
    return (v2_hyper_forward, v3plus_hyper_forward, fused_v3plus_hyper_forward, v3plus_forward)


def use_device_resize(cls):
    """Mark a head class or a learner class so that its training-path resizes run on halo_amd.resize.  Returns the class.
    Composes with the other hooks in either order (the mark is a class attribute, the forwards read it when they run)."""
    if not isinstance(cls, type):
        raise TypeError("use_device_resize: expected a class, got %r" % (cls,))
    if _training_protocol(cls) is None and not any(_inherited(cls, "forward") is f for f in _package_forwards()):
        raise TypeError("use_device_resize: %s is neither a learner (%s) nor a head class that carries one of halo_amd's forwards; "
                        "bind one first with halo_amd.install(), use_fused_feature_reweighting or use_v3plus_forward"
                        % (cls.__name__, ", ".join(_PROTOCOLS)))
    cls._halo_device_resize = True
    return cls


# ---------------------------------------------------------------- depthwise conv + frozen norm + ReLU of the separable blocks
# The five DepthwiseSeparableConv2d blocks of the v3+ heads (core/models/classifier.py:40-85: parallel_branches[1..3], decoder[0],
# decoder[1]) start with a depthwise 3x3 conv, a FrozenBatchNorm2d and a ReLU: four bandwidth-bound passes over tensors of 200 MB.
# `use_fused_depthwise(block_cls)` binds `fused_dwsep_forward`: halo_amd.dwconv.depthwise_bn_relu (halo_dwconv.hip, which keeps the
# stock statements outside its envelope) and then the three pointwise modules unchanged.  The hook sits on the BLOCK class, so it
# composes with install(), use_fused_feature_reweighting and use_device_resize in any order and serves the non-hyper
# DepthwiseSeparableASPP as well.  The previous forward is kept as `_unfused_forward`.  install() does not bind it.

_DWSEP_ATTRS = ("depthwise_conv", "depthwise_bn", "depthwise_activate", "pointwise_conv", "pointwise_bn", "pointwise_activate")


def _autocast_depthwise(block, x):
    """a block of a class marked by use_autocast_depthwise, under torch.autocast, where halo_amd.dwconv.autocast_fallback_reason
    holds: its depthwise half from halo_amd.dwconv.depthwise_bn_relu_autocast (half, what autocast's cast would hand pointwise_conv);
    None otherwise"""
    if not getattr(type(block), "_halo_autocast_depthwise", False) or type(block.depthwise_activate) is not torch.nn.ReLU:
        return None
    from .dwconv import autocast_fallback_reason, depthwise_bn_relu_autocast
    if autocast_fallback_reason(x, block.depthwise_conv, block.depthwise_bn) is not None:
        return None
    return depthwise_bn_relu_autocast(x, block.depthwise_conv, block.depthwise_bn, block.depthwise_activate)


def fused_dwsep_forward(self, x):
    from .dwconv import depthwise_bn_relu, torch_statement
    half = _autocast_depthwise(self, x)
    if half is not None:
        return pointwise_tail(self, half)
    if type(self.depthwise_activate) is torch.nn.ReLU:
        x = depthwise_bn_relu(x, self.depthwise_conv, self.depthwise_bn, self.depthwise_activate,
                              joint_backward=getattr(type(self), "_halo_joint_depthwise_backward", False))
    else:
        x = torch_statement(x, self.depthwise_conv, self.depthwise_bn, self.depthwise_activate)
    return pointwise_tail(self, x)


def _is_dwsep_class(cls):
    """the reference's DepthwiseSeparableConv2d (by name), or an nn.Module class whose instances carry the six attributes: they are
    class attributes, or the __init__ methods of the class assign them (read off the code objects: nothing is constructed)"""
    if not isinstance(cls, type) or not issubclass(cls, torch.nn.Module):
        return False
    if any(k.__name__ == "DepthwiseSeparableConv2d" for k in cls.__mro__):
        return True
    names = set()
    for klass in cls.__mro__:
        init = klass.__dict__.get("__init__")
        names.update(getattr(getattr(init, "__code__", None), "co_names", ()))
    return all(hasattr(cls, a) or a in names for a in _DWSEP_ATTRS)


def use_fused_depthwise(block_cls):
    """Bind fused_dwsep_forward on a depthwise-separable block class (the reference's DepthwiseSeparableConv2d, or any nn.Module
    class whose instances carry depthwise_conv, depthwise_bn, depthwise_activate, pointwise_conv, pointwise_bn,
    pointwise_activate).  Returns the class; the forward it replaced is kept as `_unfused_forward`.  Idempotent."""
    if not _is_dwsep_class(block_cls):
        raise TypeError("use_fused_depthwise: %r is not a depthwise-separable block class (instances with %s)"
                        % (block_cls, ", ".join(_DWSEP_ATTRS)))
    if block_cls.__dict__.get("forward") is fused_dwsep_forward:
        return block_cls
    block_cls._unfused_forward = _inherited(block_cls, "forward")
    block_cls.forward = fused_dwsep_forward
    return block_cls


# ---------------------------------------------------------------- the same half under torch.autocast
# precision=16 runs the heads under torch.autocast, where depthwise_bn_relu steps aside ("autocast is enabled") and the stock chain
# makes six passes.  `use_autocast_depthwise(block_cls)` marks a class that use_fused_depthwise has bound: under autocast, where
# halo_amd.dwconv.autocast_fallback_reason holds, fused_dwsep_forward and depthwise_half run
# halo_amd.dwconv.depthwise_bn_relu_autocast -- float32 or half in, half out -- and hand its result to pointwise_conv.  A mark of
# its own, not behaviour of use_fused_depthwise: the pass rounds every stage where the stock chain does, but its nine-term sums
# are the chain walk's, not the library's half conv's bits.  With autocast off a marked class does exactly what it did.  Not bound
# by install().  The decoder front, the LDS pyramid, the joint backward and the dropout tail keep stepping aside under autocast.

def use_autocast_depthwise(block_cls):
    """Mark a depthwise-separable block class under use_fused_depthwise so that its depthwise half runs
    halo_amd.dwconv.depthwise_bn_relu_autocast under torch.autocast.  Returns the class.  Idempotent.  TypeError for a class
    whose forward is not fused_dwsep_forward."""
    if not isinstance(block_cls, type) or _inherited(block_cls, "forward") is not fused_dwsep_forward:
        raise TypeError("use_autocast_depthwise: %r is not a class under use_fused_depthwise; bind that first" % (block_cls,))
    block_cls._halo_autocast_depthwise = True
    return block_cls


# ---------------------------------------------------------------- the front of the v3+ decoder in one pass
# Both v3+ forwards resize the bottleneck's output to the low-level map, concatenate it with the shortcut and hand the result to
# decoder[0], whose depthwise half reads it once: at the training crop a 210 MB and a 229 MB tensor that exist only to be read
# again.  `use_fused_decoder_front(head_cls)` marks a head class that carries one of the package's v3+ forwards; its instances run
# halo_amd.dwconv.upsample_cat_depthwise_bn_relu there (core.models.classifier.v3plus_decoder: the condition, the order of the
# module calls and the fallback).  A class attribute like use_device_resize's: opt-in, not bound by install(), composes with the
# other hooks in any order; parameters, module names and state_dict() are untouched.

def use_fused_decoder_front(head_cls):
    """Mark a v3+ head class (one that carries v3plus_hyper_forward, fused_v3plus_hyper_forward or v3plus_forward) so that the
    resize, the concat and the depthwise half of decoder[0] run as one HIP pass.  Returns the class.  Idempotent.  The marked head's results are
    those of the head under use_device_resize + use_fused_depthwise on that block, bit for bit -- not those of the stock
    F.interpolate / nn.Conv2d chain."""
    if not isinstance(head_cls, type):
        raise TypeError("use_fused_decoder_front: expected a class, got %r" % (head_cls,))
    if not any(_inherited(head_cls, "forward") is f for f in _package_forwards()[1:]):
        raise TypeError("use_fused_decoder_front: %s does not carry one of halo_amd's v3+ forwards; bind one first with "
                        "halo_amd.install(), use_fused_feature_reweighting or use_v3plus_forward" % head_cls.__name__)
    head_cls._halo_fused_decoder_front = True
    return head_cls


# ---------------------------------------------------------------- a separable block's two gradients from one backward pass
# The backward of a block's depthwise half is two passes over g, y and x: one for g_x, one for g_w.  `use_joint_depthwise_backward(cls)`
# marks a class so that a backward that wants every gradient of the node runs halo_joint_*_bwd instead (halo_amd.dwconv: the
# keyword joint_backward, the envelope and the speed rule JOINT_MIN_ELEMENTS, under which a route that did not win its timing is
# not served).  A class attribute like use_fused_decoder_front's: opt-in, not bound by install(), composes with the other hooks in any
# order; parameters, module names and state_dict() are untouched.

def use_joint_depthwise_backward(cls):
    """Mark a depthwise-separable block class (see use_fused_depthwise: fused_dwsep_forward reads the mark and passes it to
    depthwise_bn_relu as joint_backward) or a v3+ head class that carries v3plus_hyper_forward, fused_v3plus_hyper_forward or
    v3plus_forward (v3plus_decoder reads the mark for the front under use_fused_decoder_front).  Returns the class.  Idempotent.
    The mark alone binds no forward: a block class acts under use_fused_depthwise, a head class under use_fused_decoder_front.  A
    marked class returns the bits of the unmarked one: outputs, every input gradient and every parameter gradient.  Under
    use_fused_aspp_depthwise the three pyramid blocks run the pyramid pass and its weight-gradient calls as before; the mark then
    acts on the decoder blocks only."""
    if not isinstance(cls, type):
        raise TypeError("use_joint_depthwise_backward: expected a class, got %r" % (cls,))
    if not _is_dwsep_class(cls) and not any(_inherited(cls, "forward") is f for f in _package_forwards()[1:]):
        raise TypeError("use_joint_depthwise_backward: %s is neither a depthwise-separable block class (instances with %s) nor a head "
                        "class that carries one of halo_amd's v3+ forwards" % (cls.__name__, ", ".join(_DWSEP_ATTRS)))
    cls._halo_joint_depthwise_backward = True
    return cls


# ---------------------------------------------------------------- the ASPP pyramid's dilated depthwise halves in one pass each way
# Both v3+ forwards hand the backbone's output to parallel_branches, three of which are dilated separable blocks whose depthwise
# halves each read it, and whose backward each write a gradient of its size that the autograd engine then adds.
# `use_fused_aspp_depthwise(head_cls)` marks a head class that carries one of the package's v3+ forwards; its instances run such
# neighbours' depthwise halves as halo_amd.dwconv.multi_depthwise_bn_relu (core.models.classifier.aspp_pyramid: the conditions and
# the fallback).  A class attribute like use_fused_decoder_front's: opt-in, not bound by install(), composes with the other hooks
# in any order; parameters, module names and state_dict() are untouched.  It acts on blocks under use_fused_depthwise only.

def use_fused_aspp_depthwise(head_cls):
    """Mark a v3+ head class (one that carries v3plus_hyper_forward, fused_v3plus_hyper_forward or v3plus_forward) so that
    consecutive dilated separable blocks of parallel_branches under use_fused_depthwise run their depthwise halves as one HIP pass
    forward and one for the input gradient.  Returns the class.  Idempotent.  The marked head returns the bits of the same head
    under use_fused_depthwise alone: both outputs and every parameter gradient.  Only the gradient of the backbone's output is not
    bit-equal: the pass adds the blocks' shares first and the engine adds the remaining branches' onto that, another association
    of the same float32 terms t_i -- two summation orders of five terms differ by at most 2 gamma_4 sum |t_i|, gamma_4 =
    4u / (1 - 4u), u = 2^-24."""
    if not isinstance(head_cls, type):
        raise TypeError("use_fused_aspp_depthwise: expected a class, got %r" % (head_cls,))
    if not any(_inherited(head_cls, "forward") is f for f in _package_forwards()[1:]):
        raise TypeError("use_fused_aspp_depthwise: %s does not carry one of halo_amd's v3+ forwards; bind one first with "
                        "halo_amd.install(), use_fused_feature_reweighting or use_v3plus_forward" % head_cls.__name__)
    head_cls._halo_fused_aspp_depthwise = True
    return head_cls


# ---------------------------------------------------------------- the backbone output's five gradients added in one pass
# Under use_fused_aspp_depthwise the dilated blocks' share of the backbone output's gradient is written once; the 1 x 1 branch's and
# global_branch's shares are still joined to it by the engine: a full-size broadcast of one value per plane (MeanBackward1) and two
# full-size adds.  `use_joined_aspp_gradients(head_cls)` marks a head class that carries one of the package's v3+ forwards; on a
# class that use_fused_aspp_depthwise has marked as well, the first served run of dilated blocks runs as
# halo_amd.fanout.fan_depthwise_bn_relu, whose backward adds the other readers' gradients where the run's sum leaves LDS
# (core.models.classifier.pooled_aspp_pyramid: the conditions and the fallback).  A class attribute like use_fused_aspp_depthwise's:
# opt-in, not bound by install(), composes with the other hooks in any order; parameters, module names and state_dict() are untouched.

def use_joined_aspp_gradients(head_cls):
    """Mark a v3+ head class (one that carries v3plus_hyper_forward, fused_v3plus_hyper_forward or v3plus_forward) so that the
    gradient of the backbone's output is written once, by the pass that adds the dilated blocks' shares: the other parallel
    branches' and global_branch's gradients join it there, the latter as one value per plane.  Acts on heads that
    use_fused_aspp_depthwise marks too.  Returns the class.  Idempotent.  The marked head returns the bits of the same head under
    use_fused_aspp_depthwise alone: both outputs and every parameter gradient.  Only the gradient of the backbone's output is
    another association of the same five float32 terms t_i (the blocks' shares first, then the others in branch order), within
    2 gamma_4 sum |t_i| of any other, the bound use_fused_aspp_depthwise documents."""
    if not isinstance(head_cls, type):
        raise TypeError("use_joined_aspp_gradients: expected a class, got %r" % (head_cls,))
    if not any(_inherited(head_cls, "forward") is f for f in _package_forwards()[1:]):
        raise TypeError("use_joined_aspp_gradients: %s does not carry one of halo_amd's v3+ forwards; bind one first with "
                        "halo_amd.install(), use_fused_feature_reweighting or use_v3plus_forward" % head_cls.__name__)
    head_cls._halo_joined_aspp_gradients = True
    return head_cls


# ---------------------------------------------------------------- the image-pooling branch folded into the bottleneck's epilogue
# The last Cg of the bottleneck conv's input channels are global_branch's output, one value per (image, channel) broadcast over the
# map: a fifth of the largest convolution of the v3+ heads runs over constant planes.  `use_folded_image_pooling(head_cls)` marks a
# head class that carries one of the package's v3+ forwards; its instances hand the 1 x 1 map to the bottleneck stage without
# broadcasting it and run halo_amd.aspp.pooled_bottleneck there (core.models.classifier.v3plus_bottleneck: the condition and the
# fallback).  A class attribute like use_fused_decoder_front's: opt-in, not bound by install(), composes with the other hooks in
# any order; parameters, module names and state_dict() are untouched.

def use_folded_image_pooling(head_cls):
    """Mark a v3+ head class (one that carries v3plus_hyper_forward, fused_v3plus_hyper_forward or v3plus_forward) so that the
    bottleneck's conv runs over the parallel branches alone and the pooled branch enters its norm + ReLU pass as a border-aware bias.  Returns the
    class.  Idempotent.  The marked head's results are not the stock chain's bits: the pooled channels' share is summed in float64
    and rounded once."""
    if not isinstance(head_cls, type):
        raise TypeError("use_folded_image_pooling: expected a class, got %r" % (head_cls,))
    if not any(_inherited(head_cls, "forward") is f for f in _package_forwards()[1:]):
        raise TypeError("use_folded_image_pooling: %s does not carry one of halo_amd's v3+ forwards; bind one first with "
                        "halo_amd.install(), use_fused_feature_reweighting or use_v3plus_forward" % head_cls.__name__)
    head_cls._halo_folded_image_pooling = True
    return head_cls


# ---------------------------------------------------------------- frozen norm + residual add + ReLU of the backbone and the heads
# With MODEL.FREEZE_BN every norm of the ResNet backbone and every dense norm of the heads is a FrozenBatchNorm2d whose forward is
# torch statements (core/models/layers.py): a broadcast mul and a broadcast add over the activation, then an in-place ReLU, and at
# the end of a residual block an in-place `out += identity` and another ReLU.  halo_amd.norm.norm_relu (halo_norm.hip) runs each
# such chain as one pass with the chain's own roundings, so a hooked model returns the unhooked model's bits.  Four opt-in hooks,
# none bound by install():
#   use_fused_frozen_norm(block_cls)   class level: the two residual blocks of core/models/resnet.py (Bottleneck, BasicBlock);
#   fuse_residual_chains(module)       instance level: the nn.Sequential layers of such blocks; a block output that the next block
#                                      reads twice takes its two gradients in the tail's own backward pass (norm_relu_fork);
#   fuse_norm_relu_pairs(module)       instance level: (FrozenBatchNorm2d, nn.ReLU) neighbours that a container calls in sequence --
#                                      the stem inside the feature extractor's IntermediateLayerGetter, the v3+ heads'
#                                      parallel_branches[0], global_branch, bottleneck and shortcut.
#   fuse_norm_relu_pool(module)        instance level: (FrozenBatchNorm2d, nn.ReLU, nn.MaxPool2d(3, 2, 1)) neighbours, i.e. the stem with
#                                      its pool, as halo_amd.norm.norm_relu_maxpool (halo_maxpool.hip); upgrades a fused pair.
# The separable blocks' pointwise_bn + pointwise_activate, and the nn.Dropout2d behind the hyperbolic head's decoder[1], have hooks
# of their own further down (use_fused_pointwise_norm, use_fused_decoder_dropout): they act on the second half of a block alone, so
# they compose with use_fused_depthwise, whose first half is not bit-equal to the stock depthwise conv, without changing its bits.

_RESIDUAL_ATTRS = ("conv1", "bn1", "conv2", "bn2", "relu", "downsample")


def _norm_relu_either(x, bn, residual=None, residual_bn=None, outputs="float"):
    """halo_amd.norm.norm_relu_autocast where its envelope holds (under torch.autocast, x the half a convolution returned: "half"
    hands the next convolution what autocast's cast would), halo_amd.norm.norm_relu otherwise"""
    from .norm import autocast_fallback_reason, norm_relu, norm_relu_autocast
    if autocast_fallback_reason(x, bn, residual, residual_bn, outputs) is None:
        return norm_relu_autocast(x, bn, residual, residual_bn, outputs)
    return norm_relu(x, bn, residual, residual_bn)


def residual_body(self, x, identity, fork):
    """a residual block on input x with `identity` as what a block without a downsample adds (x itself, or the second tensor of a
    forked predecessor: the same values); returns (y, y_id), the output twice -- halo_amd.norm.norm_relu_fork's pair when `fork`,
    the same tensor object otherwise.  Under torch.autocast, where halo_amd.norm.norm_relu_autocast serves them, the results of bn1
    and bn2, which a convolution alone reads, are half inside the block; its output is the stock model's float32."""
    return _residual_body(self, x, identity, fork, False)


def _residual_body(self, x, identity, fork, half_fork):
    """residual_body; half_fork: the successor is a bound block, which reads its input with conv1 and, as `identity`, with its tail or
    its downsample.  Under torch.autocast, where halo_amd.norm.norm_relu_autocast serves the tail, return (y16, y32) from that
    operator's two-output node: y16 what autocast's cast of y32 would hand conv1, y32 the block's output as the stock model has it.
    y16 has that one reader: a second convolution on it would have the engine add two gradients in half, where the stock model,
    which casts once per convolution, adds them in float32 -- so a downsample reads `identity` and autocast casts it as before."""
    from .norm import autocast_fallback_reason, norm_relu_autocast, norm_relu_fork
    if type(self.relu) is not torch.nn.ReLU:
        y = self._unfused_forward(x)
        return y, y
    out = _norm_relu_either(self.conv1(x), self.bn1, outputs="half")
    if getattr(self, "conv3", None) is not None:             # the Bottleneck form
        out = _norm_relu_either(self.conv2(out), self.bn2, outputs="half")
        out, last = self.conv3(out), self.bn3
    else:                                                    # the BasicBlock form
        out, last = self.conv2(out), self.bn2
    down = self.downsample
    if down is None:
        residual, residual_bn = identity, None
    elif _is_conv_norm(down):
        residual, residual_bn = down[0](identity), down[1]   # the downsample norm is folded into the pass
    else:
        residual, residual_bn = down(identity), None
    if half_fork and autocast_fallback_reason(out, last, residual, residual_bn, "both") is None:
        y32, y16 = norm_relu_autocast(out, last, residual, residual_bn, outputs="both")
        return y16, y32
    if fork:
        return norm_relu_fork(out, last, residual=residual, residual_bn=residual_bn)
    y = _norm_relu_either(out, last, residual, residual_bn)
    return y, y


def _is_conv_norm(down):
    """a downsample of the form nn.Sequential(conv, norm)"""
    return type(down) is torch.nn.Sequential and len(down) == 2 and isinstance(down[0], torch.nn.Conv2d)


def fused_residual_forward(self, x):
    return residual_body(self, x, x, False)[0]


def _is_residual_class(cls):
    """the reference's Bottleneck / BasicBlock (by name), or an nn.Module class whose instances carry conv1, bn1, conv2, bn2, relu
    and downsample (class attributes, or names its __init__ methods assign: nothing is constructed)"""
    if not isinstance(cls, type) or not issubclass(cls, torch.nn.Module):
        return False
    if any(k.__name__ in ("Bottleneck", "BasicBlock") for k in cls.__mro__):
        return True
    names = set()
    for klass in cls.__mro__:
        init = klass.__dict__.get("__init__")
        names.update(getattr(getattr(init, "__code__", None), "co_names", ()))
    return all(hasattr(cls, a) or a in names for a in _RESIDUAL_ATTRS)


def use_fused_frozen_norm(block_cls):
    """Bind fused_residual_forward on a residual block class of the Bottleneck form (conv1, bn1, conv2, bn2, conv3, bn3, relu,
    downsample) or the BasicBlock form (the same without conv3 / bn3).  Returns the class; the forward it replaced is kept as
    `_unfused_forward` and serves a block whose `relu` is not nn.ReLU.  Idempotent."""
    if not _is_residual_class(block_cls):
        raise TypeError("use_fused_frozen_norm: %r is not a residual block class (instances with %s)" % (block_cls, ", ".join(_RESIDUAL_ATTRS)))
    if block_cls.__dict__.get("forward") is fused_residual_forward:
        return block_cls
    block_cls._unfused_forward = _inherited(block_cls, "forward")
    block_cls.forward = fused_residual_forward
    return block_cls


def _forks_into(block):
    """a block in front of `block` may hand it a forked output: it reads its input as conv1(x) and as the identity"""
    return block.downsample is None and type(block.relu) is torch.nn.ReLU


class _ChainWalk:
    """the call of an nn.Sequential of bound residual blocks: block i + 1 reads block i's output twice, as conv1's input and as its
    identity, so block i returns it twice from one autograd node (halo_amd.norm.norm_relu_fork) and both gradients arrive at that
    node's backward, which adds them in its own pass"""

    def __init__(self, box):
        self.box = box

    def __call__(self, x):
        from torch.nn.modules import module as M
        from .norm import _autocast_dtype
        box = self.box
        blocks = list(box._modules.values())
        hooked = any(b._forward_hooks or b._forward_pre_hooks for b in blocks) or bool(
            getattr(M, "_global_forward_hooks", None) or getattr(M, "_global_forward_pre_hooks", None))
        if hooked or not _chain_blocks(box):                 # hooks fire in __call__, which the walk does not go through
            return torch.nn.Sequential.forward(box, x)
        identity = x
        for i, block in enumerate(blocks):
            inner = type(block.relu) is torch.nn.ReLU and i + 1 < len(blocks)
            fork = inner and _forks_into(blocks[i + 1])
            # under torch.autocast a bound successor with an nn.ReLU takes (half, float32): residual_body reads the first with conv1
            # alone and the second as the identity or with the downsample
            if inner and _autocast_dtype() is not None and type(blocks[i + 1].relu) is torch.nn.ReLU:
                x, identity = _residual_body(block, x, identity, fork, True)
            else:
                x, identity = residual_body(block, x, identity, fork)
        return x


def _chain_blocks(box):
    """the children of a container that fuse_residual_chains serves (None: it does not): two or more, every one of a class bound by
    use_fused_frozen_norm, none with an instance-level forward"""
    blocks = list(box._modules.values())
    if len(blocks) < 2:
        return None
    for b in blocks:
        if b is None or getattr(type(b), "forward", None) is not fused_residual_forward or "forward" in b.__dict__:
            return None
    return blocks


def fuse_residual_chains(module):
    """Give every nn.Sequential under `module` (itself included) that holds two or more residual blocks, all of classes bound by
    use_fused_frozen_norm, and nothing else, an instance-level `forward` that walks its blocks: a block whose successor has no
    downsample (and an nn.ReLU) ends in halo_amd.norm.norm_relu_fork, the successor runs conv1 on one of the two tensors and adds the
    other, and the two gradients that come back are added inside the first block's tail backward instead of by a kernel of the
    engine's.  A block in front of a downsample, and the last block, end in norm_relu as before.  Outputs and gradients are the
    unchained model's bits.  No module is added, removed or renamed: state_dict() and named_modules() are unchanged.  A container
    that already carries an instance-level `forward`, or whose children do not qualify, is left alone.

    The walk calls the blocks' bodies, not their `__call__`: while any block of a container carries a forward hook or a forward
    pre-hook (or a global module forward hook is registered), or its children have changed so that they no longer qualify, a call of
    that container runs nn.Sequential.forward, blocks, hooks and all, without the chaining.  Returns the number of containers bound
    (0 on a second call); unfuse_residual_chains(module) undoes it."""
    n = 0
    for box in module.modules():
        if isinstance(box, torch.nn.Sequential) and "forward" not in box.__dict__ and _chain_blocks(box) is not None:
            box.forward = _ChainWalk(box)
            n += 1
    return n


def unfuse_residual_chains(module):
    """Undo fuse_residual_chains(module).  Returns the number of containers restored."""
    n = 0
    for m in module.modules():
        if isinstance(m.__dict__.get("forward"), _ChainWalk):
            del m.__dict__["forward"]
            n += 1
    return n


class _PairNorm:
    """the call of a norm whose next sibling is a ReLU: relu(norm(x)) in one pass"""

    def __init__(self, norm):
        self.norm = norm

    def __call__(self, x):
        from .norm import autocast_fallback_reason, fallback_reason, fused_norm_relu, norm_relu_autocast
        norm = self.norm
        if autocast_fallback_reason(x, norm) is None:      # under torch.autocast: float32 out, a container's reader is not known
            return norm_relu_autocast(x, norm)
        if fallback_reason(x, norm) is not None:
            return F.relu(type(norm).forward(norm, x), inplace=True)
        return fused_norm_relu(x, norm)


class _PairRelu:
    """the call of the ReLU behind such a norm: its input is already rectified"""

    def __call__(self, x):
        return x


def _pair_containers(module):
    for m in module.modules():
        if isinstance(m, torch.nn.Sequential) or (isinstance(m, torch.nn.ModuleDict) and type(m).__name__ == "IntermediateLayerGetter"):
            yield m


def fuse_norm_relu_pairs(module):
    """In every nn.Sequential and every IntermediateLayerGetter (an nn.ModuleDict subclass of that name) under `module`, make each
    FrozenBatchNorm2d child whose next sibling is an nn.ReLU return halo_amd.norm.norm_relu(x, norm) and that ReLU return its
    input.  Both get an instance-level `forward`; no module is added, removed or renamed, so state_dict(), named_modules() and a
    checkpoint loaded afterwards are unaffected.  A norm or a ReLU object that `module` holds in more than one place, and a norm
    whose output the container returns (IntermediateLayerGetter.return_layers), is left alone.  Returns the number of pairs
    fused (0 on a second call); unfuse_norm_relu_pairs(module) undoes it."""
    from .dwconv import _is_frozen
    uses = {}
    for m in module.modules():
        for child in m._modules.values():
            if child is not None:
                uses[id(child)] = uses.get(id(child), 0) + 1
    fused = 0
    for box in _pair_containers(module):
        kept = getattr(box, "return_layers", None) or {}
        items = [(n, c) for n, c in box._modules.items() if c is not None]
        for (name, norm), (_, act) in zip(items, items[1:]):
            if not _is_frozen(norm) or type(act) is not torch.nn.ReLU or name in kept:
                continue
            if uses[id(norm)] != 1 or uses[id(act)] != 1 or "forward" in norm.__dict__ or "forward" in act.__dict__:
                continue
            norm.forward, act.forward = _PairNorm(norm), _PairRelu()
            fused += 1
    return fused


def unfuse_norm_relu_pairs(module):
    """Undo fuse_norm_relu_pairs(module).  Returns the number of pairs restored."""
    n = 0
    for m in module.modules():
        f = m.__dict__.get("forward")
        if isinstance(f, (_PairNorm, _PairRelu)):
            del m.__dict__["forward"]
            n += isinstance(f, _PairNorm)
    return n


class _PoolNorm:
    """the call of a norm whose next siblings are a ReLU and the stem's max-pool: pool(relu(norm(x))) in one pass"""

    def __init__(self, norm, act, pool):
        self.norm, self.act, self.pool = norm, act, pool

    def __call__(self, x):
        from .norm import fallback_reason, fused_norm_relu, fused_norm_relu_maxpool, pool_fallback_reason
        norm, act, pool = self.norm, self.act, self.pool
        if pool_fallback_reason(x, norm, pool) is None:
            return fused_norm_relu_maxpool(x, norm)
        if fallback_reason(x, norm) is None:               # turned away by the triple's speed rule alone: the pair's pass, then the pool
            return type(pool).forward(pool, fused_norm_relu(x, norm))
        return type(pool).forward(pool, type(act).forward(act, type(norm).forward(norm, x)))


class _PoolPass:
    """the call of the ReLU and of the pool behind such a norm: their input is already rectified and pooled"""

    def __call__(self, x):
        return x


def fuse_norm_relu_pool(module):
    """In the containers fuse_norm_relu_pairs walks, make each FrozenBatchNorm2d child whose next two siblings are an nn.ReLU and an
    nn.MaxPool2d(3, 2, 1) (halo_amd.norm.pool_fallback_reason's pool) return halo_amd.norm.norm_relu_maxpool(x, norm, pool), and the
    ReLU and the pool return their input: the backbone's stem.  All three get an instance-level `forward`; no module is added,
    removed or renamed.  A (norm, ReLU) pair that fuse_norm_relu_pairs has fused is upgraded, and fuse_norm_relu_pairs afterwards
    leaves the triple alone.  Left alone: an object that `module` holds in more than one place, a norm or a ReLU whose output the
    container returns (IntermediateLayerGetter.return_layers; the pool's may be returned, it is the triple's), a foreign
    instance-level `forward`.  A call the fused pass does not serve (a CPU tensor) runs the three stock forwards.  Returns the
    number of triples fused (0 on a second call); unfuse_norm_relu_pool(module) undoes it."""
    from .dwconv import _is_frozen
    from .norm import _pool_reason
    uses = {}
    for m in module.modules():
        for child in m._modules.values():
            if child is not None:
                uses[id(child)] = uses.get(id(child), 0) + 1
    fused = 0
    for box in _pair_containers(module):
        kept = getattr(box, "return_layers", None) or {}
        items = [(n, c) for n, c in box._modules.items() if c is not None]
        for (name, norm), (act_name, act), (_, pool) in zip(items, items[1:], items[2:]):
            if not _is_frozen(norm) or type(act) is not torch.nn.ReLU or _pool_reason(pool) is not None or name in kept or act_name in kept:
                continue
            if uses[id(norm)] != 1 or uses[id(act)] != 1 or uses[id(pool)] != 1 or "forward" in pool.__dict__:
                continue
            mine, theirs = norm.__dict__.get("forward"), act.__dict__.get("forward")
            paired = isinstance(mine, _PairNorm) and isinstance(theirs, _PairRelu)
            if not paired and (mine is not None or theirs is not None):
                continue
            norm.forward, act.forward, pool.forward = _PoolNorm(norm, act, pool), _PoolPass(), _PoolPass()
            fused += 1
    return fused


def unfuse_norm_relu_pool(module):
    """Undo fuse_norm_relu_pool(module): the three modules of every triple run their class's forward again.  Returns the number of
    triples restored."""
    n = 0
    for m in module.modules():
        f = m.__dict__.get("forward")
        if isinstance(f, (_PoolNorm, _PoolPass)):
            del m.__dict__["forward"]
            n += isinstance(f, _PoolNorm)
    return n


# ---------------------------------------------------------------- the pointwise tail of the separable blocks, and the decoder's dropout
# The second half of every DepthwiseSeparableConv2d is the library's 1 x 1 conv, `pointwise_bn` (a FrozenBatchNorm2d: a broadcast
# mul and a broadcast add) and `pointwise_activate` (an in-place ReLU); behind decoder[1] the hyperbolic head adds nn.Dropout2d(0.1).
# Two opt-in marks, neither set by install(), both class attributes that the forwards read when they run:
#   use_fused_pointwise_norm(block_cls)    a marked block runs halo_amd.norm.norm_relu(pointwise_conv(x), pointwise_bn) -- in
#                                          fused_dwsep_forward, in v3plus_decoder's fused-front branch, and, on a class that
#                                          use_fused_depthwise has not bound, in fused_pointwise_forward (stock depthwise half);
#   use_fused_decoder_dropout(head_cls)    v3plus_decoder walks self.decoder itself and runs a marked separable block that is
#                                          directly followed by an nn.Dropout2d sibling together with it, as
#                                          halo_amd.norm.norm_relu_dropout2d (halo_masked_affine_relu_* of halo_norm.hip).
# Both passes return the stock statements' bits (norm_relu_dropout2d with nn.Dropout2d's use of the generator), so a marked class
# returns the unmarked class's bits, forward and backward.

def pointwise_tail(block, x):
    """the second half of a separable block from its depthwise half's output: the three pointwise modules, or -- on a class marked by
    use_fused_pointwise_norm whose pointwise_activate is an nn.ReLU -- the conv and halo_amd.norm.norm_relu (under torch.autocast,
    where its envelope holds, halo_amd.norm.norm_relu_autocast with the float32 output)"""
    x = block.pointwise_conv(x)
    if getattr(type(block), "_halo_fused_pointwise_norm", False) and type(block.pointwise_activate) is torch.nn.ReLU:
        return _norm_relu_either(x, block.pointwise_bn)      # under torch.autocast: norm_relu_autocast's float32, the stock chain's bits
    x = block.pointwise_bn(x)
    x = block.pointwise_activate(x)
    return x


def fused_pointwise_forward(self, x):
    x = self.depthwise_conv(x)
    x = self.depthwise_bn(x)
    x = self.depthwise_activate(x)
    return pointwise_tail(self, x)


def use_fused_pointwise_norm(block_cls):
    """Mark a depthwise-separable block class (see use_fused_depthwise) so that pointwise_bn + pointwise_activate run as one pass
    of halo_amd.norm.norm_relu.  Returns the class.  Idempotent; composes with use_fused_depthwise in either order.  A class whose
    forward is not fused_dwsep_forward gets fused_pointwise_forward, and the forward that replaces is kept as `_unfused_forward`."""
    if not _is_dwsep_class(block_cls):
        raise TypeError("use_fused_pointwise_norm: %r is not a depthwise-separable block class (instances with %s)"
                        % (block_cls, ", ".join(_DWSEP_ATTRS)))
    block_cls._halo_fused_pointwise_norm = True
    if _inherited(block_cls, "forward") not in (fused_dwsep_forward, fused_pointwise_forward):
        block_cls._unfused_forward = _inherited(block_cls, "forward")
        block_cls.forward = fused_pointwise_forward
    return block_cls


def use_fused_decoder_dropout(head_cls):
    """Mark a v3+ head class (one that carries v3plus_hyper_forward, fused_v3plus_hyper_forward or v3plus_forward) so that a
    separable block of its decoder marked by use_fused_pointwise_norm and the nn.Dropout2d directly behind it run their norm, ReLU and dropout as one pass
    (halo_amd.norm.norm_relu_dropout2d: the stock chain's bits and generator use).  Returns the class.  Idempotent."""
    if not isinstance(head_cls, type):
        raise TypeError("use_fused_decoder_dropout: expected a class, got %r" % (head_cls,))
    if not any(_inherited(head_cls, "forward") is f for f in _package_forwards()[1:]):
        raise TypeError("use_fused_decoder_dropout: %s does not carry one of halo_amd's v3+ forwards; bind one first with "
                        "halo_amd.install(), use_fused_feature_reweighting or use_v3plus_forward" % head_cls.__name__)
    head_cls._halo_fused_decoder_dropout = True
    return head_cls


def depthwise_half(block, x):
    """the first half of a separable block as the block's own class runs it: halo_amd.dwconv.depthwise_bn_relu under
    use_fused_depthwise, the three stock statements otherwise"""
    if _inherited(type(block), "forward") is fused_dwsep_forward and type(block.depthwise_activate) is torch.nn.ReLU:
        from .dwconv import depthwise_bn_relu
        half = _autocast_depthwise(block, x)
        if half is not None:
            return half
        return depthwise_bn_relu(x, block.depthwise_conv, block.depthwise_bn, block.depthwise_activate,
                                 joint_backward=getattr(type(block), "_halo_joint_depthwise_backward", False))
    return block.depthwise_activate(block.depthwise_bn(block.depthwise_conv(x)))


def run_decoder(head, dec, first_half_done=False):
    """head.decoder over dec.  An unmarked head, or a decoder that is no nn.Sequential, calls the container (or, behind the fused
    front, its modules in order) as before.  A head marked by use_fused_decoder_dropout walks the modules: a separable block marked
    by use_fused_pointwise_norm, with an nn.ReLU pointwise_activate and an nn.Dropout2d as its next sibling, runs its depthwise
    half, its 1 x 1 conv and norm_relu_dropout2d with that sibling; every other module is called.  first_half_done: dec is already
    the output of decoder[0]'s depthwise half (the fused front)."""
    decoder = head.decoder
    marked = getattr(type(head), "_halo_fused_decoder_dropout", False) and isinstance(decoder, torch.nn.Sequential)
    if not marked and not first_half_done:
        return decoder(dec)
    modules = list(decoder)
    i = 0
    while i < len(modules):
        m = modules[i]
        skip_front = first_half_done and i == 0
        nxt = modules[i + 1] if i + 1 < len(modules) else None
        pair = (marked and isinstance(nxt, torch.nn.Dropout2d) and getattr(type(m), "_halo_fused_pointwise_norm", False)
                and all(hasattr(m, a) for a in _DWSEP_ATTRS) and type(m.pointwise_activate) is torch.nn.ReLU
                and (skip_front or _inherited(type(m), "forward") in (fused_dwsep_forward, fused_pointwise_forward)))
        if pair:
            from .norm import norm_relu_dropout2d
            h = dec if skip_front else depthwise_half(m, dec)
            dec = norm_relu_dropout2d(m.pointwise_conv(h), m.pointwise_bn, nxt)
            i += 2
            continue
        dec = pointwise_tail(m, dec) if skip_front else m(dec)
        i += 1
    return dec


def run_decoder_pair(head, dec, first_half_done=False):
    """The old decoder layout of the Euclidean v3+ head, Sequential(block, block, Dropout2d, Conv2d), over dec (classifier.py:
    308-312): returns (decoder_out, out) -- decoder[1]'s output, and what the remaining modules make of it.  Unmarked, the walk is
    the reference's loop over the modules.  On a head class marked by use_fused_decoder_dropout, a decoder[1] that run_decoder
    would pair with its nn.Dropout2d sibling (a block marked by use_fused_pointwise_norm with an nn.ReLU pointwise_activate) runs
    its depthwise half, its 1 x 1 conv and halo_amd.norm.norm_relu_dropout2d_pair, whose first result is decoder_out and whose
    second goes on to decoder[3:].  first_half_done: as in run_decoder."""
    modules = list(head.decoder)
    marked = getattr(type(head), "_halo_fused_decoder_dropout", False) and isinstance(head.decoder, torch.nn.Sequential)
    dec = pointwise_tail(modules[0], dec) if first_half_done else modules[0](dec)
    m, nxt = modules[1], modules[2] if len(modules) > 2 else None
    pair = (marked and isinstance(nxt, torch.nn.Dropout2d) and getattr(type(m), "_halo_fused_pointwise_norm", False)
            and all(hasattr(m, a) for a in _DWSEP_ATTRS) and type(m.pointwise_activate) is torch.nn.ReLU
            and _inherited(type(m), "forward") in (fused_dwsep_forward, fused_pointwise_forward))
    if pair:
        from .norm import norm_relu_dropout2d_pair
        decoder_out, dec = norm_relu_dropout2d_pair(m.pointwise_conv(depthwise_half(m, dec)), m.pointwise_bn, nxt)
        rest = modules[3:]
    else:
        decoder_out = dec = m(dec)
        rest = modules[2:]
    for m in rest:
        dec = m(dec)
    return decoder_out, dec


# ---------------------------------------------------------------- the Euclidean DeepLab-v3+ head on the package's forward
# DepthwiseSeparableASPP (core/models/classifier.py:88-316) is the head of configs/gtav/ripu.yaml (HYPER False): the hyperbolic
# v3+ head's ASPP pyramid, bottleneck, shortcut and decoder in front of a classifier conv.  `use_v3plus_forward(head_cls)` binds
# halo_amd.core.models.classifier.v3plus_forward, which is written on the helpers of v3plus_hyper_forward: unmarked it runs the
# reference's statements, and use_device_resize, use_fused_decoder_front, use_folded_image_pooling, use_fused_decoder_dropout and
# use_fused_feature_reweighting accept the bound class.  Opt-in, not bound by install(); parameters, module names and state_dict()
# are untouched.

_V3PLUS_ATTRS = ("parallel_branches", "global_branch", "bottleneck", "shortcut", "decoder", "old_decoder")


def _is_v3plus_class(cls):
    """the reference's DepthwiseSeparableASPP (by name), or an nn.Module class whose instances carry the six attributes and no
    conv_seg (class attributes, or names its __init__ methods assign: nothing is constructed)"""
    if not isinstance(cls, type) or not issubclass(cls, torch.nn.Module):
        return False
    if any(k.__name__ == "DepthwiseSeparableASPP" for k in cls.__mro__):
        return True
    names = set()
    for klass in cls.__mro__:
        init = klass.__dict__.get("__init__")
        names.update(getattr(getattr(init, "__code__", None), "co_names", ()))
    return all(hasattr(cls, a) or a in names for a in _V3PLUS_ATTRS) and not (hasattr(cls, "conv_seg") or "conv_seg" in names)


def use_v3plus_forward(head_cls):
    """Bind v3plus_forward on a Euclidean DeepLab-v3+ head class (the reference's DepthwiseSeparableASPP, or any nn.Module class
    whose instances carry parallel_branches, global_branch, bottleneck, shortcut, decoder and old_decoder and no conv_seg).  Returns
    the class; the forward it replaced is kept as `_unfused_forward`.  Idempotent."""
    from .core.models.classifier import v3plus_forward
    if not _is_v3plus_class(head_cls):
        raise TypeError("use_v3plus_forward: %r is not a Euclidean DeepLab-v3+ head class (instances with %s and without conv_seg)"
                        % (head_cls, ", ".join(_V3PLUS_ATTRS)))
    if _inherited(head_cls, "forward") is v3plus_forward:
        return head_cls
    head_cls._unfused_forward = _inherited(head_cls, "forward")
    head_cls.forward = v3plus_forward
    return head_cls
