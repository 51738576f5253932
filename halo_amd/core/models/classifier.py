"""Hyperbolic heads -- the part of core/models/classifier.py that is on the hot path.

ASPP_Classifier_V2_Hyper.forward (classifier.py:364-379) and DepthwiseSeparableASPP_Hyper.forward
(classifier.py:552-558) both end with

    embed = mapper.expmap(feat, dim=1)                 # float64
    out   = conv_seg(embed.double()).float()           # HyperMLR
    [bilinear(align_corners=True) of out (v3+) or of out AND embed (v2)]
    return out, embed

`hyper_head_tail` is that tail on HIP kernels.  The convolutional bodies in front of it stay on
PyTorch-ROCm/MIOpen (out of scope).  Two ways to reach the tail from the reference's
`forward(x: dict{'out','low'}, size=None) -> (out, embed)` interface:

  * `ASPP_Classifier_V2_Hyper` below is a complete drop-in class (its body is a sum of dilated convs);
  * `v2_hyper_forward` / `v3plus_hyper_forward` are `forward` replacements for the reference's own head
    classes -- they run the instance's own conv modules, then the HIP tail.  `halo_amd.install()`
    binds them onto core.models.classifier's classes, so checkpoints, constructors and the
    `build_classifier` factory (core/models/build.py) stay the reference's.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..configs import cfg
from ..utils.hyperbolic import HyperMapper, HyperMLR, bilinear_align_corners, head_tail_fused


def hyper_head_tail(feat, mapper: HyperMapper, conv_seg: HyperMLR, size=None, resize_embed=False, resize=None):
    """feat (B,C,h,w) float32 from conv_reduce / the ASPP sum -> (out float32, embed float64).

    resize_embed=False: DeepLab-v3+ tail (classifier.py:552-558); True: DeepLab-v2 tail, which also
    resizes the embedding (classifier.py:375-377).  resize: None (default) resizes with F.interpolate under training; a
    callable (x, size) -> resized x replaces it there (halo_amd.resize.resize_or_interpolate for a head class marked with
    halo_amd.hooks.use_device_resize: the HIP resize with its atomic-free backward)."""
    training = torch.is_grad_enabled() and (feat.requires_grad or conv_seg.P_MLR.requires_grad)
    if training:
        # expmap and HyperMLR carry HIP backward kernels; by default the resize stays on F.interpolate, which autograd
        # already differentiates; `resize` (see above) puts it on halo_amd.resize instead
        embed = mapper.expmap(feat, dim=1)
        out = conv_seg._hyper_logits(embed, out_dtype=torch.float32)      # = conv_seg(embed).float(), the cast fused into the kernel's store
        if size is not None and resize is not None:
            out = resize(out, size)
            if resize_embed:
                embed = resize(embed, size)
        elif size is not None:
            out = F.interpolate(out, size=size, mode="bilinear", align_corners=True)
            if resize_embed:
                embed = F.interpolate(embed, size=size, mode="bilinear", align_corners=True)
        return out, embed
    with torch.no_grad():
        # the heads' own shape (64 channels): expmap -> HyperMLR -> .float() in ONE kernel, the embedding never re-read; any other
        # shape: the two calls (same bits either way)
        fused = head_tail_fused(feat, conv_seg.P_MLR, conv_seg.A_MLR, conv_seg.c) if (feat.is_cuda and feat.dim() == 4 and float(mapper.c) == float(conv_seg.c)) else None
        if fused is not None:
            out, embed = fused
        else:
            embed = mapper.expmap(feat, dim=1)
            out = conv_seg._hyper_logits(embed, out_dtype=torch.float32)
        if size is not None:
            out = bilinear_align_corners(out, size)
            if resize_embed:
                embed = bilinear_align_corners(embed, size)
    return out, embed


def _tail_modules(head):
    """(mapper, conv_seg) of a head instance as HIP-backed objects.  A reference-built head holds the
    reference's HyperMapper / HyperMLR (geoopt-backed): same curvature and the SAME parameter tensors are
    re-used, so optimiser state and checkpoints are unaffected."""
    tail = head.__dict__.get("_halo_tail")
    if tail is None or tail[1].P_MLR is not head.conv_seg.P_MLR or tail[1].A_MLR is not head.conv_seg.A_MLR:
        mapper = head.mapper if isinstance(head.mapper, HyperMapper) else HyperMapper(c=head.mapper.c)
        seg = head.conv_seg
        if not isinstance(seg, HyperMLR):
            mlr = HyperMLR.__new__(HyperMLR)
            nn.Module.__init__(mlr)
            mlr.c, mlr.K, mlr.num_classes = seg.c, seg.K, seg.num_classes
            mlr.P_MLR, mlr.A_MLR = seg.P_MLR, seg.A_MLR          # shared Parameters, not copies
            seg = mlr
        tail = (mapper, seg)
        head.__dict__["_halo_tail"] = tail                        # not a registered submodule: state_dict unchanged
    return tail


def device_resize(head_or_learner):
    """halo_amd.resize.resize_or_interpolate when the instance's class is marked by halo_amd.hooks.use_device_resize, else None"""
    if not getattr(type(head_or_learner), "_halo_device_resize", False):
        return None
    from ...resize import resize_or_interpolate
    return resize_or_interpolate


def broadcast_or_resize(pooled, size, resize):
    """The global-pooling branch under the switch: align_corners=True of a single cell returns that cell exactly, so a 1 x 1
    map is broadcast (expand's backward is torch's ordinary, deterministic sum); any other map goes through `resize`."""
    if tuple(pooled.shape[2:]) == (1, 1):
        return pooled.expand(-1, -1, int(size[0]), int(size[1]))
    return resize(pooled, size)


def folded_pooling(self, pooled):
    """whether this head hands the pooled map to the bottleneck stage as it is: its class is marked by
    halo_amd.hooks.use_folded_image_pooling and the map is 1 x 1 (the broadcast that a marked head leaves out is exact only then)"""
    return getattr(type(self), "_halo_folded_image_pooling", False) and pooled.dim() == 4 and tuple(pooled.shape[2:]) == (1, 1)


def pyramid_with_pooled(self, pyramid, pooled, size, resize):
    """today's statements for the pooled branch: resized (or, under use_device_resize, broadcast) to the map and appended"""
    if resize is None:
        return pyramid + [F.interpolate(pooled, size=size, mode="bilinear", align_corners=True)]
    return pyramid + [broadcast_or_resize(pooled, size, resize)]


def aspp_pyramid(self, top):
    """[branch(top) for branch in self.parallel_branches], the statement every v3+ forward of the package starts with.

    On a head class marked by halo_amd.hooks.use_fused_aspp_depthwise, every maximal run of 2..4 consecutive branches that are
    separable blocks under use_fused_depthwise (the block's class carries fused_dwsep_forward) with an nn.ReLU depthwise_activate,
    and whose depthwise halves halo_amd.dwconv.multi_fallback_reason serves together, gets those halves from one
    halo_amd.dwconv.multi_depthwise_bn_relu call -- top is read once for the run, and the run's share of top's gradient is
    written once -- and each output goes through halo_amd.hooks.pointwise_tail(block, y_i).  Longer runs are cut into groups of
    at most four.  Branch order is unchanged; every other branch is called as before."""
    if not getattr(type(self), "_halo_fused_aspp_depthwise", False):
        return [branch(top) for branch in self.parallel_branches]
    return [y for segment in _pyramid_segments(self, top) for y in _run_segment(segment, top)]


def _pyramid_segments(self, top):
    """parallel_branches of a head marked by use_fused_aspp_depthwise, cut in branch order into aspp_pyramid's segments: (run, blocks)
    for a run that multi_depthwise_bn_relu serves over `top`, ([branch], None) for every other branch.  Calls no branch."""
    branches = list(self.parallel_branches)
    from ...dwconv import MULTI_MAX, multi_fallback_reason
    from ...hooks import _DWSEP_ATTRS, _inherited, fused_dwsep_forward

    def eligible(m):
        return (all(hasattr(m, a) for a in _DWSEP_ATTRS) and _inherited(type(m), "forward") is fused_dwsep_forward
                and type(m.depthwise_activate) is nn.ReLU)

    segments, i = [], 0
    while i < len(branches):
        run = []
        while i + len(run) < len(branches) and len(run) < MULTI_MAX and eligible(branches[i + len(run)]):
            run.append(branches[i + len(run)])
        blocks = [(m.depthwise_conv, m.depthwise_bn, m.depthwise_activate) for m in run]
        if len(run) >= 2 and multi_fallback_reason(top, blocks) is None:
            segments.append((run, blocks))
            i += len(run)
        else:
            segments.append(([branches[i]], None))
            i += 1
    return segments


def _run_segment(segment, top):
    """the outputs of one of _pyramid_segments' segments over `top`"""
    from ...dwconv import multi_depthwise_bn_relu
    from ...hooks import pointwise_tail
    run, blocks = segment
    if blocks is None:
        return [run[0](top)]
    return [pointwise_tail(m, y) for m, y in zip(run, multi_depthwise_bn_relu(top, blocks))]


def _plane_mean_branch(branch):
    """whether `branch` is an nn.Sequential, called as one, that starts with an nn.AdaptiveAvgPool2d of output size 1 and carries no
    forward hooks: halo_amd.fanout.plane_mean can stand in for that child"""
    if not isinstance(branch, nn.Sequential) or type(branch).forward is not nn.Sequential.forward or "forward" in branch.__dict__ or len(branch) == 0:
        return False
    pool = branch[0]
    if type(pool) is not nn.AdaptiveAvgPool2d or "forward" in pool.__dict__ or pool.output_size not in (1, (1, 1), [1, 1]):
        return False
    return not any(m._forward_hooks or m._forward_pre_hooks for m in (branch, pool))


def pooled_aspp_pyramid(self, top):
    """(aspp_pyramid(self, top), self.global_branch(top)): the two statements every v3+ forward of the package starts with, and
    exactly those on a head class that halo_amd.hooks.use_joined_aspp_gradients has not marked.

    A head marked by it and by use_fused_aspp_depthwise, whose first served run of dilated blocks
    halo_amd.fanout.fan_fallback_reason accepts with one further reader per other segment of the pyramid (a branch, or a later
    served run) and one for global_branch, runs that run through halo_amd.fanout.fan_depthwise_bn_relu: every other segment reads
    one of the aliases of top it returns, in branch order, global_branch the last, and top's gradient is written once, by that
    node's pass.  A global_branch of the form Sequential(AdaptiveAvgPool2d(1), ...) without forward hooks has
    halo_amd.fanout.plane_mean stand in for the pool -- its gradient then reaches the pass as one value per plane -- and its
    remaining children called in order; any other global_branch is called whole on its alias.  Outputs and parameter gradients are
    those of the head under use_fused_aspp_depthwise alone, bit for bit."""
    cls = type(self)
    if getattr(cls, "_halo_joined_aspp_gradients", False) and getattr(cls, "_halo_fused_aspp_depthwise", False):
        from ...fanout import fan_depthwise_bn_relu, fan_fallback_reason, plane_mean
        from ...hooks import pointwise_tail
        segments = _pyramid_segments(self, top)
        served = next((k for k, s in enumerate(segments) if s[1] is not None), None)
        if served is not None and fan_fallback_reason(top, segments[served][1], len(segments)) is None:
            ys, xs = fan_depthwise_bn_relu(top, segments[served][1], len(segments))
            xs, pyramid = list(xs), []
            for k, segment in enumerate(segments):
                if k == served:
                    pyramid += [pointwise_tail(m, y) for m, y in zip(segment[0], ys)]
                else:
                    pyramid += _run_segment(segment, xs.pop(0))
            pooled = xs.pop(0)
            if _plane_mean_branch(self.global_branch):
                pooled = plane_mean(pooled)
                for child in list(self.global_branch)[1:]:
                    pooled = child(pooled)
            else:
                pooled = self.global_branch(pooled)
            return pyramid, pooled
    pyramid = aspp_pyramid(self, top)
    pooled = self.global_branch(top)
    return pyramid, pooled


def v3plus_bottleneck(self, pyramid, pooled, resize):
    """The bottleneck of a head marked by halo_amd.hooks.use_folded_image_pooling: pyramid holds the parallel branches alone, pooled
    is global_branch's (B, Cg, 1, 1) output.  A `bottleneck` of the form Sequential(Conv2d, FrozenBatchNorm2d, nn.ReLU) inside the
    operator's envelope (halo_amd.aspp.pool_fold_fallback_reason) runs halo_amd.aspp.pooled_bottleneck's operator, which reads
    bottleneck[1]'s buffers itself (so fuse_norm_relu_pairs on the same head changes nothing here); anything else runs the
    statements of an unmarked head -- over the branches' concatenation when the envelope, which looks at it, has already made it."""
    from ... import aspp
    bt = self.bottleneck
    if isinstance(bt, nn.Sequential) and len(bt) == 3 and type(bt[2]) is nn.ReLU:
        p = torch.cat(pyramid, dim=1)
        if aspp.pool_fold_fallback_reason(p, pooled, bt[0], bt[1], bt[2]) is None:
            return aspp.fused_pooled_bottleneck(p, pooled, bt[0], bt[1])
        pyramid = [p]                            # outside the envelope: the concatenation made above is kept, the pooled map joins it
    return self.bottleneck(torch.cat(pyramid_with_pooled(self, pyramid, pooled, pyramid[0].shape[2:], resize), dim=1))


def v3plus_decoder(self, pyramid, low, resize, pooled=None, run=None):
    """The v3+ heads from the ASPP pyramid to the decoder's output (classifier.py:520-527): bottleneck, resize to the low-level
    map, concat with the shortcut, decoder.  Every v3+ forward of the package calls it.

    A head class marked by halo_amd.hooks.use_fused_decoder_front runs the front of the decoder -- the resize, the concat and the
    depthwise half of decoder[0] -- as halo_amd.dwconv.upsample_cat_depthwise_bn_relu, which stores neither the resized nor the
    concatenated tensor, then decoder[0]'s three pointwise modules and the remaining decoder modules unchanged.  That holds when
    decoder[0] is a depthwise-separable block (the six DepthwiseSeparableConv2d attributes, an nn.ReLU depthwise_activate) inside
    the operator's envelope (upcat_fallback_reason); any other marked instance, and every unmarked class, runs the statements
    below.  A marked head returns what the same head returns under use_device_resize + use_fused_depthwise on that block, bit for
    bit; that is not bit-equal to the stock F.interpolate / nn.Conv2d chain.  A head class that
    halo_amd.hooks.use_joint_depthwise_backward marks as well passes joint_backward=True there: the same bits.

    All three tails hand the decoder's input to halo_amd.hooks.run_decoder: an unmarked head calls self.decoder (behind the fused
    front: decoder[0]'s pointwise half, then the remaining modules) as before; a block class marked by use_fused_pointwise_norm runs
    its pointwise norm + ReLU as one pass, and a head class marked by use_fused_decoder_dropout runs such a block and the
    nn.Dropout2d behind it through halo_amd.norm.norm_relu_dropout2d.  Both return the stock statements' bits.

    pooled: None, or -- from a head marked by halo_amd.hooks.use_folded_image_pooling -- global_branch's 1 x 1 output, which pyramid
    then does not hold: the bottleneck runs as v3plus_bottleneck.

    run: None, or the walk that takes run_decoder's place and arguments (v3plus_forward's old decoder layout hands in
    halo_amd.hooks.run_decoder_pair, whose two results come back as they are)."""
    if run is None:
        from ...hooks import run_decoder as run

    def bottleneck():                            # the one place that says how the bottleneck's output is made
        if pooled is None:
            return self.bottleneck(torch.cat(pyramid, dim=1))
        return v3plus_bottleneck(self, pyramid, pooled, resize)

    if getattr(type(self), "_halo_fused_decoder_front", False):
        from ...dwconv import upcat_fallback_reason, upsample_cat_depthwise_bn_relu
        from ...hooks import _DWSEP_ATTRS
        block = self.decoder[0] if isinstance(self.decoder, nn.Sequential) and len(self.decoder) > 0 else None
        if block is not None and all(hasattr(block, a) for a in _DWSEP_ATTRS) and type(block.depthwise_activate) is nn.ReLU:
            top = bottleneck()
            short = self.shortcut(low)
            if upcat_fallback_reason(top, short, block.depthwise_conv, block.depthwise_bn) is None:
                dec = upsample_cat_depthwise_bn_relu(top, short, block.depthwise_conv, block.depthwise_bn,
                                                     joint_backward=getattr(type(self), "_halo_joint_depthwise_backward", False))
                return run(self, dec, first_half_done=True)
            if resize is None:
                fused = F.interpolate(top, size=low.shape[2:], mode="bilinear", align_corners=True)
            else:
                fused = resize(top, low.shape[2:])
            return run(self, torch.cat([fused, short], dim=1))
    if resize is None:
        fused = bottleneck()
        fused = F.interpolate(fused, size=low.shape[2:], mode="bilinear", align_corners=True)
    else:
        fused = resize(bottleneck(), low.shape[2:])
    return run(self, torch.cat([fused, self.shortcut(low)], dim=1))


def v2_hyper_forward(self, x, size=None):
    """forward of ASPP_Classifier_V2_Hyper (classifier.py:364-379): sum of the dilated 3x3 branches, HIP tail;
    DeepLab-v2 resizes the logits AND the embedding."""
    feat = x["out"]
    branches = iter(self.conv2d_list)
    embed = next(branches)(feat)
    for conv in branches:
        embed = embed + conv(feat)
    mapper, seg = _tail_modules(self)
    return hyper_head_tail(embed, mapper, seg, size=size, resize_embed=True, resize=device_resize(self))


def v3plus_hyper_forward(self, x, size=None):
    """forward of DepthwiseSeparableASPP_Hyper (classifier.py:486-558): the instance's own ASPP / decoder
    modules (PyTorch), optional weighted normalisation (`wn_mlp`, HFR), then the HIP tail."""
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
    if getattr(self, "wn_mlp", None) is not None:                      # classifier.py:531-550
        b, ch, h, w = dec.shape
        weights = self.wn_mlp(dec.permute(0, 2, 3, 1).reshape(-1, ch)).view(b, h * w, ch).mean(dim=1)
        weights = weights.clamp(min=1e-5).view(b, ch, 1, 1)
        dec = F.normalize(dec.reshape(b, ch, h * w), dim=-1).reshape(b, ch, h, w) * weights
    mapper, seg = _tail_modules(self)
    return hyper_head_tail(dec, mapper, seg, size=size, resize_embed=False, resize=resize)


def v3plus_forward(self, x, size=None):
    """forward of DepthwiseSeparableASPP (classifier.py:248-316), the Euclidean DeepLab-v3+ head: the instance's own modules on the
    helpers v3plus_hyper_forward uses, so the class marks of halo_amd.hooks act on it as they do there.  Returns (out, decoder_out);
    `size` resizes out alone.

    New layout (`old_decoder` false): decoder, conv_reduce and the wn_mlp statement where the instance has them -- halo_amd.hfr's
    weighted_normalize on a class marked by use_fused_feature_reweighting, its torch_statement otherwise -- then cls_conv.
    Old layout: decoder = Sequential(block, block, Dropout2d, Conv2d); decoder_out is decoder[1]'s output, the remaining modules
    run on it (halo_amd.hooks.run_decoder_pair)."""
    from ...hooks import run_decoder_pair
    low, top = x["low"], x["out"]
    pyramid, pooled = pooled_aspp_pyramid(self, top)
    # the mark is about the device backward's atomics: on CPU tensors, which no operator serves, every resize is the stock statement --
    # the 1 x 1 pooled map's too, whose broadcast has F.interpolate's values but sums its gradient in another order
    resize = device_resize(self) if top.is_cuda else None
    run = run_decoder_pair if self.old_decoder else None
    if folded_pooling(self, pooled):
        dec = v3plus_decoder(self, pyramid, low, resize, pooled=pooled, run=run)
    else:
        if resize is None:
            pyramid.append(F.interpolate(pooled, size=top.shape[2:], mode="bilinear", align_corners=True))
        else:
            pyramid.append(broadcast_or_resize(pooled, top.shape[2:], resize))
        dec = v3plus_decoder(self, pyramid, low, resize, run=run)
    if self.old_decoder:
        dec, out = dec
    else:
        if self.conv_reduce is not None:
            dec = self.conv_reduce(dec)
        if self.wn_mlp is not None:                                        # classifier.py:283-304
            from ... import hfr
            fused = getattr(type(self), "_halo_fused_feature_reweighting", False)
            dec = hfr.weighted_normalize(dec, self.wn_mlp) if fused else hfr.torch_statement(dec, self.wn_mlp)
        out = self.cls_conv(dec)
    if size is not None and resize is not None:
        out = resize(out, size)
    elif size is not None:
        out = F.interpolate(out, size=size, mode="bilinear", align_corners=True)
    return out, dec


class ASPP_Classifier_V2_Hyper(nn.Module):
    """Drop-in for core/models/classifier.py:335-379 (DeepLab-v2 hyperbolic head): same constructor, same
    parameter names (`conv2d_list.N.weight/bias`, `conv_seg.P_MLR/A_MLR`), same forward interface."""

    def __init__(self, in_channels, dilation_series, padding_series, num_classes, reduced_channels):
        super().__init__()
        self.conv2d_list = nn.ModuleList(
            nn.Conv2d(in_channels, reduced_channels, kernel_size=3, stride=1, padding=p, dilation=d, bias=True)
            for d, p in zip(dilation_series, padding_series))
        for m in self.conv2d_list:
            m.weight.data.normal_(0, 0.01)
        self.mapper = HyperMapper(c=cfg.MODEL.CURVATURE)
        self.conv_seg = HyperMLR(reduced_channels, num_classes, c=cfg.MODEL.CURVATURE)

    forward = v2_hyper_forward


def patch_reference_heads(module):
    """Bind the HIP-tail forwards onto the reference's head classes found in `module`
    (core.models.classifier).  Returns the names patched."""
    done = []
    for name, fwd in (("ASPP_Classifier_V2_Hyper", v2_hyper_forward), ("DepthwiseSeparableASPP_Hyper", v3plus_hyper_forward)):
        cls = getattr(module, name, None)
        if isinstance(cls, type) and cls.__dict__.get("forward") is not fwd:
            cls._reference_forward = cls.__dict__.get("forward")
            cls.forward = fwd
            done.append(name)
    return done
