"""A stand-in for the reference's Euclidean DeepLab-v3+ head (DepthwiseSeparableASPP, core/models/classifier.py:88-316) with its
attribute layout, its two decoder layouts and its forward statements at small widths: inplanes 24, branch width 16, dilations
1 / 2 / 3, shortcut 12 -> 8, decoder 24 -> 16 -> 16, K = 5, reduced 8 in the new layout.  tests/test_euclid_head_host.py and
tests/test_gpu_euclid_head.py build their heads from it."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from dwconv_ref import FrozenBatchNorm2d


def frozen(n, seed):
    gen = torch.Generator().manual_seed(seed)
    bn = FrozenBatchNorm2d(n)
    bn.weight.copy_(0.25 + 1.5 * torch.rand(n, generator=gen)), bn.bias.copy_(0.4 * torch.randn(n, generator=gen))
    bn.running_mean.copy_(0.5 * torch.randn(n, generator=gen)), bn.running_var.copy_(0.3 + 1.5 * torch.rand(n, generator=gen))
    bn.weight[1] = -0.75
    return bn


class Block(nn.Module):
    """DepthwiseSeparableConv2d's attribute names and statements"""

    def __init__(self, cin, cout, d):
        super().__init__()
        self.depthwise_conv = nn.Conv2d(cin, cin, 3, 1, d, d, groups=cin, bias=False)
        self.depthwise_bn = frozen(cin, cin + d)
        self.depthwise_activate = nn.ReLU(inplace=True)
        self.pointwise_conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.pointwise_bn = frozen(cout, cout + d + 1)
        self.pointwise_activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.depthwise_activate(self.depthwise_bn(self.depthwise_conv(x)))
        return self.pointwise_activate(self.pointwise_bn(self.pointwise_conv(x)))


class EuclidHead(nn.Module):
    """old=True: decoder = Sequential(block, block, Dropout2d, Conv2d) (reduced 512 without HFR in the reference); old=False:
    decoder = Sequential(block, block), conv_reduce, wn_mlp (hfr) and cls_conv = Sequential(Dropout, Conv2d)"""

    def __init__(self, block=Block, old=True, hfr=False, p=0.1, top=24, mid=16, low=12, short=8, K=5, reduced=8):
        super().__init__()
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(top, mid, 1, bias=False), frozen(mid, 1), nn.ReLU(inplace=True))] + [
            block(top, mid, d) for d in (2, 3)])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Conv2d(top, mid, 1, bias=False), frozen(mid, 2), nn.ReLU(inplace=True))
        self.bottleneck = nn.Sequential(nn.Conv2d(4 * mid, mid, 3, padding=1, bias=False), frozen(mid, 3), nn.ReLU(inplace=True))
        self.shortcut = nn.Sequential(nn.Conv2d(low, short, 1, bias=False), frozen(short, 4), nn.ReLU(inplace=True))
        self.old_decoder = old
        if old:
            self.decoder = nn.Sequential(block(mid + short, mid, 1), block(mid, mid, 1), nn.Dropout2d(p), nn.Conv2d(mid, K, 1))
        else:
            self.decoder = nn.Sequential(block(mid + short, mid, 1), block(mid, mid, 1))
            self.conv_reduce = nn.Conv2d(mid, reduced, 1)
            self.wn_mlp = None
            if hfr:
                self.wn_mlp = nn.Sequential(nn.Linear(reduced, reduced), nn.BatchNorm1d(reduced), nn.ReLU(), nn.Linear(reduced, reduced))
            self.cls_conv = nn.Sequential(nn.Dropout(p), nn.Conv2d(reduced, K, 1))
        for m in self.modules():                                     # pre-activations a few times the norms' shifts: every ReLU of the
            if isinstance(m, nn.Conv2d):                             # head has active and inactive elements in most planes
                m.weight.data = torch.randn(m.weight.shape) * (2.0 / m.weight[0].numel() ** 0.5)

    def forward(self, x, size=None):
        """the reference's statements (classifier.py:248-316)"""
        low, x = x["low"], x["out"]
        aspp = [branch(x) for branch in self.parallel_branches]
        aspp.append(F.interpolate(self.global_branch(x), size=x.size()[2:], mode="bilinear", align_corners=True))
        top = self.bottleneck(torch.cat(aspp, dim=1))
        top = F.interpolate(top, size=low.size()[2:], mode="bilinear", align_corners=True)
        feats = torch.cat([top, self.shortcut(low)], dim=1)
        if not self.old_decoder:
            decoder_out = self.decoder(feats)
            if self.conv_reduce is not None:
                decoder_out = self.conv_reduce(decoder_out)
            if self.wn_mlp is not None:
                b, c, h, w = decoder_out.shape
                weights = self.wn_mlp(decoder_out.permute(0, 2, 3, 1).contiguous().view(-1, c)).view(-1, h * w, c)
                weights = torch.clamp(torch.mean(weights, dim=1).view(-1, c, 1, 1), min=1e-5)
                decoder_out = F.normalize(decoder_out.reshape(-1, c, h * w), dim=-1).reshape(-1, c, h, w) * weights
            out = self.cls_conv(decoder_out)
        else:
            for i in range(len(self.decoder)):
                feats = self.decoder[i](feats)
                if i == 1:
                    decoder_out = feats
            out = feats
        if size is not None:
            out = F.interpolate(out, size=size, mode="bilinear", align_corners=True)
        return out, decoder_out
