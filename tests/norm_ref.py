"""Stand-ins shared by tests/test_norm_relu_host.py and tests/test_gpu_norm_relu.py: the two residual block forms of
core/models/resnet.py, a ResNet-shaped backbone whose stem sits in an IntermediateLayerGetter, and a v3+-shaped head, all with the
stand-in FrozenBatchNorm2d of tests/dwconv_ref.py; the stock chain spelled out; and the comparisons of the two test files."""
import copy
from collections import OrderedDict

import torch
import torch.nn as nn

from dwconv_ref import FrozenBatchNorm2d


def stock_chain(x, bn, residual=None, residual_bn=None):
    """the statements of resnet.py:103-110 (or `bn, relu` alone), written out: the oracle of every comparison"""
    out = bn(x)
    if residual is not None:
        identity = residual if residual_bn is None else residual_bn(residual)
        out += identity
    return torch.relu_(out)


def randomize_norms(module, seed):
    """statistics with both signs of scale and of shift in every frozen norm under `module`"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if type(m).__name__ != "FrozenBatchNorm2d":
                continue
            n = m.weight.numel()
            sign = torch.where(torch.arange(n) % 2 == 0, -1.0, 1.0)
            dev = m.weight.device
            m.weight.copy_(((0.25 + 1.5 * torch.rand(n, generator=gen)) * sign).to(dev))
            m.bias.copy_((0.4 * torch.randn(n, generator=gen)).to(dev))
            m.running_mean.copy_((0.5 * torch.randn(n, generator=gen)).to(dev))
            m.running_var.copy_((0.3 + 1.5 * torch.rand(n, generator=gen)).to(dev))
    return module


def same_bits(a, b):
    """NaN positions equal, everything else torch.equal"""
    na, nb = a.isnan(), b.isnan()
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a),
                                                                      torch.where(nb, torch.zeros_like(b), b))


class Bottleneck(nn.Module):
    """the attribute names and statements of the reference's Bottleneck"""

    def __init__(self, cin, width, cout, stride=1, dilation=1, downsample=None, norm=FrozenBatchNorm2d, act=None):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = norm(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, dilation, dilation, bias=False)
        self.bn2 = norm(width)
        self.conv3 = nn.Conv2d(width, cout, 1, bias=False)
        self.bn3 = norm(cout)
        self.relu = nn.ReLU(inplace=True) if act is None else act
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class BasicBlock(nn.Module):
    """the attribute names and statements of the reference's BasicBlock"""

    def __init__(self, cin, cout, stride=1, downsample=None, norm=FrozenBatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = norm(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = norm(cout)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def down(cin, cout, stride=1, norm=FrozenBatchNorm2d):
    return nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), norm(cout))


class IntermediateLayerGetter(nn.ModuleDict):
    """torchvision's container of that name: the children run in order, the named outputs are returned"""

    def __init__(self, layers, return_layers):
        super().__init__(layers)
        self.return_layers = dict(return_layers)

    def forward(self, x):
        out = OrderedDict()
        for name, module in self.items():
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


def backbone():
    """stem + 2 bottlenecks with a Sequential(conv, norm) downsample + 1 dilated bottleneck without one, channels 8 / 32"""
    layers = OrderedDict()
    layers["conv1"] = nn.Conv2d(3, 8, 3, 2, 1, bias=False)
    layers["bn1"] = FrozenBatchNorm2d(8)
    layers["relu"] = nn.ReLU(inplace=True)
    layers["maxpool"] = nn.MaxPool2d(3, 2, 1)
    layers["layer1"] = nn.Sequential(Bottleneck(8, 8, 32, downsample=down(8, 32)), Bottleneck(32, 8, 32, stride=2, downsample=down(32, 32, 2)))
    layers["layer2"] = nn.Sequential(Bottleneck(32, 8, 32, dilation=2))
    return IntermediateLayerGetter(layers, {"layer1": "low", "layer2": "out"})


class Head(nn.Module):
    """the sequentials of a v3+ head that hold (norm, ReLU) neighbours: parallel_branches[0], global_branch, bottleneck, shortcut"""

    def __init__(self, cin=32, clow=32, mid=8):
        super().__init__()
        self.parallel_branches = nn.ModuleList([nn.Sequential(nn.Conv2d(cin, mid, 1, bias=False), FrozenBatchNorm2d(mid), nn.ReLU(inplace=True))])
        self.global_branch = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(cin, mid, 1, bias=False), FrozenBatchNorm2d(mid),
                                           nn.ReLU(inplace=True))
        self.bottleneck = nn.Sequential(nn.Conv2d(2 * mid, mid, 3, 1, 1, bias=False), FrozenBatchNorm2d(mid), nn.ReLU(inplace=True),
                                        nn.Dropout(0.0))
        self.shortcut = nn.Sequential(nn.Conv2d(clow, 6, 1, bias=False), FrozenBatchNorm2d(6), nn.ReLU(inplace=True))

    def forward(self, x):
        top, low = x["out"], x["low"]
        pooled = self.global_branch(top).expand(-1, -1, *top.shape[2:])
        fused = self.bottleneck(torch.cat([self.parallel_branches[0](top), pooled], dim=1))
        return fused, self.shortcut(low)


def hooked_copy(model):
    """a deep copy whose residual blocks run halo_amd.hooks.fused_residual_forward (bound on subclasses, the stand-in classes stay
    as they are) and whose (norm, ReLU) neighbours are fused; returns (copy, pairs fused)"""
    from halo_amd.hooks import fuse_norm_relu_pairs, use_fused_frozen_norm
    twin = copy.deepcopy(model)
    subs = {}
    for m in twin.modules():
        if type(m) in (Bottleneck, BasicBlock):
            if type(m) not in subs:
                subs[type(m)] = use_fused_frozen_norm(type(type(m).__name__, (type(m),), {}))
            m.__class__ = subs[type(m)]
    return twin, fuse_norm_relu_pairs(twin)


def conv_weights(model):
    return [m.weight for m in model.modules() if isinstance(m, nn.Conv2d)]


def run_with_grads(model, x, g_of):
    """(outputs as a list, [input gradient] + conv weight gradients) of one forward and backward; g_of(outputs) gives the incoming
    gradients"""
    xin = x.detach().clone().requires_grad_(True)
    out = model(xin)
    outs = list(out.values()) if isinstance(out, dict) else list(out) if isinstance(out, (tuple, list)) else [out]
    grads = torch.autograd.grad(outs, [xin] + conv_weights(model), g_of(outs))
    return [o.detach() for o in outs], list(grads)


class Net(nn.Module):
    """backbone + head"""

    def __init__(self):
        super().__init__()
        self.feature_extractor = backbone()
        self.classifier = Head()

    def forward(self, x):
        return self.classifier(self.feature_extractor(x))
