"""torchvision's R(2+1)D ``VideoResNet`` layout from plain ``torch.nn``
containers: the oracle of the ``arch="torchvision"`` tests.

It imports nothing from ``rnb_amd``. The layout is written down once more
here, from torchvision's published description (``R2Plus1dStem``,
``BasicBlock`` over ``Conv2Plus1D``, ``VideoResNet``), so that the product's
tree is checked against an independent statement of the key names and shapes:
depth 18 must have torchvision's published 31 505 325 parameters.

``mid_rule="block"`` is torchvision's (one mid-channel count per block, from
the block's input and output planes); ``"conv"`` recomputes it per conv from
that conv's own planes (the IG65M port's rule as the issue recalls it).
"""
import torch
import torch.nn as nn

LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}
PLANES = (64, 128, 256, 512)
# published / counted: (parameters, state-dict entries)
COUNTS = {18: (31505325, 224), 34: (61831661, 416)}


def mid(i, o):
    return (i * o * 3 * 3 * 3) // (i * 3 * 3 + 3 * o)


def conv2plus1d(i, o, m, s, eps):
    return nn.Sequential(
        nn.Conv3d(i, m, (1, 3, 3), stride=(1, s, s), padding=(0, 1, 1), bias=False),
        nn.BatchNorm3d(m, eps=eps),
        nn.ReLU(inplace=False),
        nn.Conv3d(m, o, (3, 1, 1), stride=(s, 1, 1), padding=(1, 0, 0), bias=False))


class Block(nn.Module):
    def __init__(self, i, o, s, rule, eps):
        super().__init__()
        m1 = mid(i, o)
        m2 = m1 if rule == "block" else mid(o, o)
        self.conv1 = nn.Sequential(conv2plus1d(i, o, m1, s, eps), nn.BatchNorm3d(o, eps=eps),
                                   nn.ReLU(inplace=False))
        self.conv2 = nn.Sequential(conv2plus1d(o, o, m2, 1, eps), nn.BatchNorm3d(o, eps=eps))
        if s != 1 or i != o:
            self.downsample = nn.Sequential(
                nn.Conv3d(i, o, 1, stride=(s, s, s), bias=False), nn.BatchNorm3d(o, eps=eps))
        else:
            self.downsample = None

    def forward(self, x):
        r = x if self.downsample is None else self.downsample(x)
        return torch.relu(self.conv2(self.conv1(x)) + r)


class TVOracle(nn.Module):
    def __init__(self, depth=18, num_classes=400, mid_rule="block", bn_eps=1e-5):
        super().__init__()
        assert mid_rule in ("block", "conv")
        self.stem = nn.Sequential(
            nn.Conv3d(3, 45, (1, 7, 7), stride=(1, 2, 2), padding=(0, 3, 3), bias=False),
            nn.BatchNorm3d(45, eps=bn_eps), nn.ReLU(inplace=False),
            nn.Conv3d(45, 64, (3, 1, 1), stride=1, padding=(1, 0, 0), bias=False),
            nn.BatchNorm3d(64, eps=bn_eps), nn.ReLU(inplace=False))
        inp = 64
        for li, (n, planes) in enumerate(zip(LAYERS[depth], PLANES)):
            blocks = []
            for j in range(n):
                blocks.append(Block(inp, planes, 2 if (j == 0 and li > 0) else 1, mid_rule,
                                    bn_eps))
                inp = planes
            setattr(self, "layer%d" % (li + 1), nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool3d(1)
        self.fc = nn.Linear(512, num_classes)

    def forward(self, x):
        x = self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
        return self.fc(self.avgpool(x).flatten(1))


def randomise_(model, seed=0):
    """Kaiming-normal convs, a small-normal classifier, and BN weights and
    running statistics drawn around identity (so BN folding is exercised)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Conv3d):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            elif isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.0 / 512) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.02)
            elif isinstance(m, nn.BatchNorm3d):
                c = m.num_features
                m.weight.copy_(1.0 + 0.1 * torch.randn(c, generator=g))
                m.bias.copy_(0.05 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.05 * torch.randn(c, generator=g))
                m.running_var.copy_(1.0 + 0.2 * torch.rand(c, generator=g))
    return model


def make(depth=18, num_classes=400, mid_rule="block", bn_eps=1e-5, seed=0):
    return randomise_(TVOracle(depth, num_classes, mid_rule, bn_eps), seed).eval()
