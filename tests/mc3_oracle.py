"""torchvision's ``mc3_18`` from plain ``torch.nn`` containers: the oracle of
the ``tv_block="mc3"`` tests. It imports nothing from ``rnb_amd``; the layout is
written down once more here from torchvision's published description
(``BasicStem``, ``BasicBlock`` over ``Conv3DSimple`` in layer1 and over
``Conv3DNoTemporal`` in layer2..4, ``VideoResNet``). Depth 18 has 11 695 440
parameters; no layer strides in time."""
import torch
import torch.nn as nn

from tv_oracle import randomise_

PARAMS = 11695440
PLANES = (64, 128, 256, 512)


def cbn(i, o, k, s, p, eps, relu):
    mods = [nn.Conv3d(i, o, k, stride=s, padding=p, bias=False), nn.BatchNorm3d(o, eps=eps)]
    return nn.Sequential(*(mods + [nn.ReLU(inplace=False)] if relu else mods))


class Block(nn.Module):
    def __init__(self, i, o, s, eps, flat):
        super().__init__()
        k, p, s3 = ((1, 3, 3), (0, 1, 1), (1, s, s)) if flat else (3, 1, s)
        self.conv1 = cbn(i, o, k, s3, p, eps, True)
        self.conv2 = cbn(o, o, k, 1, p, eps, False)
        self.downsample = cbn(i, o, 1, s3, 0, eps, False) if (s != 1 or i != o) else None

    def forward(self, x):
        r = x if self.downsample is None else self.downsample(x)
        return torch.relu(self.conv2(self.conv1(x)) + r)


class MC3Oracle(nn.Module):
    def __init__(self, num_classes=400, bn_eps=1e-5):
        super().__init__()
        self.stem = cbn(3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3), bn_eps, True)
        inp = 64
        for li, planes in enumerate(PLANES, 1):
            s = 2 if li > 1 else 1
            setattr(self, "layer%d" % li, nn.Sequential(Block(inp, planes, s, bn_eps, li > 1),
                                                        Block(planes, planes, 1, bn_eps, li > 1)))
            inp = planes
        self.avgpool = nn.AdaptiveAvgPool3d(1)
        self.fc = nn.Linear(512, num_classes)

    def forward(self, x):
        x = self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
        return self.fc(self.avgpool(x).flatten(1))


def make(num_classes=400, bn_eps=1e-5, seed=0):
    return randomise_(MC3Oracle(num_classes, bn_eps), seed).eval()
