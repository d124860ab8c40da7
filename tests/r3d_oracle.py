"""torchvision's ``r3d_18`` from plain ``torch.nn`` containers: the oracle of
the ``tv_block="3d"`` tests. It imports nothing from ``rnb_amd``; the layout is
written down once more here from torchvision's published description
(``BasicStem``, ``BasicBlock`` over ``Conv3DSimple``, ``VideoResNet``).
Depth 18 has 33 371 472 parameters."""
import torch
import torch.nn as nn

from tv_oracle import randomise_

PARAMS, ENTRIES = 33371472, 122
PLANES = (64, 128, 256, 512)


def cbn(i, o, k, s, p, eps, relu):
    mods = [nn.Conv3d(i, o, k, stride=s, padding=p, bias=False), nn.BatchNorm3d(o, eps=eps)]
    return nn.Sequential(*(mods + [nn.ReLU(inplace=False)] if relu else mods))


class Block(nn.Module):
    def __init__(self, i, o, s, eps):
        super().__init__()
        self.conv1 = cbn(i, o, 3, s, 1, eps, True)
        self.conv2 = cbn(o, o, 3, 1, 1, eps, False)
        self.downsample = cbn(i, o, 1, s, 0, eps, False) if (s != 1 or i != o) else None

    def forward(self, x):
        r = x if self.downsample is None else self.downsample(x)
        return torch.relu(self.conv2(self.conv1(x)) + r)


class R3DOracle(nn.Module):
    def __init__(self, num_classes=400, bn_eps=1e-5):
        super().__init__()
        self.stem = cbn(3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3), bn_eps, True)
        inp = 64
        for li, planes in enumerate(PLANES, 1):
            s = 2 if li > 1 else 1
            setattr(self, "layer%d" % li, nn.Sequential(Block(inp, planes, s, bn_eps),
                                                        Block(planes, planes, 1, bn_eps)))
            inp = planes
        self.avgpool = nn.AdaptiveAvgPool3d(1)
        self.fc = nn.Linear(512, num_classes)

    def forward(self, x):
        x = self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
        return self.fc(self.avgpool(x).flatten(1))


def make(num_classes=400, bn_eps=1e-5, seed=0):
    return randomise_(R3DOracle(num_classes, bn_eps), seed).eval()
