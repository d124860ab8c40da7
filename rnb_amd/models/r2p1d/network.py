"""R(2+1)D network in plain PyTorch: the numerics oracle.

The reference imports these building blocks from the ``R2Plus1D-PyTorch``
git submodule, which is empty in the mount; they are
reconstructed here from the reference's call sites (models/r2p1d/network.py:
3-60, model.py:14-16, 171-177) and the boundary shapes it asserts
(model.py:29-33). Parameter names follow the upstream module tree
(``res2plus1d.conv2.block1.conv1.spatial_conv.weight`` ...), so a state dict
saved by the reference loads unchanged (``load_reference_state_dict``).

Architecture:

* ``SpatioTemporalConv(in, out, k, stride, padding)`` = spatial 1×k×k conv
  -> BN -> ReLU -> temporal k×1×1 conv, intermediate width
  ``floor(kt·kh·kw·in·out / (kh·kw·in + kt·out))``; both convs carry a bias.
* ``SpatioTemporalResBlock`` = conv1 -> bn1 -> relu -> conv2 -> bn2
  (+ downsample STConv(k=1, stride 2) -> bn) -> add -> relu.
* stem ``conv1 = STConv(3, 64, [3,7,7], stride [1,2,2], pad [1,3,3])`` with no
  BN/ReLU after it, ``conv2..conv5`` residual layers, global average pool,
  ``Linear(512, num_classes)``.

``R2Plus1DLayerNet`` builds any contiguous range of layers 1..5 (the
layer-partitioned pipeline of model.py:20-84 / network.py:9-60).

``arch="torchvision"`` (``TVVideoResNet``) is the other R(2+1)D people hold
weights for: torchvision's ``VideoResNet`` with ``R2Plus1dStem``,
``BasicBlock`` and ``Conv2Plus1D`` (``r2plus1d_18``, the IG65M
``r2plus1d_34``). It is a different network -- a 45-channel stem followed by
BN + ReLU, bias-free convs, a plain 1x1x1 stride-(2, 2, 2) conv + BN shortcut,
one mid-channel count per block (or per conv: ``midplanes``) -- with the keys
``stem.*``, ``layerN.M.*`` and ``fc.*`` (``load_torchvision_state_dict``).
The layer ranges keep their meaning: index 1 is ``stem``, index k is
``layer(k-1)``, and ``fc`` comes with index 5.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

DEPTH_LAYER_SIZES = {10: (1, 1, 1, 1), 18: (2, 2, 2, 2), 26: (2, 3, 4, 3),
                     34: (3, 4, 6, 3)}

# (channels, T, H, W) entering each layer for 8x112x112 clips (model.py:29-33)
LAYER_INPUT_CTHW = {1: (3, 8, 112, 112), 2: (64, 8, 56, 56),
                    3: (64, 8, 56, 56), 4: (128, 4, 28, 28),
                    5: (256, 2, 14, 14)}
# (channels, T, H, W) leaving each layer (layer 5 leaves logits)
LAYER_OUTPUT_CTHW = {1: (64, 8, 56, 56), 2: (64, 8, 56, 56),
                     3: (128, 4, 28, 28), 4: (256, 2, 14, 14),
                     5: None}
LAYER_CHANNELS = {1: (3, 64), 2: (64, 64), 3: (64, 128), 4: (128, 256),
                  5: (256, 512)}

DEFAULT_CLIP_LENGTH = 8
# 8: the reference's clips; 16: the paper's / torchvision r2plus1d_18;
# 32: the Kinetics / IG-65M R(2+1)D-34 checkpoints
CLIP_LENGTHS = (8, 16, 32)


def check_clip_length(clip_length, key: str = "clip_length") -> int:
    """``clip_length`` as an int; ValueError (naming ``key``) unless 8, 16 or 32."""
    if isinstance(clip_length, bool) or clip_length not in CLIP_LENGTHS:
        raise ValueError("%s must be one of %s, got %r"
                         % (key, ", ".join(str(c) for c in CLIP_LENGTHS), clip_length))
    return int(clip_length)


def layer_geometry(clip_length: int = DEFAULT_CLIP_LENGTH):
    """(LAYER_INPUT_CTHW, LAYER_OUTPUT_CTHW) for ``clip_length`` x 112 x 112
    clips: T is unchanged through conv1 and conv2 and ``(T - 1) // 2 + 1``
    after each of conv3, conv4 and conv5 (their first block's stride-2
    temporal conv, k 3, pad 1); H x W as at 8 frames."""
    t = check_clip_length(clip_length)
    t3 = (t - 1) // 2 + 1
    t4 = (t3 - 1) // 2 + 1
    inp = {1: (3, t, 112, 112), 2: (64, t, 56, 56), 3: (64, t, 56, 56),
           4: (128, t3, 28, 28), 5: (256, t4, 14, 14)}
    out = {1: (64, t, 56, 56), 2: (64, t, 56, 56), 3: (128, t3, 28, 28),
           4: (256, t4, 14, 14), 5: None}
    return inp, out


def _triple(v):
    if isinstance(v, (list, tuple)):
        assert len(v) == 3
        return tuple(int(x) for x in v)
    return (int(v),) * 3


def intermediate_channels(in_ch: int, out_ch: int, kernel) -> int:
    kt, kh, kw = _triple(kernel)
    return int(math.floor((kt * kh * kw * in_ch * out_ch)
                          / (kh * kw * in_ch + kt * out_ch)))


class SpatioTemporalConv(nn.Module):
    """(2+1)D factorised convolution."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1,
                 padding=0, bias=True):
        super().__init__()
        kt, kh, kw = _triple(kernel_size)
        st, sh, sw = _triple(stride)
        pt, ph, pw = _triple(padding)
        mid = intermediate_channels(in_channels, out_channels, (kt, kh, kw))
        self.kernel_size = (kt, kh, kw)
        self.stride = (st, sh, sw)
        self.padding = (pt, ph, pw)
        self.intermed_channels = mid
        self.spatial_conv = nn.Conv3d(in_channels, mid, (1, kh, kw),
                                      stride=(1, sh, sw), padding=(0, ph, pw),
                                      bias=bias)
        self.bn = nn.BatchNorm3d(mid)
        self.relu = nn.ReLU()
        self.temporal_conv = nn.Conv3d(mid, out_channels, (kt, 1, 1),
                                       stride=(st, 1, 1), padding=(pt, 0, 0),
                                       bias=bias)

    def forward(self, x):
        return self.temporal_conv(self.relu(self.bn(self.spatial_conv(x))))


class SpatioTemporalResBlock(nn.Module):
    """Residual block of two STConvs with an optional strided shortcut."""

    def __init__(self, in_channels, out_channels, kernel_size, downsample=False):
        super().__init__()
        self.downsample = downsample
        padding = kernel_size // 2
        if downsample:
            self.downsampleconv = SpatioTemporalConv(in_channels, out_channels,
                                                     1, stride=2)
            self.downsamplebn = nn.BatchNorm3d(out_channels)
            self.conv1 = SpatioTemporalConv(in_channels, out_channels,
                                            kernel_size, padding=padding,
                                            stride=2)
        else:
            self.conv1 = SpatioTemporalConv(in_channels, out_channels,
                                            kernel_size, padding=padding)
        self.bn1 = nn.BatchNorm3d(out_channels)
        self.relu1 = nn.ReLU()
        self.conv2 = SpatioTemporalConv(out_channels, out_channels, kernel_size,
                                        padding=padding)
        self.bn2 = nn.BatchNorm3d(out_channels)
        self.outrelu = nn.ReLU()

    def forward(self, x):
        res = self.relu1(self.bn1(self.conv1(x)))
        res = self.bn2(self.conv2(res))
        if self.downsample:
            x = self.downsamplebn(self.downsampleconv(x))
        return self.outrelu(x + res)


class SpatioTemporalResLayer(nn.Module):
    """``layer_size`` residual blocks; the first may downsample."""

    def __init__(self, in_channels, out_channels, kernel_size, layer_size,
                 block_type=SpatioTemporalResBlock, downsample=False):
        super().__init__()
        self.block1 = block_type(in_channels, out_channels, kernel_size,
                                 downsample)
        self.blocks = nn.ModuleList(
            [block_type(out_channels, out_channels, kernel_size)
             for _ in range(layer_size - 1)])

    def forward(self, x):
        x = self.block1(x)
        for block in self.blocks:
            x = block(x)
        return x


def normalize_layer_sizes(start_idx: int, end_idx: int, layer_sizes=None,
                          depth: Optional[int] = None) -> Dict[int, int]:
    """Residual-layer sizes keyed by layer index 2..5.

    Accepts both conventions found in the reference: a 4-entry list for
    conv2..conv5 (``R2P1DSingleStep``, model.py:171) and a list positional over
    ``range(start_idx, end_idx + 1)`` (``R2P1DRunner``, network.py:20-34).
    ``depth`` (18 or 34) selects the standard sizes when no list is given.
    """
    if layer_sizes is None:
        if depth is None:
            depth = 18
        if depth not in DEPTH_LAYER_SIZES:
            raise ValueError("unsupported R(2+1)D depth %r" % depth)
        sizes = DEPTH_LAYER_SIZES[depth]
        return {i + 2: sizes[i] for i in range(4)}
    layer_sizes = [int(x) for x in layer_sizes]
    n = end_idx - start_idx + 1
    if len(layer_sizes) == n and not (n == 4 and start_idx == 2):
        return {idx: layer_sizes[i]
                for i, idx in enumerate(range(start_idx, end_idx + 1))
                if idx >= 2}
    if len(layer_sizes) == 4:
        return {i + 2: layer_sizes[i] for i in range(4)}
    if len(layer_sizes) == n:
        return {idx: layer_sizes[i]
                for i, idx in enumerate(range(start_idx, end_idx + 1))}
    raise ValueError("layer_sizes %r does not match layers %d..%d"
                     % (layer_sizes, start_idx, end_idx))


class R2Plus1DLayerNet(nn.Module):
    """Any contiguous range [start_idx, end_idx] of layers 1..5."""

    def __init__(self, start_idx, end_idx, layer_sizes: Dict[int, int],
                 block_type=SpatioTemporalResBlock):
        super().__init__()
        if not 1 <= start_idx <= end_idx <= 5:
            raise ValueError("layer range must satisfy 1 <= start <= end <= 5, "
                             "got %d..%d" % (start_idx, end_idx))
        self.start_idx, self.end_idx = start_idx, end_idx
        self.layer_list: List[nn.Module] = []
        for idx in range(start_idx, end_idx + 1):
            if idx == 1:
                self.conv1 = SpatioTemporalConv(3, 64, [3, 7, 7], stride=[1, 2, 2],
                                                padding=[1, 3, 3])
                self.layer_list.append(self.conv1)
            else:
                cin, cout = LAYER_CHANNELS[idx]
                layer = SpatioTemporalResLayer(cin, cout, 3, layer_sizes[idx],
                                               block_type=block_type,
                                               downsample=idx > 2)
                setattr(self, "conv%d" % idx, layer)
                self.layer_list.append(layer)
                if idx == 5:
                    self.pool = nn.AdaptiveAvgPool3d(1)
                    self.layer_list.append(self.pool)

    def forward(self, x):
        for layer in self.layer_list:
            x = layer(x)
        return x.view(-1, 512) if self.end_idx == 5 else x


class R2Plus1DLayerWrapper(nn.Module):
    """Layer range + the classifier when layer 5 is included."""

    def __init__(self, start_idx, end_idx, num_classes, layer_sizes,
                 block_type=SpatioTemporalResBlock):
        super().__init__()
        self.res2plus1d = R2Plus1DLayerNet(start_idx, end_idx, layer_sizes,
                                           block_type)
        self.start_idx, self.end_idx = start_idx, end_idx
        self.num_classes = num_classes
        if end_idx == 5:
            self.linear = nn.Linear(512, num_classes)

    def forward(self, x):
        x = self.res2plus1d(x)
        return self.linear(x) if self.end_idx == 5 else x


def R2Plus1DClassifier(num_classes=400, layer_sizes=(2, 2, 2, 2),
                       block_type=SpatioTemporalResBlock):
    """Full model; same module tree as upstream ``R2Plus1DClassifier``."""
    sizes = normalize_layer_sizes(1, 5, list(layer_sizes))
    return R2Plus1DLayerWrapper(1, 5, num_classes, sizes, block_type)


def init_random_(model: nn.Module, seed: int = 0) -> nn.Module:
    """Deterministic random init with non-trivial BN statistics.

    Every module draws from its own generator seeded by (seed, module name),
    so a layer-range runner holds exactly the weights of the same layers of
    the whole model: split pipelines compute the same function as one runner.
    Weights are Kaiming-normal (fan-in); BN gamma/beta/running stats are
    randomised around identity so eval-mode folding is actually exercised.
    """
    import zlib
    with torch.no_grad():
        for name, m in model.named_modules():
            g = torch.Generator().manual_seed(
                (zlib.crc32(name.encode()) * 1000003 + int(seed)) & 0x7FFFFFFFFFFF)
            if isinstance(m, (nn.Conv3d, nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g)
                               * math.sqrt(2.0 / fan_in))
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.02)
            elif isinstance(m, nn.BatchNorm3d):
                c = m.num_features
                m.weight.copy_(1.0 + 0.1 * torch.randn(c, generator=g))
                m.bias.copy_(0.05 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.05 * torch.randn(c, generator=g))
                m.running_var.copy_(1.0 + 0.2 * torch.rand(c, generator=g))
    return model


def load_reference_state_dict(model: R2Plus1DLayerWrapper, state_dict,
                              strict: bool = True):
    """Load a reference checkpoint's ``state_dict`` restricted to this range.

    Mirrors the key filter of model.py:50-63 (``res2plus1d.conv{i}.*`` for the
    built layers plus ``linear.*`` when layer 5 is built).
    """
    keep = {}
    for i in range(model.start_idx, model.end_idx + 1):
        prefix = "res2plus1d.conv%d" % i
        keep.update({k: v for k, v in state_dict.items()
                     if k.startswith(prefix + ".")})
    if model.end_idx == 5:
        keep.update({k: v for k, v in state_dict.items()
                     if k.startswith("linear.")})
    return model.load_state_dict(keep, strict=strict)


# ---------------------------------------------------------------------------
# torchvision layout (VideoResNet: R2Plus1dStem, BasicBlock, Conv2Plus1D)
# ---------------------------------------------------------------------------
ARCHS = ("reference", "torchvision")
MIDPLANES_RULES = ("block", "conv")
TV_STEM_MID = 45
DEFAULT_BN_EPS = 1e-5


def check_arch(arch, key: str = "arch") -> str:
    """``arch`` (None = "reference"); ValueError (naming ``key``) otherwise."""
    if arch is None:
        return "reference"
    if not isinstance(arch, str) or arch not in ARCHS:
        raise ValueError("%s must be one of %s, got %r"
                         % (key, ", ".join(repr(a) for a in ARCHS), arch))
    return arch


def check_midplanes(midplanes, key: str = "midplanes") -> Optional[str]:
    """``midplanes`` ("block", "conv" or None = from the checkpoint, else
    "block"); ValueError (naming ``key``) otherwise."""
    if midplanes is None:
        return None
    if not isinstance(midplanes, str) or midplanes not in MIDPLANES_RULES:
        raise ValueError("%s must be one of %s, got %r"
                         % (key, ", ".join(repr(a) for a in MIDPLANES_RULES), midplanes))
    return midplanes


def check_bn_eps(bn_eps, key: str = "bn_eps") -> Optional[float]:
    """``bn_eps`` as a positive float (None = the layout's 1e-5); ValueError
    (naming ``key``) otherwise."""
    if bn_eps is None:
        return None
    if isinstance(bn_eps, bool) or not isinstance(bn_eps, (int, float)) \
            or not (0.0 < float(bn_eps) < 1.0):
        raise ValueError("%s must be a float in (0, 1), got %r" % (key, bn_eps))
    return float(bn_eps)


def tv_midplanes(in_planes: int, planes: int) -> int:
    """torchvision's ``Conv2Plus1D`` mid-channel count."""
    return (in_planes * planes * 3 * 3 * 3) // (in_planes * 3 * 3 + 3 * planes)


def tv_block_mids(layer_sizes: Dict[int, int], rule: str = "block") -> Dict[str, int]:
    """``{"layerN.M.conv1": mid, "layerN.M.conv2": mid}`` for the residual
    layers of ``layer_sizes`` (keyed 2..5). ``rule="block"`` is torchvision's:
    one value per block, from the block's input and output planes, used by
    both convs. ``rule="conv"`` recomputes it per conv from that conv's own
    input and output planes (the reference's rule); the two differ only in the
    second conv of a downsampling block (230 / 288, 460 / 576, 921 / 1152)."""
    if rule not in MIDPLANES_RULES:
        raise ValueError("midplanes must be 'block' or 'conv', got %r" % (rule,))
    mids = {}
    for idx, size in layer_sizes.items():
        cin, planes = LAYER_CHANNELS[idx]
        for j in range(size):
            inp = cin if j == 0 else planes
            name = "layer%d.%d" % (idx - 1, j)
            mids[name + ".conv1"] = tv_midplanes(inp, planes)
            mids[name + ".conv2"] = tv_midplanes(inp if rule == "block" else planes, planes)
    return mids


def tv_state_mids(state_dict) -> Dict[str, int]:
    """The mid-channel count of every (2+1)D conv a torchvision-layout state
    dict holds, from the shape of its spatial conv's weight."""
    mids = {}
    for k, v in state_dict.items():
        parts = k.split(".")
        if (len(parts) == 6 and parts[0].startswith("layer") and parts[2] in ("conv1", "conv2")
                and parts[3:] == ["0", "0", "weight"] and hasattr(v, "shape") and len(v.shape) == 5):
            mids[".".join(parts[:3])] = int(v.shape[0])
    return mids


def _conv2plus1d(in_planes, out_planes, mid, stride, eps):
    return nn.Sequential(
        nn.Conv3d(in_planes, mid, (1, 3, 3), stride=(1, stride, stride), padding=(0, 1, 1),
                  bias=False),
        nn.BatchNorm3d(mid, eps=eps),
        nn.ReLU(),
        nn.Conv3d(mid, out_planes, (3, 1, 1), stride=(stride, 1, 1), padding=(1, 0, 0),
                  bias=False))


class TVBasicBlock(nn.Module):
    """torchvision's video ``BasicBlock`` over ``Conv2Plus1D``."""

    def __init__(self, in_planes, planes, mid1, mid2, stride=1, eps=DEFAULT_BN_EPS):
        super().__init__()
        self.conv1 = nn.Sequential(_conv2plus1d(in_planes, planes, mid1, stride, eps),
                                   nn.BatchNorm3d(planes, eps=eps), nn.ReLU())
        self.conv2 = nn.Sequential(_conv2plus1d(planes, planes, mid2, 1, eps),
                                   nn.BatchNorm3d(planes, eps=eps))
        self.relu = nn.ReLU()
        self.downsample = None
        if stride != 1 or in_planes != planes:
            self.downsample = nn.Sequential(
                nn.Conv3d(in_planes, planes, 1, stride=(stride, stride, stride), bias=False),
                nn.BatchNorm3d(planes, eps=eps))

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        res = x if self.downsample is None else self.downsample(x)
        return self.relu(out + res)


class TVVideoResNet(nn.Module):
    """Layers [start_idx, end_idx] of torchvision's R(2+1)D ``VideoResNet``;
    the state-dict keys of the built range are torchvision's own. ``mids``
    names a (2+1)D conv's mid-channel count (``tv_block_mids`` /
    ``tv_state_mids``); convs it does not name follow ``midplanes``."""

    arch = "torchvision"

    def __init__(self, start_idx, end_idx, num_classes, layer_sizes: Dict[int, int],
                 midplanes: str = "block", bn_eps: float = DEFAULT_BN_EPS,
                 mids: Optional[Dict[str, int]] = None):
        super().__init__()
        if not 1 <= start_idx <= end_idx <= 5:
            raise ValueError("layer range must satisfy 1 <= start <= end <= 5, "
                             "got %d..%d" % (start_idx, end_idx))
        self.start_idx, self.end_idx = start_idx, end_idx
        self.num_classes = num_classes
        self.bn_eps = float(bn_eps)
        table = tv_block_mids({i: layer_sizes[i] for i in range(max(2, start_idx), end_idx + 1)},
                              midplanes)
        table.update({k: int(v) for k, v in (mids or {}).items() if k in table})
        self.mids = table
        for idx in range(start_idx, end_idx + 1):
            if idx == 1:
                self.stem = nn.Sequential(
                    nn.Conv3d(3, TV_STEM_MID, (1, 7, 7), stride=(1, 2, 2), padding=(0, 3, 3),
                              bias=False),
                    nn.BatchNorm3d(TV_STEM_MID, eps=bn_eps), nn.ReLU(),
                    nn.Conv3d(TV_STEM_MID, 64, (3, 1, 1), padding=(1, 0, 0), bias=False),
                    nn.BatchNorm3d(64, eps=bn_eps), nn.ReLU())
                continue
            cin, planes = LAYER_CHANNELS[idx]
            blocks = []
            for j in range(layer_sizes[idx]):
                name = "layer%d.%d" % (idx - 1, j)
                blocks.append(TVBasicBlock(cin if j == 0 else planes, planes,
                                           table[name + ".conv1"], table[name + ".conv2"],
                                           stride=2 if (j == 0 and idx > 2) else 1, eps=bn_eps))
            setattr(self, "layer%d" % (idx - 1), nn.Sequential(*blocks))
        if end_idx == 5:
            self.avgpool = nn.AdaptiveAvgPool3d(1)
            self.fc = nn.Linear(512, num_classes)

    def key_prefixes(self) -> List[str]:
        """State-dict key prefixes of the built range."""
        out = ["stem." if i == 1 else "layer%d." % (i - 1)
               for i in range(self.start_idx, self.end_idx + 1)]
        return out + (["fc."] if self.end_idx == 5 else [])

    def forward(self, x):
        for idx in range(self.start_idx, self.end_idx + 1):
            x = self.stem(x) if idx == 1 else getattr(self, "layer%d" % (idx - 1))(x)
        if self.end_idx == 5:
            x = self.fc(self.avgpool(x).flatten(1))
        return x


def _unwrap_state(state):
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        return state["state_dict"]
    return state


def load_torchvision_state_dict(model: TVVideoResNet, state, strict: bool = True):
    """Load a torchvision-layout R(2+1)D state dict (raw, or wrapped as
    ``{"state_dict": ...}``) restricted to the range ``model`` builds;
    ``num_batches_tracked`` entries are accepted. Raises a ValueError naming
    the first missing key, the first unexpected key (within the built range's
    prefixes) or the first key whose shape differs, with both shapes."""
    state = _unwrap_state(state)
    if not isinstance(state, dict):
        raise ValueError("expected a state dict, got %s" % type(state).__name__)
    if getattr(model, "arch", "reference") != "torchvision":
        raise ValueError("load_torchvision_state_dict needs a model built with "
                         "arch='torchvision'")
    ref_keys = [k for k in state if k.startswith(("res2plus1d.", "linear."))]
    if ref_keys and not any(k.startswith(("stem.", "layer", "fc.")) for k in state):
        raise ValueError("the checkpoint holds reference-format keys (first: %r): load it with "
                         "arch='reference', not arch='torchvision'" % ref_keys[0])
    prefixes = tuple(model.key_prefixes())
    keep = {k: v for k, v in state.items() if k.startswith(prefixes)}
    own = model.state_dict()
    if strict:
        for k in own:
            if k not in keep and not k.endswith("num_batches_tracked"):
                raise ValueError("torchvision checkpoint: missing key %r (layers %d..%d)"
                                 % (k, model.start_idx, model.end_idx))
        for k in keep:
            if k not in own:
                raise ValueError("torchvision checkpoint: unexpected key %r (layers %d..%d; "
                                 "another depth or layout?)"
                                 % (k, model.start_idx, model.end_idx))
    for k, v in keep.items():
        if k in own and tuple(v.shape) != tuple(own[k].shape):
            if k == "fc.weight" and tuple(v.shape[1:]) == tuple(own[k].shape[1:]):
                raise ValueError("torchvision checkpoint: fc.weight has %d rows but the model "
                                 "was built with num_classes %d: set num_classes to %d"
                                 % (v.shape[0], own[k].shape[0], v.shape[0]))
            raise ValueError("torchvision checkpoint: shape mismatch at %r: checkpoint %s, "
                             "model %s" % (k, tuple(v.shape), tuple(own[k].shape)))
    keep = {k: v for k, v in keep.items() if k in own}
    return model.load_state_dict(keep, strict=False)
