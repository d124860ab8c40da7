"""Temporal frame-band h3 kernel (conv_h3t_kernel) with stacked pixel tiles
and tap skipping: pixel tile j covers [j P, j P + P) of the linear index clip
* HW + pixel over the whole launch, so a block holds rows of several clips
and videos; the patch holds the clip's T frames only and a tile issues a tap
only where its input frame exists. Shapes (the smallest at which each path
can go wrong):

- T 2 on 14 x 14, 3 clips: 588 pixels in five tiles of 128 (the last
  partial), 16-pixel tiles straddling clips (196 % 16 = 4); three tiles of 256
  under variant 0;
- T 4 on 7 x 7, 5 clips: HW < P, a block holds two or three clips; tp = frame
  (variants 0 and 3) and a wave per half of the clip (variants 1 and 2);
- T 8 on 6 x 6, 3 clips: end and middle frames in one wave, the second half of
  the clip mirrored (variants 0 and 3; 1 and 2 have no stacked form here);
- T 2 on 16 x 16: HW % P == 0, the launch's rule answers "per clip".

The tests ask for the stacked form wherever a variant has one (the launch's
own rule keeps per-clip tiles where stacking removes no block)."""
import pytest
import torch

import h3_two_level as tl
from test_gpu_f32 import DEV, _input, _ref64
from test_gpu_h3 import _tlayer
from test_gpu_h3_lo_path import _build, _exact_ref, _pad_res, _precondition

pytestmark = pytest.mark.gpu

# (N, T, H, W)
SHAPES = [(3, 2, 14, 14), (5, 4, 7, 7), (3, 8, 6, 6)]
# Cin 48: the second chunk's upper 16 channels are past Cin_p; Cout 80: one
# partial 128-channel tile / a partial second 64-channel tile, 144: more tiles
CHANNELS = [(48, 80), (64, 144)]
# clip -> video maps: blocks with one, two and three videos
SEGS = {3: [[0, 0, 1], [0, 1, 2]], 5: [[0, 0, 0, 1, 1], [0, 1, 2, 3, 4]]}


def _sid(s):
    return "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _stacked_form():
    from rnb_amd.ops.native import kernels
    kernels().conv_h3t_form(1)
    yield
    kernels().conv_h3t_form(0)


def _ids(layer, shape, need_stacked=True):
    """(config id, stacked) of every h3t variant that runs the shape."""
    from rnb_amd.ops.conv_f32 import H3T_BASE
    from rnb_amd.ops.native import kernels
    k = kernels()
    N, T, H, W, _ = shape
    assert layer.h3t_ok(shape)
    ids = [(H3T_BASE + v, k.conv_h3t_stacked(v, N, T, H, W, layer.geom.cout_p))
           for v in range(k.h3t_variants) if layer.h3t_fits(v, shape)]
    assert ids, shape
    if need_stacked:
        assert sum(s for _, s in ids) >= 2, (shape, ids)
    return ids


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("nthw", SHAPES + [(2, 2, 16, 16)], ids=_sid)
def test_h3t_stacked_exact_integers(nthw, cin, cout):
    """Bit-exact on small integers against the fp64 conv, residual + ReLU,
    padding channels zero."""
    n, thw = nthw[0], tuple(nthw[1:])
    layer = _tlayer(cin, cout, relu=True, integer=True)
    x = _input(n, thw, layer.geom.cin_p, cin, integer=True)
    res = _input(n, thw, layer.geom.cout_p, cout, integer=True, seed=3)
    ref = _ref64(layer, x, res).float()
    for cid, stk in _ids(layer, x.shape):
        y = layer.forward_hip(x, res, config=cid)
        torch.cuda.synchronize()
        assert torch.equal(y[..., :cout].cpu(), ref), (cid, stk)
        assert torch.all(y[..., cout:] == 0), (cid, stk)


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("nthw", SHAPES, ids=_sid)
def test_h3t_stacked_two_level_exact(nthw, cin, cout):
    """The two-level data of tests/h3_two_level.py (non-zero lo parts in the
    activations, then in the weights): bit-exact against the fp64 conv."""
    case = tl._case("temporal", cin, cout, tl.TEMPORAL, tuple(nthw[1:]), nthw[0], cin_pad16=True)
    for which in (1, 2):
        d = tl.make_data(case, which)
        layer = _build(case, d)
        x = d.x.to(DEV)
        _precondition(case, d, which, layer, x, d.res)
        ref = _exact_ref(layer, x, d.res)
        resd = _pad_res(layer, d.res)
        for cid, stk in _ids(layer, x.shape):
            y = layer.forward_hip(x, resd, config=cid)
            torch.cuda.synchronize()
            assert torch.equal(y[..., :cout].cpu(), ref), (which, cid, stk)


def _rows(nvid, cp, seed=11):
    """Per-video input BN rows: mixed-sign scales, large positive shifts."""
    g = torch.Generator().manual_seed(seed)
    ss = torch.empty((nvid, 2, cp), dtype=torch.float32)
    sign = torch.randint(0, 2, (nvid, cp), generator=g).float() * 2 - 1
    ss[:, 0] = sign * (torch.rand((nvid, cp), generator=g) + 0.5)
    ss[:, 1] = torch.rand((nvid, cp), generator=g) * 8 + 8
    return ss.to(DEV)


def _check_sums(sums, yd, segl, cout, tag):
    """Per-video sums against fp64 sums of the stored output, at the bound of
    tests/test_gpu_h3.py."""
    for v in range(segl[-1] + 1):
        clips = [i for i, s in enumerate(segl) if s == v]
        part = yd[clips].reshape(-1, cout)
        got = sums[v, :, :cout].cpu()
        assert ((got[0] - part.sum(0)).abs() <= 1e-6 * part.abs().sum(0) + 1e-9).all(), (tag, v)
        assert torch.allclose(got[1], (part * part).sum(0), rtol=1e-6, atol=1e-9), (tag, v)


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("nthw", SHAPES, ids=_sid)
def test_h3t_stacked_random_stats_and_input_bn(nthw, cin, cout):
    """Random data within 1e-5 of the fp64 conv; epilogue sums per video with
    one, two and three videos in a block; the input BN + ReLU on load with
    per-video rows of mixed-sign scales and large positive shifts, so a tap
    taken outside the clip or a row normalised as another video's is a gross
    error. A block whose clips are different videos with equal rows (the
    per-entry path) gives the bits of the one-video call."""
    n, thw = nthw[0], tuple(nthw[1:])
    layer = _tlayer(cin, cout, relu=False)
    cp = layer.geom.cin_p
    x = _input(n, thw, cp, cin)
    ref = _ref64(layer, x)
    scale = ref.abs().max().item()
    ids = _ids(layer, x.shape)
    for cid, stk in ids:
        y = layer.forward_hip(x, config=cid)
        torch.cuda.synchronize()
        err = (y[..., :cout].double().cpu() - ref).abs().max().item()
        print("h3t stacked %s cid %d stacked %d: err %.3e of %.3e" % (_sid(nthw), cid, stk, err,
                                                                     scale))
        assert err <= 1e-5 * scale, (cid, stk, err, scale)
    one = torch.zeros(n, dtype=torch.int32, device=DEV)
    each = torch.arange(n, dtype=torch.int32, device=DEV)
    for segl in SEGS[n]:
        nvid = segl[-1] + 1
        seg = torch.tensor(segl, dtype=torch.int32, device=DEV)
        ss = _rows(nvid, cp)
        xa = torch.relu(x * ss[seg.long(), 0][:, None, None, None, :] +
                        ss[seg.long(), 1][:, None, None, None, :])
        xa[..., cin:] = 0
        ref_a = _ref64(layer, xa)
        scale_a = ref_a.abs().max().item()
        for cid, stk in ids:
            sums = torch.zeros((nvid, 2, layer.geom.cout_p), dtype=torch.float64, device=DEV)
            y = layer.forward_hip(x, config=cid, out_stats=(sums, seg))
            torch.cuda.synchronize()
            _check_sums(sums, y[..., :cout].double().cpu(), segl, cout, (cid, stk, segl))
            for ost in (None, (torch.zeros_like(sums), seg)):
                ya = layer.forward_hip(x, config=cid, in_affine=(ss, seg), out_stats=ost)
                torch.cuda.synchronize()
                yd = ya[..., :cout].double().cpu()
                err = (yd - ref_a).abs().max().item()
                assert err <= 1e-5 * scale_a, (cid, stk, segl, ost is not None, err, scale_a)
                if ost is not None:
                    _check_sums(ost[0], yd, segl, cout, (cid, stk, segl, "affine"))
    ss_same = _rows(1, cp).expand(n, 2, cp).contiguous()
    for cid, stk in ids:
        y_one = layer.forward_hip(x, config=cid, in_affine=(ss_same, one)).clone()
        y_each = layer.forward_hip(x, config=cid, in_affine=(ss_same, each))
        torch.cuda.synchronize()
        assert torch.equal(y_one, y_each), (cid, stk)


def test_h3t_stacked_more_videos_than_summed_from_registers():
    """20 one-clip videos on 4 x 4 frames, T 2: a 128-pixel tile holds 8
    videos, the most that are summed from registers, and a 256-pixel tile 16:
    that block reads its rows back. Sums per video against fp64."""
    n, thw, cin, cout = 20, (2, 4, 4), 48, 80
    layer = _tlayer(cin, cout, relu=False)
    x = _input(n, thw, layer.geom.cin_p, cin)
    ref = _ref64(layer, x)
    segl = list(range(n))
    seg = torch.tensor(segl, dtype=torch.int32, device=DEV)
    for cid, stk in _ids(layer, x.shape):
        sums = torch.zeros((n, 2, layer.geom.cout_p), dtype=torch.float64, device=DEV)
        y = layer.forward_hip(x, config=cid, out_stats=(sums, seg))
        torch.cuda.synchronize()
        yd = y[..., :cout].double().cpu()
        assert (yd - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), (cid, stk)
        _check_sums(sums, yd, segl, cout, (cid, stk))


def test_h3t_stacked_range_guard_trips():
    """An input of magnitude 2^12 (2^18 after the scale, past fp16) sets the
    range flag in the stacked kernels; 2^9 does not."""
    from rnb_amd.ops.conv_f32 import RangeGuard
    from rnb_amd.ops.native import kernels
    n, thw, cin, cout = 3, (2, 14, 14), 48, 80
    layer = _tlayer(cin, cout, relu=True)
    guard = RangeGuard()
    guard.activate()
    try:
        g = torch.Generator().manual_seed(12)
        x = torch.randn((n,) + thw + (layer.geom.cin_p,), generator=g)
        x = x / x.abs().max()
        x[..., cin:] = 0
        for cid, stk in _ids(layer, x.shape):
            if not stk:
                continue
            guard.reset()
            layer.forward_hip((x * 2.0 ** 9).to(DEV), config=cid)
            torch.cuda.synchronize()
            assert not guard.tripped(), cid
            layer.forward_hip((x * 2.0 ** 12).to(DEV), config=cid)
            torch.cuda.synchronize()
            assert guard.tripped(), cid
    finally:
        kernels().h3_set_range_flag(0)


def test_h3t_tile_rule_and_grid_sizes():
    """The launch's own rule at 128 clips: conv4's temporal convs (T 2, 14 x
    14, 256 channels) under variant 2 run 25088 / 128 = 196 stacked tiles x 2
    channel tiles = 392 blocks (per clip 128 x 2 x 2 = 512); conv3's (T 4, 28
    x 28, 128 channels) under variant 0 run 100352 / 128 = 784 x 2 = 1568
    (per clip 128 x 7 x 2 = 1792). Per-clip tiles stay where stacking removes
    no block: HW % P == 0, or one clip."""
    from rnb_amd.ops.native import kernels
    k = kernels()
    k.conv_h3t_form(0)
    assert k.conv_h3t_stacked(2, 128, 2, 14, 14, 256)
    assert k.conv_h3t_blocks(2, 128, 2, 14, 14, 256) == 392
    assert k.conv_h3t_stacked(0, 128, 4, 28, 28, 128)
    assert k.conv_h3t_blocks(0, 128, 4, 28, 28, 128) == 1568
    k.conv_h3t_form(-1)
    assert k.conv_h3t_blocks(2, 128, 2, 14, 14, 256) == 512
    assert k.conv_h3t_blocks(0, 128, 4, 28, 28, 128) == 1792
    k.conv_h3t_form(0)
    # variant 3 at T 2: the (T + 2) x P patch of per-clip tiles does not fit
    assert k.conv_h3t_pixels(3, 2) == 0
    assert k.conv_h3t_stacked(3, 128, 2, 14, 14, 256)
    assert k.conv_h3t_blocks(3, 128, 2, 14, 14, 256) == 196 * 4
    assert k.conv_h3t_occupancy(3, True) == 2
    # HW % P == 0 (conv2: T 8, 56 x 56; here 16 x 16): no block to remove
    for v in range(3):
        assert not k.conv_h3t_stacked(v, 128, 8, 56, 56, 64), v
    for v in (1, 2):              # (variant 0 at T 2 has no per-clip form either)
        assert not k.conv_h3t_stacked(v, 128, 2, 16, 16, 256), v
    assert k.conv_h3t_blocks(2, 128, 2, 16, 16, 256) == 128 * 2 * 2
    # a grid within one round of blocks is stacked too (16 x 2 x 2 = 64 per clip)
    assert k.conv_h3t_stacked(2, 16, 2, 14, 14, 256)
    assert k.conv_h3t_blocks(2, 16, 2, 14, 14, 256) == 50
    # one clip: no block to remove
    assert not k.conv_h3t_stacked(2, 1, 2, 14, 14, 256)
    assert k.conv_h3t_blocks(2, 1, 2, 14, 14, 256) == 4
    # T 8 under the two-tile variants: no stacked form
    k.conv_h3t_form(1)
    assert not k.conv_h3t_stacked(1, 128, 8, 14, 14, 256)
    assert k.conv_h3t_stacked(0, 128, 8, 14, 14, 256)
