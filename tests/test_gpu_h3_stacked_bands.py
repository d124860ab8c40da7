"""Row-band h3 kernels (conv_h3r_kernel, conv_h3q_kernel) with stacked bands:
a band is R consecutive rows of the N * T * H rows of the tensor, so it
crosses frames, clips and videos. Shapes are chosen so that bands cross
frames: 28 x 28 (one boundary per 256-px band), 14 x 14 (R > H: two
boundaries, partial last band), 15 x 13 (odd sizes, both patch pitches) and
7 x 7 (many frames, clips and videos per band). Launches this small fit one
round of blocks, where the launch keeps bands per frame: the tests switch
that rule off, so every launch here is stacked where the variant can be."""
import pytest
import torch

from test_gpu_f32 import DEV, _input, _layer, _ref64

pytestmark = pytest.mark.gpu

K, S, P = (1, 3, 3), (1, 1, 1), (0, 1, 1)
# (N, T, H, W)
SHAPES = [(2, 2, 28, 28), (3, 2, 14, 14), (2, 3, 15, 13), (5, 1, 7, 7)]
# + 12 one-clip videos on 7 x 7: 9 videos in a 63-row band, more than the
# epilogue sums from registers (X6D_MSEG_MAX 8): the tile is read back
SUM_SHAPES = SHAPES + [(12, 1, 7, 7)]
# clip -> video maps with an empty video inside the range: two videos per band
# where a clip has more rows than a band, three and more on 7 x 7 (a clip is 7
# rows of bands of 36 and more)
SEGS = {2: [0, 2], 3: [0, 2, 3], 5: [0, 2, 2, 3, 5], 12: list(range(12))}


@pytest.fixture(autouse=True)
def _stack_small_launches():
    from rnb_amd.ops.native import kernels
    kernels().conv_h3r_stack_small(True)
    yield
    kernels().conv_h3r_stack_small(False)


def _ids(layer, shape):
    from rnb_amd.ops.conv_f32 import H3R_BASE
    from rnb_amd.ops.native import kernels
    ids = [H3R_BASE + v for v in range(kernels().h3r_variants)
           if layer.h3r_fits(v, shape, efficient=False)]
    assert ids, shape
    return ids


def _crosses_frames(cid, shape):
    from rnb_amd.ops.conv_f32 import H3R_BASE
    from rnb_amd.ops.native import kernels
    N, T, H, W, _ = shape
    return kernels().conv_h3r_stacked(cid - H3R_BASE, N, T, H, W, 150)


@pytest.mark.parametrize("nthw", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stacked_bands_exact_integers(nthw):
    """Bit-exact on small integers against the fp64 conv, residual + ReLU,
    150 output channels (two channel tiles, the second partial)."""
    n, thw = nthw[0], tuple(nthw[1:])
    layer = _layer(64, 150, K, S, P, relu=True, integer=True)
    x = _input(n, thw, 64, 64, integer=True)
    res = _input(n, thw, layer.geom.cout_p, 150, integer=True, seed=3)
    ref = _ref64(layer, x, res).float()
    ids = _ids(layer, x.shape)
    assert any(_crosses_frames(c, x.shape) for c in ids)
    for cid in ids:
        y = layer.forward_hip(x, res, config=cid)
        torch.cuda.synchronize()
        assert torch.equal(y[..., :150].cpu(), ref), cid


@pytest.mark.parametrize("nthw", SUM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stacked_bands_per_video_sums(nthw):
    """Epilogue BN sums per video against fp64 sums of the stored output
    (1e-6 relative), with several videos and an empty one inside a band;
    the rows of videos without clips stay zero."""
    n, thw = nthw[0], tuple(nthw[1:])
    layer = _layer(64, 150, K, S, P, relu=False)
    x = _input(n, thw, 64, 64)
    segl = SEGS[n]
    nvid = segl[-1] + 1
    seg = torch.tensor(segl, dtype=torch.int32, device=DEV)
    for cid in _ids(layer, x.shape):
        sums = torch.zeros((nvid, 2, layer.geom.cout_p), dtype=torch.float64, device=DEV)
        y = layer.forward_hip(x, config=cid, out_stats=(sums, seg))
        torch.cuda.synchronize()
        yd = y[..., :150].double().cpu()
        got = sums[:, :, :150].cpu()
        for v in range(nvid):
            clips = [i for i, s in enumerate(segl) if s == v]
            if not clips:
                assert (got[v] == 0).all(), (cid, v)
                continue
            part = yd[clips].reshape(-1, 150)
            assert ((got[v, 0] - part.sum(0)).abs() <= 1e-6 * part.abs().sum(0) + 1e-9).all(), \
                (cid, v)
            assert torch.allclose(got[v, 1], (part * part).sum(0), rtol=1e-6, atol=1e-9), (cid, v)


@pytest.mark.parametrize("nthw", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stacked_bands_input_bn_across_videos(nthw):
    """Input BN + ReLU on load with a band's entries in different videos:
    mixed-sign scales and large positive shifts, so a separator or padding
    entry that received the affine would be a gross error; within 1e-5 of
    the fp64 conv of the applied input. A band whose clips are different
    videos with equal scale / shift rows (the per-entry path) gives the bits
    of the one-video call."""
    n, thw = nthw[0], tuple(nthw[1:])
    layer = _layer(64, 150, K, S, P, relu=False)
    x = _input(n, thw, 64, 64)
    segl = SEGS[n]
    nvid = segl[-1] + 1
    seg = torch.tensor(segl, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(11)
    ss = torch.empty((nvid, 2, 64), dtype=torch.float32)
    sign = torch.randint(0, 2, (nvid, 64), generator=g).float() * 2 - 1
    ss[:, 0] = sign * (torch.rand((nvid, 64), generator=g) + 0.5)
    ss[:, 1] = torch.rand((nvid, 64), generator=g) * 8 + 8
    ss = ss.to(DEV)
    xa = torch.relu(x * ss[seg.long(), 0][:, None, None, None, :] +
                    ss[seg.long(), 1][:, None, None, None, :])
    ref = _ref64(layer, xa)
    scale = ref.abs().max().item()
    one = torch.zeros(n, dtype=torch.int32, device=DEV)
    each = torch.arange(n, dtype=torch.int32, device=DEV)
    ss_same = ss[:1].expand(n, 2, 64).contiguous()
    for cid in _ids(layer, x.shape):
        sums = torch.zeros((nvid, 2, layer.geom.cout_p), dtype=torch.float64, device=DEV)
        for ost in (None, (sums, seg)):
            y = layer.forward_hip(x, config=cid, in_affine=(ss, seg), out_stats=ost)
            torch.cuda.synchronize()
            err = (y[..., :150].double().cpu() - ref).abs().max().item()
            assert err <= 1e-5 * scale, (cid, ost is not None, err, scale)
        y_one = layer.forward_hip(x, config=cid, in_affine=(ss_same, one)).clone()
        y_each = layer.forward_hip(x, config=cid, in_affine=(ss_same, each))
        torch.cuda.synchronize()
        assert torch.equal(y_one, y_each), cid


def test_stacked_bands_grid_sizes():
    """Blocks per launch from the launch's own rule. 28 x 28 in 256-px bands
    runs 9 rows a band (the 352-entry patch; not the 8-row fallback)."""
    from rnb_amd.ops.native import kernels
    k = kernels()
    assert k.conv_h3r_band_rows(7, 28, 28) == 9
    assert k.conv_h3r_blocks(7, 128, 4, 28, 28, 288) == 3186
    assert k.conv_h3r_blocks(3, 128, 4, 28, 28, 288) == 1792
    assert k.conv_h3r_blocks(7, 128, 2, 14, 14, 576) == 800
    assert k.conv_h3r_blocks(0, 128, 8, 56, 56, 144) == 7168
    assert k.conv_h3r_blocks(3, 128, 8, 56, 56, 144) == 7168
    # two 80-KiB blocks of the stacked 256-px kernel still share a CU
    assert k.conv_h3r_occupancy(7, True) == 2
    # a grid within one round of blocks stays per frame (4 bands a frame)
    k.conv_h3r_stack_small(False)
    assert not k.conv_h3r_stacked(7, 1, 4, 28, 28, 288)
    assert k.conv_h3r_blocks(7, 1, 4, 28, 28, 288) == 32
    assert k.conv_h3r_stacked(7, 128, 4, 28, 28, 288)
