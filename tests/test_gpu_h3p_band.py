"""Frame-band form of the pixel-major temporal h3 kernel (csrc/conv_h3p.hip).

Clips longer than the kernel's compiled frame count run in bands of 8 output
frames: a task is (16-pixel tile, clip, band) and loads the band's frames plus
one halo frame on either side per 32-channel chunk. Checked as the one-band
form is in tests/test_gpu_h3.py (the same four assertions, the same bounds):
bit-exact on small integers with residual + ReLU, zero padding channels, the
epilogue's per-video BN sums against fp64 sums of the output, and the input BN
+ ReLU on load against the fp64 conv of the applied input -- where a halo
frame outside the clip must contribute nothing although the BN would turn its
zeros into the shift. Then the halo in both directions on planted values, a
forced single pixel range (bands of one clip on different waves, task runs
across clips and videos), and the shapes the predicate declines.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAND = 8            # output frames per task of every banded instantiation

# (T, H, W), Cin, Cout
BAND_SHAPES = [((16, 4, 4), 144, 64),      # two bands, smallest case
               ((16, 4, 8), 83, 64),       # Cin_p 96: the half-empty last chunk
               ((32, 4, 4), 48, 64),       # four bands, two chunks
               ((8, 4, 8), 288, 128),      # the 32-channel-slice form at 16-frame clips
               ((16, 4, 4), 288, 64)]      # the 32-channel-slice form, banded


def _layer(cin, cout, relu=True, integer=False, seed=0, w=None, b=None):
    """A 3x1x1 stride-1 temporal layer with Cin_p padded to 16 channels, as
    the engine builds the stem's temporal conv (83 -> Cin_p 96)."""
    from rnb_amd.ops.conv import ConvGeom
    from rnb_amd.ops.conv_f32 import F32_ALIGN, ConvLayerF32
    g = torch.Generator().manual_seed(seed)
    if w is None:
        if integer:
            w = torch.randint(-2, 3, (cout, cin, 3, 1, 1), generator=g).float()
            b = torch.randint(-4, 5, (cout,), generator=g).float()
        else:
            w = torch.randn((cout, cin, 3, 1, 1), generator=g) * (2.0 / (3 * cin)) ** 0.5
            b = torch.randn(cout, generator=g) * 0.1
    geom = ConvGeom(cin=cin, cout=cout, kernel=(3, 1, 1), stride=(1, 1, 1), padding=(1, 0, 0),
                    align=F32_ALIGN, cin_pad=(cin + 15) // 16 * 16)
    return ConvLayerF32(w, b, geom, relu, DEV, "h3pband")


def _input(n, thw, cin_p, cin, integer=False, seed=1):
    g = torch.Generator().manual_seed(seed)
    if integer:
        x = torch.randint(-3, 4, (n,) + thw + (cin_p,), generator=g).float()
    else:
        x = torch.randn((n,) + thw + (cin_p,), generator=g)
    x[..., cin:] = 0
    return x.to(DEV)


def _ref64(layer, x, res=None):
    """fp64 CPU conv of the layer (the exact answer fp32 is measured against)."""
    g = layer.geom
    xin = x[..., :g.cin].double().cpu().permute(0, 4, 1, 2, 3)
    y = F.conv3d(xin, layer.w_ref.double().cpu(), layer.b_ref.double().cpu(),
                 stride=g.stride, padding=g.padding).permute(0, 2, 3, 4, 1)
    if res is not None:
        y = y + res[..., :g.cout].double().cpu()
    if layer.relu:
        y = torch.relu(y)
    return y


def _h3p_ids(layer, shape):
    from rnb_amd.ops.conv_f32 import H3P_BASE, H3P_BPC
    return [H3P_BASE + i for i in range(len(H3P_BPC))] if layer.h3p_ok(shape) else []


@pytest.mark.parametrize("thw,cin,cout", BAND_SHAPES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_h3p_band_exact_integers_stats_and_affine(thw, cin, cout):
    layer = _layer(cin, cout, relu=True, integer=True)
    x = _input(3, thw, layer.geom.cin_p, cin, integer=True)
    res = _input(3, thw, layer.geom.cout_p, cout, integer=True, seed=3)
    ref = _ref64(layer, x, res).float()
    assert layer.h3p_ok(x.shape)
    ids = _h3p_ids(layer, x.shape)
    assert ids
    for cid in ids:
        y = layer.forward_hip(x, res, config=cid)
        torch.cuda.synchronize()
        assert torch.equal(y[..., :cout].cpu(), ref), cid
        assert torch.all(y[..., cout:] == 0), cid
    lay2 = _layer(cin, cout, relu=False)
    xf = _input(3, thw, lay2.geom.cin_p, cin)
    seg = torch.tensor([0, 2, 2], dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(11)
    cp = lay2.geom.cin_p
    ss = torch.empty((3, 2, cp), dtype=torch.float32)
    ss[:, 0] = torch.rand((3, cp), generator=g) + 0.5
    ss[:, 1] = torch.randn((3, cp), generator=g) * 0.5
    ss = ss.to(DEV)
    xa = torch.relu(xf * ss[seg.long(), 0][:, None, None, None, :] +
                    ss[seg.long(), 1][:, None, None, None, :])
    ref_a = _ref64(lay2, xa)
    scale = ref_a.abs().max().item()
    for cid in ids:
        sums = torch.zeros((3, 2, lay2.geom.cout_p), dtype=torch.float64, device=DEV)
        y = lay2.forward_hip(xf, config=cid, out_stats=(sums, seg))
        torch.cuda.synchronize()
        yd = y[..., :cout].double().cpu()
        for v, (a, b) in enumerate([(0, 1), (1, 1), (1, 3)]):
            part = yd[a:b].reshape(-1, cout)
            got = sums[v, :, :cout].cpu()
            assert ((got[0] - part.sum(0)).abs() <= 1e-6 * part.abs().sum(0) + 1e-9).all(), cid
            assert torch.allclose(got[1], (part * part).sum(0), rtol=1e-6, atol=1e-9), cid
        for ost in (None, (torch.zeros_like(sums), seg)):
            ya = lay2.forward_hip(xf, config=cid, in_affine=(ss, seg), out_stats=ost)
            torch.cuda.synchronize()
            err = (ya[..., :cout].double().cpu() - ref_a).abs().max().item()
            print("h3p band %s %d->%d cid %d affine err %.3e of scale %.3e"
                  % (thw, cin, cout, cid, err, scale))
            assert err <= 1e-5 * scale, (cid, err, scale)


@pytest.mark.parametrize("cin,cout,thw", [(144, 64, (16, 12, 8)), (288, 128, (8, 12, 12))])
def test_h3p_band_single_range_cross_video(monkeypatch, cin, cout, thw):
    """A forced single pixel range: 4 waves per channel slice, each a run of
    tasks over several clips and videos; at 16 frames the two bands of one
    clip's tile land on different waves at the wave boundaries, and the
    per-wave BN sums are flushed on every video change."""
    from rnb_amd.ops import conv_f32
    monkeypatch.setattr(conv_f32, "H3P_BPC", (-1, -3))
    layer = _layer(cin, cout, relu=True, integer=True)
    n = 5
    x = _input(n, thw, layer.geom.cin_p, cin, integer=True)
    res = _input(n, thw, layer.geom.cout_p, cout, integer=True, seed=3)
    ref = _ref64(layer, x, res).float()
    ids = _h3p_ids(layer, x.shape)
    assert ids
    for cid in ids:
        y = layer.forward_hip(x, res, config=cid)
        torch.cuda.synchronize()
        assert torch.equal(y[..., :cout].cpu(), ref), cid
    lay2 = _layer(cin, cout, relu=False)
    xf = _input(n, thw, lay2.geom.cin_p, cin)
    seg = torch.tensor([0, 0, 1, 3, 3], dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(5)
    cp = lay2.geom.cin_p
    ss = torch.empty((4, 2, cp), dtype=torch.float32)
    ss[:, 0] = torch.rand((4, cp), generator=g) + 0.5
    ss[:, 1] = torch.randn((4, cp), generator=g) * 0.5
    ss = ss.to(DEV)
    xa = torch.relu(xf * ss[seg.long(), 0][:, None, None, None, :] +
                    ss[seg.long(), 1][:, None, None, None, :])
    ref_a = _ref64(lay2, xa)
    scale = ref_a.abs().max().item()
    for cid in ids:
        sums = torch.zeros((4, 2, lay2.geom.cout_p), dtype=torch.float64, device=DEV)
        ya = lay2.forward_hip(xf, config=cid, in_affine=(ss, seg), out_stats=(sums, seg))
        torch.cuda.synchronize()
        yd = ya[..., :cout].double().cpu()
        err = (yd - ref_a).abs().max().item()
        assert err <= 1e-5 * scale, (cid, err, scale)
        for v, (a, b) in enumerate([(0, 2), (2, 3), (3, 3), (3, 5)]):
            part = yd[a:b].reshape(-1, cout)
            got = sums[v, :, :cout].cpu()
            assert ((got[0] - part.sum(0)).abs() <= 1e-6 * part.abs().sum(0) + 1e-9).all(), cid
            assert torch.allclose(got[1], (part * part).sum(0), rtol=1e-6, atol=1e-9), cid


@pytest.mark.parametrize("thw,cin,cout", [((16, 4, 4), 144, 64), ((32, 4, 4), 48, 64),
                                          ((16, 4, 4), 288, 64)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_h3p_band_halo_both_directions(thw, cin, cout):
    """One planted input value per case, integer weights with distinct taps
    and no bias: the last frame of band 0 reaches output frame BAND (of band
    1) through tap 0 only by band 1's leading halo frame; the first frame of
    band 1 reaches output frame BAND - 1 (of band 0) through tap 2 only by
    band 0's trailing halo frame. Exact."""
    g = torch.Generator().manual_seed(2)
    w = torch.randint(1, 4, (cout, cin, 3, 1, 1), generator=g).float()
    w[:, :, 1] += 3.0                      # taps differ: a wrong tap shows
    w[:, :, 2] += 7.0
    layer = _layer(cin, cout, relu=False, w=w, b=torch.zeros(cout))
    cp = layer.geom.cin_p
    ci, px = cin - 1, (1, 2)
    for frame, out_frame, tap in ((BAND - 1, BAND, 0), (BAND, BAND - 1, 2)):
        x = torch.zeros((2,) + thw + (cp,), device=DEV)
        x[1, frame, px[0], px[1], ci] = 3.0
        ref = _ref64(layer, x).float()
        want = 3.0 * w[:, ci, tap, 0, 0]
        assert torch.equal(ref[1, out_frame, px[0], px[1]], want)      # the test's own premise
        for cid in _h3p_ids(layer, x.shape):
            y = layer.forward_hip(x, config=cid)
            torch.cuda.synchronize()
            assert torch.equal(y[1, out_frame, px[0], px[1], :cout].cpu(), want), (cid, frame)
            assert torch.equal(y[..., :cout].cpu(), ref), (cid, frame)


def test_h3p_band_predicate_and_declined_frame_count():
    """The shapes above are offered; a frame count that is no multiple of the
    band is not, and the launcher refuses it with -2 on the host, before any
    launch."""
    from rnb_amd.ops.native import kernels
    for thw, cin, cout in BAND_SHAPES:
        lay = _layer(cin, cout)
        assert lay.h3p_ok((3,) + thw + (lay.geom.cin_p,)), (thw, cin, cout)
    k = kernels()
    assert k.conv_h3p_ok(16, 56, 56, 144, 64) and k.conv_h3p_ok(32, 56, 56, 96, 64)
    assert k.conv_h3p_ok(8, 28, 28, 288, 128) and k.conv_h3p_ok(16, 28, 28, 288, 128)
    assert not k.conv_h3p_ok(12, 56, 56, 144, 64) and not k.conv_h3p_ok(12, 28, 28, 288, 128)
    assert not k.conv_h3p_ok(16, 56, 56, 176, 64)          # weights past the LDS
    lay = _layer(144, 64)
    shape = (2, 12, 4, 4, lay.geom.cin_p)
    assert lay.h3t_ok(shape) and not lay.h3p_ok(shape)
    x = torch.zeros(shape, device=DEV)
    y = torch.zeros(lay.out_shape(shape), device=DEV)
    p = lay.params(x, y, None, h3t=True)
    _, _, s_in, s_out = lay.h3t_buffers()
    rc = k.lib.rnb_conv_h3p_launch(ctypes.byref(p), 1, None, None, None, 0, s_in, s_out,
                                   None, None)
    assert rc == -2
