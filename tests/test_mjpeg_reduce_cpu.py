"""Reduced-size MJPEG decode (``reduce`` = 2, 4, 8: libjpeg's ``scale_denom``,
PIL's ``draft``) on the CPU: the IDCT mirror against box means of the fp64 ideal
IDCT and against PIL's own reduced luma, the surface layout, MjpegDecoder on a
CPU device against the clip mirror fed with the oracle's reduced planes, the
``"auto"`` rule, and a reference-free pin of the geometry handed downstream.

``python tests/test_mjpeg_reduce_cpu.py --write-golden`` (needs PIL) writes
tests/golden/mjpeg/<name>_draft<s>_luma.npy: per golden stream and s, PIL's
``Image.draft("L", (W // s, H // s))`` luma of its two frames."""
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rnb_amd.models.r2p1d.decoder import MjpegDecoder, make_decoder  # noqa: E402
from rnb_amd.ops import video as vops  # noqa: E402
from rnb_amd.utils import mjpeg  # noqa: E402
from test_chroma_cpu import GOLDEN_CHROMA, chroma_frames  # noqa: E402
from test_mjpeg_cpu import (GOLDEN, GOLDEN_STREAMS, SHAPES, check_band, frame_bytes,  # noqa: E402
                            idct_inputs, records_tensor)

CPU = torch.device("cpu")
REDUCES = (2, 4, 8)
# (W, H, sampling) of the IDCT cases: test_mjpeg_cpu's shapes, one 4:2:2 and one 4:4:4
IDCT_CASES = [(W, H, "420") for W, H in SHAPES] + [(52, 37, "422"), (37, 26, "444")]
# name -> (W, H) of all seven golden streams
ALL_GOLDEN = dict({k: v[:2] for k, v in GOLDEN_STREAMS.items()},
                  **{k: v[:2] for k, v in GOLDEN_CHROMA.items()})
# PIL does not reduce the 7 x 9 stream by 8 (a requested size of 0 x 1)
DRAFT_CASES = [(name, s) for name in sorted(ALL_GOLDEN) for s in REDUCES
               if not (name == "ramp_q30_444" and s == 8)]
# MjpegDecoder against a reference that may round a tie differently, by one level
# in Y and in one chroma plane at once: (1 + 1.772) / (255 * 0.217) = 0.0501 after
# normalisation (test_gpu_mjpeg.MIRROR_TOL and its argument)
MIRROR_TOL = 0.051


def box_mean(plane, s):
    """numpy box mean over s x s of an fp64 plane whose sides are multiples of 8."""
    h, w = plane.shape
    return plane.reshape(h // s, s, w // s, s).mean(axis=(1, 3))


def reduce_inputs(W, H, sampling):
    """kind -> [(coefs, qt)] x 6 frames: ``idct_inputs`` for 4:2:0; for the other
    samplings encoder output of noise frames and random coefficients far outside
    [0, 255], a different table on every frame."""
    if sampling == "420":
        return idct_inputs(W, H)
    mw, mh, _ = mjpeg.geometry(W, H, sampling)
    nb = mjpeg.mcu_blocks(sampling) * mw * mh
    tables = [np.stack([np.clip(mjpeg.QT_LUMA * (i + 1) // 3, 1, 255),
                        np.clip(mjpeg.QT_CHROMA * (i + 2) // 4, 1, 255)]).astype(np.uint16)
              for i in range(6)]
    rng = np.random.default_rng(W * H)
    noise = [(mjpeg.encode_frame(*f, tables[i], sampling=sampling)[1], tables[i][[0, 1, 1]])
             for i, f in enumerate(chroma_frames(W, H, 6, 40 + W, sampling))]
    clamp = []
    for i in range(6):
        c = rng.integers(-1023, 1024, (nb, 64)).astype(np.int16)
        c[:, 0] = np.where(np.arange(nb) % 2 == 0, 1016, -1024)
        clamp.append((c, tables[i][[0, 1, 1]]))
    return dict(noise=noise, clamp=clamp)


def reduced_ideal_planes(frames, mw, mh, sampling, s):
    """The oracle: ``mjpeg.idct_planes_f64`` at full size, then a numpy box mean;
    a flat list (Y0, Cb0, Cr0, Y1, ...)."""
    return [box_mean(p, s) for c, q in frames
            for p in mjpeg.idct_planes_f64(c, q, mw, mh, sampling)]


# -- 1. the mirror against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("W,H,sampling", IDCT_CASES)
def test_reduced_idct_mirror_against_box_means_of_fp64(W, H, sampling):
    mw, mh, rb = mjpeg.geometry(W, H, sampling)
    for kind, frames in reduce_inputs(W, H, sampling).items():
        rec = records_tensor(frames)
        for s in REDUCES:
            got = vops.jpeg_idct(rec, 6, mw, mh, sampling=sampling, reduce=s).numpy()
            assert got.shape == (6 * vops.jpeg_frame_bytes(mw, mh, sampling, s)[1],)
            check_band(got, reduced_ideal_planes(frames, mw, mh, sampling, s),
                       "%dx%d %s %s reduce %d" % (W, H, sampling, kind, s),
                       tie_only=kind == "dc_only")
            if kind == "clamp" and s < 8:
                assert (got == 0).any() and (got == 255).any()
        # reduce=1 is the full-size decode, byte for byte
        assert torch.equal(vops.jpeg_idct(rec, 6, mw, mh, sampling=sampling, reduce=1),
                           vops.jpeg_idct(rec, 6, mw, mh, sampling=sampling))
    for bad in (0, 3, 16, "2", 2.5, True, None):
        with pytest.raises(ValueError, match="reduce"):
            vops.jpeg_idct(torch.zeros(rb, dtype=torch.uint8), 1, mw, mh, sampling=sampling,
                           reduce=bad)
    with pytest.raises(ValueError, match="outside"):
        vops.jpeg_idct(torch.zeros(rb - 16, dtype=torch.uint8), 1, mw, mh, sampling=sampling,
                       reduce=2)


# -- 2. against PIL -----------------------------------------------------------------------------
def golden_frames(name):
    """[(coefs, qt)] of a golden stream's two frames (numpy reference decoder),
    and (mw, mh, sampling)."""
    path = os.path.join(GOLDEN, name + ".mjpeg")
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    refs = [mjpeg.decode_reference(frame_bytes(data, idx, i), planes=False) for i in range(2)]
    return [(r["coefs"], r["qt"]) for r in refs], (idx.mw, idx.mh, idx.sampling)


def reduced_luma(surf, i, W, H, mw, mh, sampling, s):
    """Frame ``i``'s luma corner ceil(W / s) x ceil(H / s) of a reduced surface."""
    hs, vs = vops.sampling_factors(sampling)
    N = 8 // s
    fb = vops.jpeg_frame_bytes(mw, mh, sampling, s)[1]
    y = surf[i * fb:i * fb + N * N * hs * vs * mw * mh].reshape(N * vs * mh, N * hs * mw)
    return y[:-(-H // s), :-(-W // s)]


@pytest.mark.parametrize("name,s", DRAFT_CASES)
def test_reduced_mirror_luma_against_pils_draft(name, s):
    W, H = ALL_GOLDEN[name]
    lumas = np.load(os.path.join(GOLDEN, "%s_draft%d_luma.npy" % (name, s)))
    assert lumas.shape == (2, -(-H // s), -(-W // s)) and lumas.dtype == np.uint8
    frames, (mw, mh, sampling) = golden_frames(name)
    surf = vops.jpeg_idct(records_tensor(frames), 2, mw, mh, sampling=sampling, reduce=s).numpy()
    for i in range(2):
        d = np.abs(reduced_luma(surf, i, W, H, mw, mh, sampling, s).astype(int)
                   - lumas[i].astype(int))
        print(name, s, i, "max |mirror luma - PIL draft luma| =", d.max(), "mean", d.mean())
        # the rounded box mean of the fp64 IDCT is within 1 level of PIL's draft; the fp32
        # tie band adds one
        assert d.max() <= 2


# -- 3. surface layout ----------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", [1, 2, 4, 8])
@pytest.mark.parametrize("sampling", ["420", "422", "444"])
def test_reduced_surface_layout(sampling, reduce):
    """Plane sizes, plane offsets and frame bytes; and flat blocks of a value per
    block land where ``jpeg_surface_planes`` says (2 frames, 3 x 2 MCUs)."""
    mw, mh = 3, 2
    hs, vs = vops.sampling_factors(sampling)
    N, B, n = 8 // reduce, hs * vs + 2, mw * mh
    rb, fb = vops.jpeg_frame_bytes(mw, mh, sampling, reduce)
    assert rb == 384 + 128 * B * n
    assert rb == vops.jpeg_frame_bytes(mw, mh, sampling)[0]        # the records do not change
    assert fb == N * N * B * n
    pl = vops.jpeg_surface_planes(mw, mh, sampling, reduce)
    ysize = (N * vs * mh) * (N * hs * mw)
    csize = (N * mh) * (N * mw)
    assert pl == vops.YuvPlanes(0, ysize, ysize + csize, N * hs * mw, N * mw, N * mw, 1)
    assert ysize + 2 * csize == fb
    if reduce == 1:
        assert pl == vops.jpeg_surface_planes(mw, mh, sampling)
    frames = []
    for f in range(2):
        c = np.zeros((B * n, 64), dtype=np.int16)
        c[:, 0] = (np.arange(B * n) * 5 + 40 * f) % 200 - 100      # flat blocks: DC / 8 + 128
        frames.append((c, np.full((3, 64), 8, dtype=np.uint16)))
    surf = vops.jpeg_idct(records_tensor(frames), 2, mw, mh, sampling=sampling,
                          reduce=reduce).numpy()
    assert surf.shape == (2 * fb,)
    for f, (c, _) in enumerate(frames):
        want = (c[:, 0].astype(np.int64) + 128).astype(np.uint8)
        fr = surf[f * fb:(f + 1) * fb]
        for off, stride, rows, cols, first in ((pl.y, pl.y_stride, vs * mh, hs * mw, 0),
                                               (pl.u, pl.u_stride, mh, mw, hs * vs * n),
                                               (pl.v, pl.v_stride, mh, mw, (hs * vs + 1) * n)):
            plane = fr[off:off + rows * N * stride].reshape(rows, N, cols, N)
            blocks = want[first:first + rows * cols].reshape(rows, 1, cols, 1)
            assert np.array_equal(plane, np.broadcast_to(blocks, plane.shape))
    for fn in (vops.jpeg_surface_planes, vops.jpeg_frame_bytes):
        with pytest.raises(ValueError, match="reduce"):
            fn(mw, mh, sampling, 3)


# -- 4. the decoder end to end on a CPU device ---------------------------------------------------
def oracle_clips(path, starts, F, s, out_w, out_h, crop, filter):
    """``yuv420_to_clip``'s mirror on the rounded box means of ``decode_reference``'s
    fp64 planes, ``crop`` (one box or one per row, in full-size pixels) divided by s."""
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    clips = crop if isinstance(crop, list) else None
    surf = []
    for st in starts:
        for f in range(F):
            planes = mjpeg.decode_reference(frame_bytes(data, idx, st + f))["planes_f64"]
            surf += [np.clip(np.rint(box_mean(p, s)), 0, 255).astype(np.uint8).reshape(-1)
                     for p in planes]
    surf = torch.from_numpy(np.concatenate(surf))
    fb = vops.jpeg_frame_bytes(idx.mw, idx.mh, idx.sampling, s)[1]
    if clips is None:
        offsets, boxes = [i * F * fb for i in range(len(starts))], tuple(c / s for c in crop)
    else:                                           # views: every box on every clip, clip-major
        offsets = [i * F * fb for i in range(len(starts)) for _ in clips]
        boxes = [tuple(c / s for c in b) for _ in starts for b in clips]
    return vops.yuv420_to_clip(surf, offsets, F, -(-idx.width // s), -(-idx.height // s), fb,
                               vops.jpeg_surface_planes(idx.mw, idx.mh, idx.sampling, s),
                               out_w, out_h, crop=boxes, matrix="jfif", filter=filter,
                               sampling=idx.sampling)


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    """64x48 4:2:0 without restart markers, 46x34 4:2:0 with them, 52x37 4:2:2."""
    from test_mjpeg_cpu import noise_frames, ramp_frames
    d = tmp_path_factory.mktemp("reduce")
    mjpeg.write_mjpeg(str(d / "a.mjpeg"), ramp_frames(64, 48, 12), quality=85)
    mjpeg.write_mjpeg(str(d / "b.mjpeg"), noise_frames(46, 34, 12, 5), quality=80,
                      restart_interval=2)
    mjpeg.write_mjpeg(str(d / "c.mjpeg"), chroma_frames(52, 37, 12, 9, "422"), quality=80,
                      sampling="422")
    return {"a": (str(d / "a.mjpeg"), 64, 48), "b": (str(d / "b.mjpeg"), 46, 34),
            "c": (str(d / "c.mjpeg"), 52, 37)}


@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_cpu_decoder_with_reduce_equals_the_oracle_through_the_clip_mirror(streams, name, s):
    from rnb_amd.models.r2p1d.decoder import view_boxes
    path, W, H = streams[name]
    F, out_w, out_h = 3, 12, 8
    side = min(W, H)
    center = ((W - side) / 2.0, (H - side) / 2.0, float(side), float(side))
    views = {"short_side": 16, "views": 3}
    for crop, boxes, filter in (("center", center, "bilinear"),
                                (views, view_boxes(W, H, out_w, out_h, 16, 3), "antialias"),
                                ("full", (0.0, 0.0, float(W), float(H)), "antialias")):
        dec = MjpegDecoder(CPU, clip_length=F, height=out_h, width=out_w, dtype=torch.float32,
                           crop=crop, filter=filter, reduce=s)
        vid, n = dec.probe(path)
        assert n == 12 and dec.reduce_of(vid) == s and dec.reduce == s
        got = dec.decode(vid, [0, 7])
        want = oracle_clips(path, [0, 7], F, s, out_w, out_h, boxes, filter)
        assert got.shape == want.shape == (2 * dec.views, F, out_h, out_w, 4)
        err = (got - want).abs().max().item()
        print(name, s, crop, "max |decoder - oracle| =", err)
        assert err <= MIRROR_TOL, err
    # the other entropy modes produce the same records, hence the same clips
    for kw in (dict(entropy="gpu", subseq_bytes=0), dict(entropy="gpu", subseq_bytes=48)):
        other = MjpegDecoder(CPU, clip_length=F, height=out_h, width=out_w, dtype=torch.float32,
                             crop="full", filter="antialias", reduce=s, **kw)
        v, _ = other.probe(path)
        assert torch.equal(other.decode(v, [0, 7]), got)


def test_reduce_argument_and_factory():
    for bad in (0, 3, 16, "2", "Auto", 2.5, True, None):
        with pytest.raises(ValueError, match="reduce"):
            MjpegDecoder(CPU, reduce=bad)
        with pytest.raises(ValueError, match="reduce"):
            make_decoder("mjpeg", CPU, decoder_args={"reduce": bad})
    assert MjpegDecoder(CPU).reduce == 1
    dec = make_decoder("mjpeg", CPU, decoder_args={"reduce": "auto", "crop": "center"})
    assert isinstance(dec, MjpegDecoder) and dec.reduce == "auto"
    assert make_decoder("mjpeg", CPU, decoder_args={"reduce": 4}).reduce == 4
    dec.warmup(1)                                          # needs no file


# -- 5. the auto rule -------------------------------------------------------------------------------
THREE = {"short_side": 128, "views": 3}
AUTO_TABLE = [
    # W, H, crop, out_w, out_h -> s
    (340, 256, "full", 112, 112, 2),             # 170 x 128 >= 112; 85 x 64 is not
    (340, 256, "center", 112, 112, 2),           # 256 / 2 = 128
    (340, 256, THREE, 112, 112, 2),              # the window is 224: exactly 112 at 2
    (340, 256, {"short_side": 128, "views": 1}, 112, 112, 2),
    (340, 256, {"short_side": 112, "views": 3}, 112, 112, 2),        # window 256
    (340, 256, {"short_side": 160, "views": 3}, 112, 112, 1),        # window 179.2
    (1280, 720, "center", 112, 112, 4),          # 720 / 4 = 180; / 8 = 90
    (1280, 720, "full", 112, 112, 4),            # the height decides
    (1280, 720, THREE, 112, 112, 4),             # window 630: 157.5 at 4, 78.75 at 8
    (1920, 1080, "full", 112, 112, 8),           # 240 x 135
    (128, 128, "full", 112, 112, 1),             # 64 x 64 would be upscaled
    (223, 400, "center", 112, 112, 1),           # 223 / 2 = 111.5 < 112
    (224, 400, "center", 112, 112, 2),
    (64, 48, "full", 16, 16, 2),                 # 32 x 24 >= 16; 16 x 12 is not
    (64, 48, "full", 16, 12, 4),
    (64, 48, "full", 8, 6, 8),
]


@pytest.mark.parametrize("W,H,crop,out_w,out_h,s", AUTO_TABLE)
def test_auto_reduce_table(W, H, crop, out_w, out_h, s):
    dec = MjpegDecoder(CPU, height=out_h, width=out_w, crop=crop, reduce="auto")
    assert dec.auto_reduce(W, H) == s


def test_auto_reduce_is_decided_per_file_at_probe(streams):
    dec = MjpegDecoder(CPU, clip_length=2, height=16, width=16, dtype=torch.float32,
                       reduce="auto")
    va, _ = dec.probe(streams["a"][0])                     # 64 x 48 -> 2
    vb, _ = dec.probe(streams["b"][0])                     # 46 x 34: 23 x 17 -> 2
    assert (dec.reduce_of(va), dec.reduce_of(vb)) == (2, 2)
    small = MjpegDecoder(CPU, clip_length=2, height=12, width=8, dtype=torch.float32,
                         crop="center", reduce="auto")
    sa, _ = small.probe(streams["a"][0])                   # 48 / 4 = 12 -> 4
    sb, _ = small.probe(streams["b"][0])                   # 34 / 2 = 17; 34 / 4 = 8.5 -> 2
    assert (small.reduce_of(sa), small.reduce_of(sb)) == (4, 2)
    fixed = MjpegDecoder(CPU, clip_length=2, height=12, width=8, dtype=torch.float32,
                         crop="center", reduce=4)
    fa, _ = fixed.probe(streams["a"][0])
    assert torch.equal(small.decode(sa, [0, 3]), fixed.decode(fa, [0, 3]))
    with pytest.raises(KeyError):
        dec.reduce_of(99)


def test_reduce_config_loads():
    import json
    from rnb_amd.config import load_pipeline
    path = os.path.join(ROOT, "configs", "r2p1d-whole-mjpeg-3crop-reduce.json")
    base = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-mjpeg-3crop.json")))
    cfg = json.load(open(path))
    assert cfg["pipeline"][0].pop("decoder_args") == {"reduce": "auto"}
    assert cfg == base                                     # the -3crop config plus the key
    spec = load_pipeline(path)
    assert spec.steps[0].kwargs["decoder_args"] == {"reduce": "auto"}


# -- 6. the geometry handed downstream, without a reference -----------------------------------------
SLOPE = 4


@pytest.fixture(scope="module")
def ramps(tmp_path_factory):
    """Two 64x48 streams of non-wrapping linear luma ramps, Y = 2 + 4 x and
    Y = 30 + 4 y, flat chroma, quality 100."""
    d = tmp_path_factory.mktemp("ramps")
    yy, xx = np.mgrid[0:48, 0:64]
    flat = np.full((24, 32), 128, dtype=np.uint8)
    out = {}
    for name, y in (("x", 2 + SLOPE * xx), ("y", 30 + SLOPE * yy)):
        assert y.min() >= 0 and y.max() <= 255
        path = str(d / (name + ".mjpeg"))
        mjpeg.write_mjpeg(path, [(y.astype(np.uint8), flat, flat)] * 2, quality=100)
        out[name] = path
    return out


def geometry_pin(device, ramps, s, axis, **kw):
    """(distance, threshold) between ``reduce=s`` and ``reduce=1`` on a linear ramp
    along ``axis``, bilinear, the whole 64x48 frame to 32x24, on interior pixels:
    those whose taps are not edge-clamped in the reduced frame. Box mean and linear
    sampling commute on a linear ramp, so a decoder that hands the clip kernel the
    right frame size, planes and boxes gives the same picture up to rounding; the
    threshold is what a shift by a quarter of a reduced pixel would change,
    0.25 s slope levels, normalised with the largest of the three std."""
    W, H, out_w, out_h = 64, 48, 32, 24
    clips = []
    for r in (1, s):
        dec = MjpegDecoder(device, clip_length=2, height=out_h, width=out_w,
                           dtype=torch.float32, crop="full", reduce=r, **kw)
        vid, _ = dec.probe(ramps[axis])
        clips.append(dec.decode(vid, [0]).float().cpu())

    def interior(n_src, n_out):
        x = (np.arange(n_out) + 0.5) * (n_src / n_out) - 0.5       # full-size coordinate
        xr = (x + 0.5) / s - 0.5                                   # reduced coordinate
        return (xr >= 0) & (xr <= n_src // s - 1)
    mx, my = interior(W, out_w), interior(H, out_h)
    assert mx.sum() >= out_w // 2 and my.sum() >= out_h // 2
    a, b = (c[0, :, my][:, :, mx][..., :3] for c in clips)
    dist = (a - b).abs().max().item()
    thr = 0.25 * s * SLOPE / (255.0 * max(vops.KINETICS_STD))
    # the picture is a ramp: the pin is not vacuous
    span = a[..., 0].max().item() - a[..., 0].min().item()
    assert span > 10 * thr
    return dist, thr


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_reduced_geometry_pin_on_linear_ramps(ramps, s, axis):
    dist, thr = geometry_pin(CPU, ramps, s, axis)
    print("reduce %d along %s: distance %.4f, quarter-pixel threshold %.4f (half: %.4f)"
          % (s, axis, dist, thr, thr / 2))
    assert dist <= thr, (dist, thr)
    # on the mirror the distance stays under half the threshold: quality 100 is enough
    assert dist <= thr / 2, (dist, thr)


def write_golden():
    from PIL import Image
    for name, s in DRAFT_CASES:
        W, H = ALL_GOLDEN[name]
        path = os.path.join(GOLDEN, name + ".mjpeg")
        data = np.fromfile(path, dtype=np.uint8)
        idx = mjpeg.read_index(path)
        lumas = []
        for i in range(2):
            im = Image.open(io.BytesIO(frame_bytes(data, idx, i)))
            im.draft("L", (W // s, H // s))
            assert im.mode == "L" and im.size == (-(-W // s), -(-H // s)), (name, s, im.size)
            lumas.append(np.asarray(im).copy())
        np.save(os.path.join(GOLDEN, "%s_draft%d_luma.npy" % (name, s)), np.stack(lumas))
        print(name, s, lumas[0].shape)


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        write_golden()
