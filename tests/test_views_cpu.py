"""Short-side resize and three-crop views of the file-backed decoders, on the CPU:
the crop geometry against ``decode_oracle_views.py``, the op's box-per-clip form
against the fp64 oracles and against single-box calls, the decoders' row contract
(one staging, one IDCT, one clip call per request) and the loader's row counts.
``test_gpu_views.py`` takes its inputs from here."""
import itertools

import numpy as np
import pytest
import torch

import decode_oracle as orc
import decode_oracle_chroma as occ
import decode_oracle_views as ov
from rnb_amd.models.r2p1d import decoder as dmod
from rnb_amd.models.r2p1d.decoder import MjpegDecoder, Y4mDecoder, view_boxes
from rnb_amd.ops import video as vops
from rnb_amd.utils import mjpeg, y4m
from test_chroma_cpu import chroma_frames, y4m_planes

CPU = torch.device("cpu")
# non-dyadic short sides: each fits a 12 x 12 window into every 16..64 frame, a 16 x 12 into most
SWEEP_S = (12.1, 12.7, 13.3, 14.9, 16.1, 17.3, 18.9, 19.7, 21.1, 23.9, 27.7, 31.3)
# (id, W, H, out_w, out_h, S, axis): landscape, portrait, and a square frame whose
# non-square window leaves more room along y
FRAMES = [("landscape", 46, 34, 16, 12, 13.7, "x"), ("portrait", 34, 46, 16, 12, 17.3, "y"),
          ("square", 40, 40, 16, 12, 17.3, "y")]


def frame_case(name):
    return next(c for c in FRAMES if c[0] == name)


# -- 1. geometry ---------------------------------------------------------------------------------
def test_the_340x256_example():
    want = [(0.0, 16.0, 224.0, 224.0), (58.0, 16.0, 224.0, 224.0), (116.0, 16.0, 224.0, 224.0)]
    assert ov.boxes(340, 256, 112, 112, 128, 3) == want
    assert view_boxes(340, 256, 112, 112, 128, 3) == want
    assert view_boxes(340, 256, 112, 112, 128, 1) == [want[1]]


@pytest.mark.parametrize("name", [c[0] for c in FRAMES])
def test_views_follow_the_larger_free_length(name):
    _, W, H, ow, oh, S, axis = frame_case(name)
    assert ov.axis_of(W, H, ow, oh, S) == axis
    got, ref = view_boxes(W, H, ow, oh, S, 3), ov.boxes(W, H, ow, oh, S, 3)
    assert len(got) == 3
    k = 0 if axis == "x" else 1
    assert got[0][k] == 0.0 and got[0][k] < got[1][k] < got[2][k]          # left / top first
    assert got[0][1 - k] == got[1][1 - k] == got[2][1 - k]                  # centred across
    for g, r in zip(got, ref):
        assert ov.is_f32(g) and ov.close(g, r) and ov.inside_f32(g, W, H), (g, r)
    one = view_boxes(W, H, ow, oh, S, 1)
    assert len(one) == 1 and ov.close(one[0], ov.boxes(W, H, ow, oh, S, 1)[0])


def test_an_exact_tie_goes_to_x():
    got = view_boxes(40, 40, 12, 12, 16, 3)              # 30 x 30 windows: 10 free both ways
    assert got == [(0.0, 5.0, 30.0, 30.0), (5.0, 5.0, 30.0, 30.0), (10.0, 5.0, 30.0, 30.0)]
    assert got == ov.boxes(40, 40, 12, 12, 16, 3)


def write_y4m_file(tmp_path, W, H, frames, seed, sampling="420", name="v.y4m"):
    fr = y4m_planes(W, H, frames, seed, sampling)
    path = str(tmp_path / name)
    y4m.write_y4m(path, fr, sampling=sampling)
    return path, fr


def test_short_side_equal_to_the_output_is_center(tmp_path):
    for W, H in ((46, 34), (34, 46)):
        side = min(W, H)
        assert view_boxes(W, H, 12, 12, 12, 1) == [((W - side) / 2.0, (H - side) / 2.0,
                                                    float(side), float(side))]
    path, _ = write_y4m_file(tmp_path, 46, 34, 5, 11)
    for filt in vops.FILTERS:
        a = Y4mDecoder(CPU, clip_length=2, height=12, width=12, dtype=torch.float32,
                       crop={"short_side": 12}, filter=filt)
        b = Y4mDecoder(CPU, clip_length=2, height=12, width=12, dtype=torch.float32,
                       crop="center", filter=filt)
        assert a.views == 1 and b.views == 1
        assert torch.equal(a.decode(a.probe(path)[0], [3, 0]), b.decode(b.probe(path)[0], [3, 0]))


def test_every_fp32_box_passes_the_antialias_launchers_check():
    """W, H over 16..64 and a dozen non-dyadic S: the boxes are fp32 values, lie
    inside the frame by the launcher's double-precision sum, and are the
    definition's boxes to within the rounding."""
    n = refused = 0
    for W, H, S in itertools.product(range(16, 65), range(16, 65), SWEEP_S):
        for ow, oh in ((16, 12), (12, 12)):
            ref = ov.boxes(W, H, ow, oh, S, 3)
            got = view_boxes(W, H, ow, oh, S, 3)
            if ref is None:                 # the window is larger than the frame: both say so
                assert got is None, (W, H, S)
                refused += 1
                continue
            assert got is not None and len(got) == 3
            for g, r in zip(got, ref):
                assert ov.is_f32(g) and ov.inside_f32(g, W, H) and ov.close(g, r), (W, H, S, g, r)
            n += 3
    # 12 x 12 fits every frame at every S (S > 12); 16 x 12 does not when S < 16 W / min(W, H)
    assert n + 3 * refused == 49 * 49 * 12 * 2 * 3 and n >= 49 * 49 * 12 * 3 and refused > 1000


def test_refusals_name_their_cause(tmp_path):
    with pytest.raises(ValueError, match="views.*1 or 3.*2"):
        Y4mDecoder(CPU, crop={"short_side": 128, "views": 2})
    with pytest.raises(ValueError, match="flip"):
        MjpegDecoder(CPU, crop={"short_side": 128, "flip": True})
    with pytest.raises(ValueError, match="short_side.*positive"):
        Y4mDecoder(CPU, crop={"short_side": 0})
    with pytest.raises(ValueError, match="crop must be"):
        Y4mDecoder(CPU, crop="left")
    # a window larger than the frame (16 * 34 / 13.7 = 39.7 > 34): at probe, naming the file
    # and the field; the same decoder serves a frame it fits
    small, _ = write_y4m_file(tmp_path, 34, 46, 3, 1, name="small.y4m")
    path, _ = write_y4m_file(tmp_path, 46, 34, 3, 1, name="ok.y4m")
    dec = Y4mDecoder(CPU, clip_length=2, height=12, width=16, crop={"short_side": 13.7, "views": 3})
    with pytest.raises(ValueError) as e:
        dec.probe(small)
    assert "small.y4m" in str(e.value) and "'crop'" in str(e.value)
    mpath = str(tmp_path / "small.mjpeg")
    mjpeg.write_mjpeg(mpath, chroma_frames(34, 46, 2, 3, "420"))
    with pytest.raises(ValueError) as e:
        MjpegDecoder(CPU, clip_length=2, height=12, width=16, crop={"short_side": 13.7}).probe(mpath)
    assert "small.mjpeg" in str(e.value) and "'crop'" in str(e.value)
    assert dec.probe(path)[1] == 3
    with pytest.raises(ValueError):
        dec.probe(small)                                  # still refused, not remembered
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    with pytest.raises(ValueError, match="max_clips.*views"):
        R2P1DLoader(CPU, decoder="y4m", max_clips=2, warmup=0,
                    decoder_args={"crop": {"short_side": 128, "views": 3}})
    # the op: a box sequence of the wrong length, an antialias box outside the frame
    y, u, v = orc.noise_planes(46, 34, 2, 5)
    buf, stride, pl = orc.pack_i420(y, u, v, 6)
    t = torch.from_numpy(buf)
    good = (3.5, 1.25, 40.0, 30.0)
    with pytest.raises(ValueError, match="2 boxes for 3 clips"):
        vops.yuv420_to_clip(t, [0, 0, 0], 2, 46, 34, stride, pl, 16, 12, crop=[good, good])
    with pytest.raises(ValueError, match="antialias.*inside"):
        vops.yuv420_to_clip(t, [0, 0, 0], 2, 46, 34, stride, pl, 16, 12, filter="antialias",
                            crop=[good, (7.0, 1.25, 40.0, 30.0), good])
    with pytest.raises(ValueError, match="view ind"):
        d = Y4mDecoder(CPU, clip_length=2, height=12, width=16, crop={"short_side": 13.7, "views": 3})
        d.decode(d.probe(path)[0], [0, 0], views=[0, 3])


# -- 2. the mirror against the fp64 oracle -----------------------------------------------------------
# (id, matrix, sampling, W, H, frame case for out / S); the JFIF case is odd-sized
ORACLE_CASES = [("bt601_420", "bt601", "420", 46, 34), ("bt601_422", "bt601", "422", 46, 34),
                ("bt601_444", "bt601", "444", 34, 46), ("jfif_420_45x33", "jfif", "420", 45, 33)]
ORACLE_S = 13.7


def oracle_case(name, F=2, header=7):
    """(planes, buffer, stride, YuvPlanes, W, H, matrix, sampling, decoder boxes, exact boxes)."""
    _, matrix, sampling, W, H = next(c for c in ORACLE_CASES if c[0] == name)
    S = ORACLE_S if W > H else 17.3
    y, u, v = occ.noise_planes(W, H, F, orc.case_seed(name), matrix, sampling)
    buf, stride, pl = occ.pack_planar(y, u, v, header)
    return (y, u, v), buf, stride, pl, W, H, matrix, sampling, \
        view_boxes(W, H, 16, 12, S, 3), ov.boxes(W, H, 16, 12, S, 3)


def check_views_against_oracle(name, filt, device):
    (y, u, v), buf, stride, pl, W, H, matrix, sampling, boxes, exact = oracle_case(name)
    got = vops.yuv420_to_clip(torch.from_numpy(buf).to(device), [0, 0, 0], 2, W, H, stride, pl,
                              16, 12, crop=boxes, dtype=torch.float32, matrix=matrix, filter=filt,
                              sampling=sampling).cpu().numpy()
    assert got.shape == (3, 2, 12, 16, 4)
    for k in range(3):
        ref, _, d, tol = occ.tolerance(y, u, v, 16, 12, exact[k], matrix, sampling, filt)
        err = float(np.abs(got[k][..., :3].astype(np.float64) - ref).max())
        print("%s %s view %d: d = %.3g tol = %.3g err = %.3g" % (name, filt, k, d, tol, err))
        assert d > 0 and tol <= orc.TOL_CEILING
        assert err <= tol, (name, filt, k, err, tol)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


@pytest.mark.parametrize("filt", vops.FILTERS)
@pytest.mark.parametrize("name", [c[0] for c in ORACLE_CASES])
def test_mirror_views_against_the_oracle(name, filt):
    check_views_against_oracle(name, filt, CPU)


# -- 3. n boxes == n single-box calls -------------------------------------------------------------------
def boxed_case(matrix="bt601", sampling="420", header=6, clips=3, F=3):
    """A buffer of ``clips`` clips of 46 x 34 behind ``header`` bytes per frame,
    rows in a repeated, non-monotonic order, each with a box of its own."""
    y, u, v = occ.noise_planes(46, 34, clips * F, 91 + header, matrix, sampling)
    buf, stride, pl = occ.pack_planar(y, u, v, header)
    span = F * stride
    vb = view_boxes(46, 34, 16, 12, 13.7, 3)
    rows = [(2, 0), (0, 2), (2, 1), (1, 1), (0, 0), (2, 2), (0, 1)][:2 * clips + 1]
    offsets = [c * span for c, _ in rows]
    boxes = [vb[k] for _, k in rows[:-1]] + [(-2.5, 1.0, 50.0, 30.5)]     # one leaves the frame
    return buf, stride, pl, offsets, boxes, F


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("filt", vops.FILTERS)
def test_n_boxes_equal_n_single_box_calls(filt, dtype):
    buf, stride, pl, offsets, boxes, F = boxed_case()
    if filt == "antialias":
        boxes = boxes[:-1] + [(3.5, 1.25, 40.0, 30.0)]
    t = torch.from_numpy(buf)
    got = vops.yuv420_to_clip(t, offsets, F, 46, 34, stride, pl, 16, 12, crop=boxes, dtype=dtype,
                              filter=filt)
    want = torch.cat([vops.yuv420_to_clip(t, [o], F, 46, 34, stride, pl, 16, 12, crop=b,
                                          dtype=dtype, filter=filt)
                      for o, b in zip(offsets, boxes)])
    assert got.shape == want.shape == (len(offsets), F, 12, 16, 4 if dtype == torch.float32 else 8)
    assert torch.equal(got, want)
    out = torch.empty_like(got)
    assert vops.yuv420_to_clip(t, offsets, F, 46, 34, stride, pl, 16, 12, crop=boxes, dtype=dtype,
                               filter=filt, out=out) is out and torch.equal(out, want)
    # one box, given as a tuple, a list or a tensor, is today's call
    one = vops.yuv420_to_clip(t, offsets, F, 46, 34, stride, pl, 16, 12, crop=boxes[0], dtype=dtype,
                              filter=filt)
    for form in (list(boxes[0]), torch.tensor(boxes[0], dtype=torch.float64)):
        assert torch.equal(one, vops.yuv420_to_clip(t, offsets, F, 46, 34, stride, pl, 16, 12,
                                                    crop=form, dtype=dtype, filter=filt))


# -- 4. decoders ---------------------------------------------------------------------------------------
def make_files(tmp_path, W=46, H=34, frames=9):
    ypath, _ = write_y4m_file(tmp_path, W, H, frames, 21)
    mpath = str(tmp_path / "v.mjpeg")
    mjpeg.write_mjpeg(mpath, chroma_frames(W, H, frames, 22, "420"), quality=90, restart_interval=2)
    return ypath, mpath


DECODERS = [("y4m", Y4mDecoder, {}), ("mjpeg_host", MjpegDecoder, {}),
            ("mjpeg_gpu", MjpegDecoder, {"entropy": "gpu", "subseq_bytes": 0}),
            ("mjpeg_subseq", MjpegDecoder, {"entropy": "gpu", "subseq_bytes": 48})]
VIEW_CROP = {"short_side": 13.7, "views": 3}


def make_decoder(kind, device, filt="antialias", F=2, dtype=torch.float32):
    _, cls, args = next(d for d in DECODERS if d[0] == kind)
    return cls(device, clip_length=F, height=12, width=16, dtype=dtype, crop=dict(VIEW_CROP),
               filter=filt, **args)


@pytest.mark.parametrize("kind", [d[0] for d in DECODERS])
def test_decode_rows_and_the_row_indexed_form(tmp_path, kind):
    ypath, mpath = make_files(tmp_path)
    path = ypath if kind == "y4m" else mpath
    dec = make_decoder(kind, CPU)
    assert dec.views == 3
    vid, n = dec.probe(path)
    assert n == 9
    full = dec.decode(vid, [5, 0])
    assert full.shape == (6, 2, 12, 16, 4)
    assert dec.decode(vid, []).shape == (0, 2, 12, 16, 4)
    # clip-major, the views of a clip adjacent: each row is the one-view decode of its box
    boxes = view_boxes(46, 34, 16, 12, 13.7, 3)
    rows = [(5, 0), (5, 1), (5, 2), (0, 0), (0, 1), (0, 2)]
    assert torch.equal(full, dec.decode(vid, [s for s, _ in rows], views=[v for _, v in rows]))
    pick = [4, 1, 3, 1]                                     # any rows, any order, repeats
    got = dec.decode(vid, [rows[r][0] for r in pick], views=[rows[r][1] for r in pick])
    assert torch.equal(got, full[pick])
    slot = torch.full((8, 2, 12, 16, 4), 7.0)
    assert dec.decode(vid, [5, 0], out=slot[:6]).data_ptr() == slot.data_ptr()
    assert torch.equal(slot[:6], full) and torch.all(slot[6:] == 7.0)
    if kind == "y4m":      # against the op, one box at a time
        _, data = dec._map(vid, path)
        hdr = dec._videos[vid][1]
        for r, (s, k) in enumerate(rows):
            a = hdr.frame_offset(s)
            one = vops.yuv420_to_clip(torch.from_numpy(data[a:a + 2 * hdr.frame_stride].copy()), [0],
                                      2, 46, 34, hdr.frame_stride, vops.i420_planes(46, 34, 6), 16,
                                      12, crop=boxes[k], filter="antialias")
            assert torch.equal(full[r], one[0])


@pytest.mark.parametrize("kind", [d[0] for d in DECODERS])
def test_a_request_stages_each_clip_once_and_launches_once(tmp_path, monkeypatch, kind):
    ypath, mpath = make_files(tmp_path)
    dec = make_decoder(kind, CPU, F=2)
    vid, _ = dec.probe(ypath if kind == "y4m" else mpath)
    calls = {"clip": [], "idct": []}
    real_clip, real_idct = vops.yuv420_to_clip, vops.jpeg_idct

    def clip(buf, offsets, *a, **kw):
        calls["clip"].append((int(buf.numel()), list(offsets), kw.get("crop")))
        return real_clip(buf, offsets, *a, **kw)

    def idct(records, nframes, *a, **kw):
        calls["idct"].append(int(nframes))
        return real_idct(records, nframes, *a, **kw)
    monkeypatch.setattr(dmod.vops, "yuv420_to_clip", clip)
    monkeypatch.setattr(dmod.vops, "jpeg_idct", idct)
    dec.decode(vid, [5, 0])
    assert len(calls["clip"]) == 1
    numel, offsets, crop = calls["clip"][0]
    assert len(offsets) == 6 and len(set(offsets)) == 2 and offsets[0] == offsets[1] == offsets[2]
    span = max(offsets) - min(offsets)
    assert span > 0 and numel == 2 * span                    # a buffer of 2 spans
    assert len(crop) == 6 and crop[:3] == crop[3:] and len(set(crop)) == 3
    assert calls["idct"] == ([] if kind == "y4m" else [2 * 2])
    if kind != "y4m":
        assert dec.stats["requests"] == 1


# -- 5. loader --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loader_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("views_loader")
    return write_y4m_file(d, 64, 48, 48, 31, name="l.y4m")[0]


def make_loader(max_clips, device=CPU, clips=5, **kw):
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    return R2P1DLoader(device, decoder="y4m", num_clips_population=[clips], num_clips_weights=[1],
                       seed=0, dtype="fp32", warmup=0, max_clips=max_clips,
                       crop={"short_side": 112, "views": 3}, **kw)


@pytest.mark.parametrize("max_clips,rows", [(3, 3), (4, 3), (45, 15)])
def test_loader_row_counts(loader_file, max_clips, rows):
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    from rnb_amd.timecard import TimeCard
    loader = make_loader(max_clips)
    assert loader.views == 3 and loader.decoder.views == 3
    assert R2P1DLoader.output_shape_for(max_clips=max_clips, dtype="fp32")[0][0] == max_clips
    tc = TimeCard(13)
    (frames,), _, tc = loader((None,), loader_file, tc)
    assert frames.shape == (rows, 8, 112, 112, 4) and tc.num_clips == rows
    vid, starts = tc.extra["clip_src"]
    assert len(starts) == rows and starts[0::3] == starts[1::3] == starts[2::3]
    assert len(set(starts)) == rows // 3
    want = loader.decoder.decode(vid, starts[0::3])
    assert torch.equal(frames, want)
    assert not torch.equal(frames[0], frames[1]) and not torch.equal(frames[1], frames[2])


@pytest.mark.parametrize("segments", [2, 3])
def test_segments_concatenated_equal_the_one_piece_decode(loader_file, segments):
    from rnb_amd.control import segment_bounds
    from rnb_amd.timecard import TimeCard
    loader = make_loader(45, clips=2)
    tc = TimeCard(13)
    outs = [(torch.full((6, 8, 112, 112, 4), 9.0),) for _ in range(segments)]
    rows, _, tc = loader.call_into_segments((None,), loader_file, tc, outs)
    assert sum(rows) == 6 == tc.num_clips
    assert rows == [b - a for a, b in (segment_bounds(6, segments, k) for k in range(segments))]
    vid, starts = tc.extra["clip_src"]
    whole = loader.decoder.decode(vid, starts[0::3])
    assert torch.equal(torch.cat([o[0][:r] for o, r in zip(outs, rows)]), whole)
    assert all(torch.all(o[0][r:] == 9.0) for o, r in zip(outs, rows))


def test_decoders_without_views_have_one(tmp_path):
    from rnb_amd.models.r2p1d.decoder import Decoder, NpyDecoder, SyntheticDecoder
    assert Decoder.views == 1 and SyntheticDecoder(CPU).views == 1 and NpyDecoder(CPU).views == 1
    assert Y4mDecoder(CPU).views == 1 and MjpegDecoder(CPU, crop="center").views == 1
    assert Y4mDecoder(CPU, crop={"short_side": 128}).views == 1


def test_shipped_configs(tmp_path):
    import json
    import os
    from rnb_amd.config import load_pipeline
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for backend in ("y4m", "mjpeg"):
        path = os.path.join(root, "configs", "r2p1d-whole-%s-3crop.json" % backend)
        d = json.load(open(path))["defaults"]
        assert d["crop"] == {"short_side": 128, "views": 3} and d["filter"] == "antialias"
        assert d["max_clips"] == 45
        spec = load_pipeline(path)
        assert spec.steps[0].kwargs["decoder"] == backend
        assert all(s.kwargs["max_clips"] == 45 for s in spec.steps)
