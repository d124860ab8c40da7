"""4:2:2 and 4:4:4 chroma through the file-backed decode path, on the CPU: the
clip mirrors against the fp64 oracle (decode_oracle_chroma.py), the host MJPEG
decoders (librnb_jpeg.so, the numpy reference, the interval and subsequence
mirrors) on ``write_mjpeg(sampling=)`` streams and on four PIL-written golden
streams, ``MjpegDecoder`` against PIL's RGB, Y4M ``C422`` / ``C444`` headers and
``Y4mDecoder``, the refusals, and the byte identity of the 4:2:0 entry points.
The helpers here also serve tests/test_gpu_chroma.py.
"""
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_oracle as orc  # noqa: E402
import decode_oracle_chroma as occ  # noqa: E402
from rnb_amd.models.r2p1d.decoder import MjpegDecoder, Y4mDecoder  # noqa: E402
from rnb_amd.ops import native, video as vops  # noqa: E402
from rnb_amd.utils import mjpeg, y4m  # noqa: E402
from test_mjpeg_cpu import GOLDEN, GOLDEN_STREAMS, check_band, frame_bytes, lib, pil_rgb  # noqa: E402

CPU = torch.device("cpu")
SAMPLINGS = ("422", "444")
SUBSEQ = (48, 64)
# name -> (W, H, sampling, PIL save options, kind); two frames each. Sizes that are no
# multiple of 16 or 8: padding blocks right and below, ceil chroma sizes, and (7 x 9 at
# 4:4:4) a frame one MCU wide and two high.
GOLDEN_CHROMA = {
    "noise_q90_422_rows": (52, 37, "422", dict(quality=90, subsampling=1, restart_marker_rows=1),
                           "noise"),
    "noise_q75_422_opt": (52, 37, "422", dict(quality=75, subsampling=1, optimize=True), "noise"),
    "noise_q95_444_blocks": (37, 26, "444", dict(quality=95, subsampling=0,
                                                 restart_marker_blocks=3), "noise"),
    "ramp_q30_444": (7, 9, "444", dict(quality=30, subsampling=0), "ramp"),
}
# |fp64 clip oracle at identity scale on decode_reference's rounded planes - PIL's RGB|,
# per golden the maximum over its two frames of (max, mean) in 8-bit levels, measured on
# the CPU with PIL 12.2 (libjpeg-turbo's integer IDCT, h2v1 "fancy" upsampling for 4:2:2,
# none for 4:4:4, and its colour conversion); see profiles/chroma_formats.txt
# (measured: 2.515 / 0.4257, 2.703 / 0.4273, 2.264 / 0.2856, 1.420 / 0.2662; rounded up)
PIL_ORACLE = {
    "noise_q90_422_rows": (2.52, 0.43),
    "noise_q75_422_opt": (2.71, 0.43),
    "noise_q95_444_blocks": (2.27, 0.29),
    "ramp_q30_444": (1.43, 0.27),
}
# test_decode_oracle_cpu.py's rule and constants for the decoder against PIL
PIL_MAX_SLACK = 2.8
PIL_MEAN_FACTOR = 1.25
# name -> (W, H, restart interval, sampling, quality) of the write_mjpeg streams
WRITTEN = {
    "w422_r0": (52, 37, 0, "422", 75),          # one interval: the subsequence path
    "w422_r3": (52, 37, 3, "422", 95),          # 4 x 5 MCUs, intervals that wrap rows
    "w444_r0": (37, 26, 0, "444", 75),
    "w444_r2": (37, 26, 2, "444", 95),          # 5 x 4 MCUs
    "w444_7x9": (7, 9, 0, "444", 50),           # one MCU wide, two high
    "w422_7x9": (7, 9, 1, "422", 50),           # one MCU wide, two high, an interval each
}


# -- inputs ------------------------------------------------------------------------------------
def chroma_frames(W, H, frames, seed, sampling):
    """Random frames: [(Y [H, W], U, V [ceil(H/Vs), ceil(W/Hs)])]."""
    rng = np.random.default_rng(seed)
    cw, ch = mjpeg.chroma_size(W, H, sampling)
    return [(rng.integers(0, 256, (H, W), dtype=np.uint8),
             rng.integers(0, 256, (ch, cw), dtype=np.uint8),
             rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(frames)]


def build_written(d):
    """name -> (path, truth) of the WRITTEN streams in directory ``d``."""
    out = {}
    for name, (W, H, restart, sampling, quality) in WRITTEN.items():
        path = os.path.join(str(d), name + ".mjpeg")
        truth = mjpeg.write_mjpeg(path, chroma_frames(W, H, 2, W + H + restart, sampling),
                                  quality=quality, restart_interval=restart, sampling=sampling)
        out[name] = (path, truth)
    for name in GOLDEN_CHROMA:
        out[name] = (os.path.join(GOLDEN, name + ".mjpeg"), None)
    return out


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    return build_written(tmp_path_factory.mktemp("chroma"))


def host_records(data, idx):
    """Flat records of every frame from the host entropy decoder."""
    out = np.zeros(idx.num_frames * idx.record_bytes, dtype=np.uint8)
    mjpeg.entropy_decode(data, idx.offsets, idx.lengths, out, idx.record_bytes, 1,
                         sampling=idx.sampling)
    return out


def packed(data, idx, sel=None):
    """(scan records, offsets) of the frames ``sel`` (default: all)."""
    offs = idx.offsets if sel is None else idx.offsets[sel]
    lens = idx.lengths if sel is None else idx.lengths[sel]
    buf = np.zeros(sum(mjpeg.scan_record_bound(idx.mw, idx.mh, n) for n in lens), dtype=np.uint8)
    n, scan_offs = mjpeg.pack_scans(data, offs, lens, buf, name="<test>", sampling=idx.sampling)
    assert n == scan_offs[-1] and n <= buf.size and (scan_offs % 16 == 0).all()
    return buf[:n].copy(), scan_offs


def stream_case(streams, name):
    """(idx, serial host records, scan records, offsets) of a stream."""
    path, _ = streams[name]
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    scans, offs = packed(data, idx)
    return idx, host_records(data, idx), scans, offs


def damaged_records(streams, name):
    """(idx, clean scan record of frame 0, {case: damaged copy}) of a stream: the
    fixed list the host mirrors, the stand-alone programs' kin and then the GPU
    kernels are given. Truncated spans, flipped scan bytes, broken tables and
    header words, and every wrong value of the sampling word. These are the
    decoders' ordinary error returns."""
    idx, _, scans, offs = stream_case(streams, name)
    clean = scans[:int(offs[1])].copy()
    n_int = int(clean[2016:2020].view(np.uint32)[0])
    scan_len = int(clean[2024:2028].view(np.uint32)[0])
    body = 2032 + 8 * n_int
    spans = clean[2032:body].view(np.uint32).reshape(n_int, 2)
    end = int(spans[-1, 1])
    word = mjpeg.SAMPLINGS.index(idx.sampling)
    assert int(clean[2028:2032].view(np.uint32)[0]) == word
    out = {}

    def case(cname, at, value=None, xor=None, u32=None):
        bad = clean.copy()
        if u32 is not None:
            bad[at:at + 4].view(np.uint32)[0] = u32
        else:
            bad[at] = value if value is not None else bad[at] ^ xor
        assert not np.array_equal(bad, clean), cname
        out[cname] = bad
    for at, xor in ((1, 0x01), (17, 0x80), (scan_len // 3, 0x55), (scan_len // 2, 0x3C),
                    (scan_len - 20, 0xAA), (scan_len - 2, 0x11)):
        case("flip_%04d" % at, body + at, xor=xor)
    for cut in (1, 7, 60):
        case("end_minus_%d" % cut, body - 4, u32=end - cut)
    case("span0_begin_past_end", 2032, u32=int(spans[0, 1]) + 1)
    case("last_span_past_scan_len", body - 4, u32=scan_len + 1)
    case("y_ac_count_raised", 384 + 272 + 15, value=int(clean[384 + 272 + 15]) + 40)
    case("one_interval_more", 2016, u32=n_int + 1)
    case("scan_len_huge", 2024, u32=0x7FFFFFF0)
    for other in (0, 1, 2, 3, 0xFFFFFFFF):
        if other != word:
            case("sampling_word_%x" % other, 2028, u32=other)
    return idx, clean, out


def decode_one(rec, idx, S=0):
    offs = np.array([0, rec.size], dtype=np.int64)
    return mjpeg.decode_scans_host(rec, offs, 1, idx.mw, idx.mh, subseq_bytes=S,
                                   sampling=idx.sampling)


# -- golden streams ------------------------------------------------------------------------------
def pil_chroma_stream(W, H, options, kind, seed):
    """Bytes of two PIL-written frames."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    data = b""
    for f in range(2):
        if kind == "ramp":
            yy, xx = np.mgrid[0:H, 0:W]
            rgb = np.stack([(xx * 23 + yy * 5 + 9 * f) % 256, (yy * 19 + 40 * f) % 256,
                            (xx * 11 + yy * 13) % 256], axis=-1).astype(np.uint8)
        else:
            rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        fp = io.BytesIO()
        Image.fromarray(rgb).save(fp, "JPEG", **options)
        data += fp.getvalue()
    return data


def write_golden():
    """The GOLDEN_CHROMA streams as PIL writes them here, with PIL's own RGB of
    every frame; a stream that is already there is kept."""
    for name, (W, H, sampling, options, kind) in GOLDEN_CHROMA.items():
        path = os.path.join(GOLDEN, name + ".mjpeg")
        if not os.path.exists(path):
            open(path, "wb").write(pil_chroma_stream(W, H, options, kind, seed=len(name)))
        assert mjpeg.read_index(path).sampling == sampling
        rgb = pil_rgb(path)
        assert rgb.shape == (2, H, W, 3) and rgb.dtype == np.uint8
        np.save(os.path.join(GOLDEN, name + "_rgb.npy"), rgb)
        print(name, os.path.getsize(path), "bytes")


@functools.lru_cache(maxsize=None)
def pil_oracle(name):
    """(PIL's RGB [2, H, W, 3], per-frame (max, mean) of |oracle - PIL|): the
    fp64 oracle at native size on decode_reference's rounded planes."""
    W, H, sampling = GOLDEN_CHROMA[name][:3]
    path = os.path.join(GOLDEN, name + ".mjpeg")
    want = np.load(os.path.join(GOLDEN, name + "_rgb.npy"))
    assert want.shape == (2, H, W, 3) and want.dtype == np.uint8
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    cw, ch = mjpeg.chroma_size(W, H, sampling)
    stats = []
    for i in range(2):
        py, pu, pv = mjpeg.decode_reference(frame_bytes(data, idx, i))["planes_u8"]
        _, rgb = occ.clip_oracle(np.asarray(py)[None, :H, :W], np.asarray(pu)[None, :ch, :cw],
                                 np.asarray(pv)[None, :ch, :cw], W, H, None, "jfif", sampling)
        diff = np.abs(np.clip(rgb[0], 0, 255) - want[i])
        stats.append((float(diff.max()), float(diff.mean())))
    want.setflags(write=False)
    return want, tuple(stats)


def check_pil_rgb(name, device, **decoder_args):
    """``MjpegDecoder`` at identity scale against PIL's RGB, bounded from the
    oracle's own distance as test_decode_oracle_cpu.py does."""
    W, H, sampling = GOLDEN_CHROMA[name][:3]
    want, stats = pil_oracle(name)
    # the oracle is still what was measured: the bounds grow with these figures, so a
    # wrong oracle must not pass as a generous one
    assert max(s[0] for s in stats) <= PIL_ORACLE[name][0] and \
        max(s[1] for s in stats) <= PIL_ORACLE[name][1], (name, stats)
    dec = MjpegDecoder(device, clip_length=2, height=H, width=W, dtype=torch.float32,
                       crop="full", **decoder_args)
    vid, n = dec.probe(os.path.join(GOLDEN, name + ".mjpeg"))
    assert n == 2
    got = dec.decode(vid, [0])
    dec.drain()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    assert tuple(got.shape) == (1, 2, H, W, 4)
    rgb = orc.denormalise(got.detach().cpu().numpy()[0])
    for i, (omax, omean) in enumerate(stats):
        diff = np.abs(rgb[i] - want[i])
        print("%s frame %d on %s %s: |oracle - PIL| max %.3f mean %.4f; |decoder - PIL| max %.3f "
              "mean %.4f" % (name, i, device.type, decoder_args, omax, omean, diff.max(),
                             diff.mean()))
        assert diff.max() <= omax + PIL_MAX_SLACK, (name, i, diff.max(), omax)
        assert diff.mean() <= PIL_MEAN_FACTOR * omean, (name, i, diff.mean(), omean)


# -- clip cases ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip_reference(sampling, name):
    """(planes, ref64, d, tol) of a case of decode_oracle_chroma.cases: computed
    once, shared and left unchanged."""
    _, matrix, filt, w, h, ow, oh, crop, frames = next(c for c in occ.cases(sampling)
                                                       if c[0] == name)
    y, u, v = occ.noise_planes(w, h, frames, occ.case_seed(name, sampling), matrix, sampling)
    ref, rgb, d, tol = occ.tolerance(y, u, v, ow, oh, crop, matrix, sampling, filt)
    assert tol <= orc.TOL_CEILING, (sampling, name, tol)
    for a in (y, u, v, ref):
        a.setflags(write=False)
    return (y, u, v), ref, d, tol


def run_clip(sampling, name, device, dtype, clips=1, surface=False):
    """The op on a case's planes: an unaligned planar buffer (header 7), or the
    padded ``jpeg_idct`` surface layout for a JFIF case with ``surface``."""
    _, matrix, filt, w, h, ow, oh, crop, frames = next(c for c in occ.cases(sampling)
                                                       if c[0] == name)
    (y, u, v), _, _, _ = clip_reference(sampling, name)
    if surface:
        mw, mh, _ = mjpeg.geometry(w, h, sampling)
        buf, stride, pl = occ.pack_jpeg_surface(y, u, v, mw, mh, sampling, 0x5A)
        assert pl == vops.jpeg_surface_planes(mw, mh, sampling)
    else:
        buf, stride, pl = occ.pack_planar(y, u, v)
        if matrix == "bt601":
            maker = vops.i422_planes if sampling == "422" else vops.i444_planes
            assert pl == maker(w, h, 7), (pl, maker(w, h, 7))
    t = torch.from_numpy(np.tile(buf, clips)).to(device)
    offs = [c * frames * stride for c in range(clips)]
    return vops.yuv420_to_clip(t, offs, frames, w, h, stride, pl, ow, oh, crop=crop, dtype=dtype,
                               matrix=matrix, filter=filt, sampling=sampling)


def bf16_of(x32):
    """RNE(fp32) -> bf16 bits, as the kernels round."""
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).to(torch.int32)


def check_clip_case(sampling, name, device, clips=1, surface=False):
    _, ref, d, tol = clip_reference(sampling, name)
    got = run_clip(sampling, name, device, torch.float32, clips, surface)
    g = got.detach().cpu()
    assert g.shape[-1] == 4 and not g[..., 3].any()
    err = max(float(np.abs(g[c].numpy()[..., :3].astype(np.float64) - ref).max())
              for c in range(clips))
    print("%s %s on %s: oracle fp32-vs-fp64 %.3e, tol %.3e, |got - oracle| %.3e"
          % (sampling, name, device.type, d, tol, err))
    assert err <= tol, (sampling, name, err, tol)
    b = run_clip(sampling, name, device, torch.bfloat16, clips, surface).detach().cpu()
    assert b.shape[-1] == 8 and not b[..., 3:].float().any()
    assert torch.equal(b[..., :3].contiguous().view(torch.int16).to(torch.int32) & 0xFFFF,
                       bf16_of(g[..., :3]))


# == the tests =====================================================================================
@pytest.mark.parametrize("name", [c[0] for c in occ.cases("422")])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_clip_mirror_against_oracle(sampling, name):
    check_clip_case(sampling, name, CPU, surface=name == "jfif_bil_45x33")


@pytest.mark.parametrize("matrix", ["bt601", "jfif"])
@pytest.mark.parametrize("filt", ["bilinear", "antialias"])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_chroma_ramp_pins_the_siting_per_axis(sampling, filt, matrix):
    """4:2:2: the vertical chroma coordinate is luma's, the horizontal one half
    luma's plus the centre offset; 4:4:4: both are luma's. From the mapping
    alone, no resampling code (an upscale, so both filters are two taps)."""
    y, u, v = occ.chroma_ramp_planes(sampling)
    buf, stride, pl = occ.pack_planar(y, u, v)
    for ow, oh, crop in ((96, 64, None), (60, 40, (4, 4, 30, 20))):
        got = vops.yuv420_to_clip(torch.from_numpy(buf), [0], 2, occ.RAMP_W, occ.RAMP_H, stride,
                                  pl, ow, oh, crop=crop, matrix=matrix, filter=filt,
                                  sampling=sampling).numpy()[0]
        exp, bmask, rmask = occ.chroma_ramp_expectation(ow, oh, crop, matrix, sampling)
        assert bmask.mean() > 0.5 and rmask.mean() > 0.5
        for f in range(2):
            assert np.abs(got[f][..., 2] - exp[..., 2])[bmask].max() <= 2e-5
            assert np.abs(got[f][..., 0] - exp[..., 0])[rmask].max() <= 2e-5
    if sampling == "422":
        # and it is NOT the 4:2:0 mapping: read as 4:2:0 rows the same planes differ
        hs_only = occ.chroma_ramp_expectation(96, 64, None, matrix, "420")[0]
        exp = occ.chroma_ramp_expectation(96, 64, None, matrix, "422")[0]
        assert np.abs(hs_only[..., 0] - exp[..., 0]).max() > 1e-2


def test_bad_sampling_raises_naming_the_argument(tmp_path):
    buf = torch.zeros(64, dtype=torch.uint8)
    for call in (lambda: vops.yuv420_to_clip(buf, [0], 1, 4, 4, 48, vops.i444_planes(4, 4), 2, 2,
                                             sampling="440"),
                 lambda: vops.jpeg_surface_planes(1, 1, sampling="411"),
                 lambda: vops.jpeg_idct(buf, 1, 1, 1, sampling=422),
                 lambda: vops.jpeg_huff(buf, [0, 0], 1, 1, 1, sampling="4:2:2"),
                 lambda: mjpeg.write_mjpeg(str(tmp_path / "x"), chroma_frames(8, 8, 1, 0, "444"),
                                           sampling="440"),
                 lambda: mjpeg.geometry(8, 8, "mono"),
                 lambda: y4m.write_y4m(str(tmp_path / "y"), chroma_frames(8, 8, 1, 0, "444"),
                                       sampling="440")):
        with pytest.raises(ValueError, match="sampling"):
            call()
    # BT.601: an even size only along a subsampled axis
    y, u, v = occ.noise_planes(46, 33, 1, 0, "bt601", "422")
    b, stride, pl = occ.pack_planar(y, u, v)
    vops.yuv420_to_clip(torch.from_numpy(b), [0], 1, 46, 33, stride, pl, 4, 4, sampling="422")
    with pytest.raises(ValueError, match="even"):
        vops.yuv420_to_clip(torch.from_numpy(b), [0], 1, 45, 33, stride, pl, 4, 4, sampling="422")


def test_geometry_and_layouts():
    assert mjpeg.geometry(52, 37, "422") == (4, 5, 384 + 128 * 4 * 20)
    assert mjpeg.geometry(37, 26, "444") == (5, 4, 384 + 128 * 3 * 20)
    assert mjpeg.geometry(7, 9, "444") == (1, 2, 384 + 128 * 3 * 2)
    assert mjpeg.geometry(7, 9, "422") == (1, 2, 384 + 128 * 4 * 2)
    assert mjpeg.geometry(46, 34) == mjpeg.geometry(46, 34, "420") == (3, 3, 384 + 768 * 9)
    assert vops.jpeg_surface_planes(3, 2) == vops.jpeg_surface_planes(3, 2, "420") == \
        vops.YuvPlanes(0, 256 * 6, 320 * 6, 48, 24, 24, 1)
    assert vops.jpeg_surface_planes(3, 2, "422") == vops.YuvPlanes(0, 128 * 6, 192 * 6, 48, 24, 24, 1)
    assert vops.jpeg_surface_planes(3, 2, "444") == vops.YuvPlanes(0, 64 * 6, 128 * 6, 24, 24, 24, 1)
    assert vops.jpeg_frame_bytes(3, 2, "422") == (384 + 512 * 6, 256 * 6)
    assert vops.i422_planes(46, 33, 7) == vops.YuvPlanes(7, 7 + 46 * 33, 7 + 46 * 33 + 23 * 33,
                                                         46, 23, 23, 1)
    assert vops.i444_planes(45, 33, 6) == vops.YuvPlanes(6, 6 + 45 * 33, 6 + 2 * 45 * 33,
                                                         45, 45, 45, 1)


# -- MJPEG: entropy decoders ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WRITTEN) + sorted(GOLDEN_CHROMA))
def test_host_decoders_agree_on_every_stream(written, name):
    """decode_reference gives the encoder's coefficients; librnb_jpeg.so's
    records equal decode_reference's byte for byte; pack_scans ->
    decode_scans_host equals them with and without subseq_bytes."""
    lib()
    path, truth = written[name]
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    W, H, sampling = (WRITTEN[name][0], WRITTEN[name][1], WRITTEN[name][3]) if truth else \
        GOLDEN_CHROMA[name][:3]
    assert (idx.width, idx.height, idx.sampling, idx.num_frames) == (W, H, sampling, 2)
    assert (idx.mw, idx.mh, idx.record_bytes) == mjpeg.geometry(W, H, sampling)
    want = host_records(data, idx)
    for i in range(2):
        ref = mjpeg.decode_reference(frame_bytes(data, idx, i), planes=False)
        assert ref["sampling"] == sampling
        if truth:
            assert np.array_equal(ref["coefs"], truth[i][0]) and \
                np.array_equal(ref["qt"], truth[i][1])
        rec = mjpeg.pack_record(ref["coefs"], ref["qt"])
        assert rec.size == idx.record_bytes
        assert np.array_equal(want[i * rec.size:(i + 1) * rec.size], rec), (name, i)
    scans, offs = packed(data, idx)
    word = mjpeg.SAMPLINGS.index(sampling)
    for i in range(2):
        assert int(scans[int(offs[i]) + 2028:int(offs[i]) + 2032].view(np.uint32)[0]) == word
    got, status = mjpeg.decode_scans_host(scans, offs, 2, idx.mw, idx.mh, sampling=sampling)
    assert status.tolist() == [0, 0] and np.array_equal(got, want)
    total_rounds = 0
    for S in SUBSEQ:
        out = np.full(want.size + 16, 0x5A, dtype=np.uint8)
        _, status, rounds = mjpeg.decode_scans_host(scans, offs, 2, idx.mw, idx.mh, out=out,
                                                    subseq_bytes=S, return_rounds=True,
                                                    sampling=sampling)
        assert status.tolist() == [0, 0], (name, S)
        assert np.array_equal(out[:want.size], want) and (out[want.size:] == 0x5A).all(), (name, S)
        total_rounds += int(rounds.sum())
    if name in ("w422_r0", "w444_r0", "noise_q75_422_opt"):
        # one interval of dozens of subsequences: the subsequence path ran
        n_int = int(scans[2016:2020].view(np.uint32)[0])
        span = scans[2032:2040].view(np.uint32)
        assert n_int == 1 and (int(span[1]) - int(span[0])) // 48 >= 24 and total_rounds > 0
    # the CPU op is the same mirror
    rec, status = vops.jpeg_huff(torch.from_numpy(scans), offs, 2, idx.mw, idx.mh,
                                 subseq_bytes=48, sampling=sampling)
    assert np.array_equal(rec.numpy(), want) and status.tolist() == [0, 0]


def test_entropy_decode_without_the_library(written, monkeypatch):
    """The numpy fallback of read_index / entropy_decode gives the same index and
    records."""
    for name in ("w422_r3", "ramp_q30_444"):
        path, _ = written[name]
        data = np.fromfile(path, dtype=np.uint8)
        idx = mjpeg.read_index(path)
        want = host_records(data, idx)
        with monkeypatch.context() as m:
            m.setattr(mjpeg, "_native", lambda: None)
            idx2 = mjpeg.read_index(path)
            assert idx2[:6] == idx[:6] and idx2.sampling == idx.sampling
            assert np.array_equal(idx2.offsets, idx.offsets)
            assert np.array_equal(host_records(data, idx2), want)


@pytest.mark.parametrize("name", ["w422_r0", "w422_r3", "w444_r0", "w444_r2"])
def test_damaged_records_equal_the_serial_decoder(written, name):
    lib()
    idx, clean, cases = damaged_records(written, name)
    refused = 0
    for cname, bad in [("clean", clean)] + sorted(cases.items()):
        want, ws = decode_one(bad, idx)
        refused += int(ws[0] < 0)
        if cname.startswith("sampling_word"):
            assert mjpeg.status_field(int(ws[0])) == "scan record" and not want[384:].any()
        for S in SUBSEQ:
            got, gs = decode_one(bad, idx, S)
            assert gs[0] == ws[0], (name, cname, S, int(gs[0]), int(ws[0]))
            assert np.array_equal(got, want), (name, cname, S)
        print(name, cname, int(ws[0]), mjpeg.status_field(int(ws[0])) if ws[0] else "ok")
    assert refused >= 8
    # a record of this sampling given to another geometry is refused as a whole, too
    for other in mjpeg.SAMPLINGS:
        if other != idx.sampling:
            mw, mh, _ = mjpeg.geometry(idx.width, idx.height, other)
            _, st = mjpeg.decode_scans_host(clean, np.array([0, clean.size]), 1, mw, mh,
                                            sampling=other)
            assert mjpeg.status_field(int(st[0])) == "scan record"


def test_truncated_and_corrupted_frames_same_decision_in_every_decoder():
    """Truncations and seeded single-byte corruptions of a 4:2:2 and a 4:4:4
    frame: wherever the packer accepts, the interval mirror gives the frame
    decoder's decision, and the subsequence emulation the interval mirror's
    status and record."""
    j = lib()
    for sampling, restart in (("422", 0), ("444", 0), ("422", 2)):
        W, H = (52, 37) if sampling == "422" else (37, 26)
        f = mjpeg.encode_frame(*chroma_frames(W, H, 1, 11, sampling)[0], mjpeg.quality_tables(60),
                               restart, sampling=sampling)[0]
        mw, mh, rb = mjpeg.geometry(W, H, sampling)
        word = mjpeg.SAMPLINGS.index(sampling)
        frames = [f[:len(f) * i // 32] for i in range(32)]
        rng = np.random.default_rng(4321)
        for i in range(200):
            bad = np.frombuffer(f, dtype=np.uint8).copy()
            bad[int(rng.integers(2, bad.size))] = int(rng.integers(0, 256))
            frames.append(bad.tobytes())
        accepted = 0
        for fb in frames:
            buf = np.frombuffer(fb, dtype=np.uint8)
            if buf.size == 0:
                continue
            rec = np.zeros(rb, dtype=np.uint8)
            rc = j.decode_frames_rc(buf, [0], [buf.size], rec, rb, sampling=word)
            out = np.zeros(mjpeg.scan_record_bound(mw, mh, buf.size), dtype=np.uint8)
            got, offs = j.pack_scans(buf, [0], [buf.size], out, sampling=word)
            if got < 0:
                assert rc < 0
                continue
            accepted += 1
            scans = out[:got]
            r0, s0 = mjpeg.decode_scans_host(scans, offs, 1, mw, mh, sampling=sampling)
            assert (s0[0] == 0) == (rc == 0), (sampling, rc, int(s0[0]))
            if rc == 0:
                assert np.array_equal(r0, rec)
            for S in SUBSEQ:
                r1, s1 = mjpeg.decode_scans_host(scans, offs, 1, mw, mh, subseq_bytes=S,
                                                 sampling=sampling)
                assert s1[0] == s0[0] and np.array_equal(r1, r0), (sampling, S)
        assert accepted >= 100


def test_mixed_stream_gives_sampling_change(tmp_path):
    j = lib()
    q = mjpeg.quality_tables(75)
    a = mjpeg.encode_frame(*chroma_frames(52, 37, 1, 1, "420")[0], q)[0]
    b = mjpeg.encode_frame(*chroma_frames(52, 37, 1, 2, "422")[0], q, sampling="422")[0]
    path = str(tmp_path / "mixed.mjpeg")
    open(path, "wb").write(a + b)
    assert j.error_name(-22) == "sampling change" and "sampling change" in mjpeg._REASONS
    buf = np.frombuffer(a + b, dtype=np.uint8)
    info = (ctypes.c_int * 5)()
    assert j.lib.rnb_mjpeg_index_s(buf.ctypes.data, buf.size, None, None, 0, info) == -22
    assert info[2] == 1
    for call in (mjpeg.read_index, MjpegDecoder(CPU).probe):
        with pytest.raises(ValueError, match=r"mixed\.mjpeg: frame 1 .*'sampling change'"):
            call(path)
    # frame by frame: the decoders refuse a frame of another sampling than the stream's
    rec = np.zeros(mjpeg.geometry(52, 37, "422")[2], dtype=np.uint8)
    offs, lens = [0, len(a)], [len(a), len(b)]
    assert j.decode_frames_rc(buf, offs, lens, np.zeros(2 * rec.size, dtype=np.uint8), rec.size,
                              sampling=1) == -22
    out = np.zeros(2 * mjpeg.scan_record_bound(4, 5, len(a)), dtype=np.uint8)
    assert j.pack_scans(buf, offs, lens, out, sampling=1) == (-22, 0)
    # the 4:2:0 entry points keep refusing 4:2:2 and 4:4:4 as 'sampling'
    b_only = np.frombuffer(b, dtype=np.uint8)
    assert j.index(b_only)[0] == "sampling"
    assert j.error_name(j.decode_frames_rc(b_only, [0], [len(b)], rec, rec.size)) == "sampling"
    assert j.error_name(j.pack_scans(b_only, [0], [len(b)], out)[0]) == "sampling"
    # other factors are refused everywhere, naming what was found
    for hv in (0x41, 0x12, 0x14):
        bad = bytearray(b)
        bad[bad.index(b"\xff\xc0") + 11] = hv
        p = str(tmp_path / ("s%02x.mjpeg" % hv))
        open(p, "wb").write(bytes(bad))
        with pytest.raises(ValueError, match="'sampling'"):
            mjpeg.read_index(p)


def test_index_refuses_a_header_whose_sampling_the_scan_contradicts(tmp_path, monkeypatch):
    """A luma sampling byte that announces another of the three layouts than the
    scan was written for: read_index decodes the first frame once and names
    'sampling'. A first frame that decodes under no layout still indexes (its
    refusal comes from decode, as before)."""
    lib()
    q = mjpeg.quality_tables(75)
    bytes_of = {"420": 0x22, "422": 0x21, "444": 0x11}
    for true in mjpeg.SAMPLINGS:
        f = mjpeg.encode_frame(*chroma_frames(52, 37, 1, 4, true)[0], q, sampling=true)[0]
        sof = f.index(b"\xff\xc0")
        for claimed in mjpeg.SAMPLINGS:
            data = bytearray(f)
            data[sof + 11] = bytes_of[claimed]
            p = str(tmp_path / ("%s_as_%s.mjpeg" % (true, claimed)))
            open(p, "wb").write(bytes(data))
            for native_lib in (True, False):
                with monkeypatch.context() as m:
                    if not native_lib:
                        m.setattr(mjpeg, "_native", lambda: None)
                    if claimed == true:
                        assert mjpeg.read_index(p).sampling == true
                    else:
                        with pytest.raises(ValueError, match="frame 0 .*'sampling'.*only as %s"
                                           % ":".join(true)):
                            mjpeg.read_index(p)
    # a scan byte damaged so that no layout decodes: the index is as before
    f = bytearray(mjpeg.encode_frame(*chroma_frames(52, 37, 1, 4, "422")[0], q, sampling="422")[0])
    rec = np.zeros(mjpeg.geometry(52, 37, "422")[2], dtype=np.uint8)
    for at in range(len(f) - 40, len(f) - 400, -1):
        bad = bytearray(f)
        bad[at] ^= 0x55
        if 0xFF in (bad[at], f[at]):
            continue
        buf = np.frombuffer(bytes(bad), dtype=np.uint8)
        if len(lib().index_s(buf)) == 6 and \
                lib().decode_frames_rc(buf, [0], [buf.size], rec, rec.size, sampling=1) < 0:
            p = str(tmp_path / "damaged.mjpeg")
            open(p, "wb").write(bytes(bad))
            assert mjpeg.read_index(p).sampling == "422"
            break
    else:
        raise AssertionError("no damaged byte makes the decode fail")


def test_420_entry_points_are_byte_identical():
    """The three 4:2:0 golden streams through the unchanged 4:2:0 entry points
    and through the generalised ones at sampling 0: the same frame records,
    scan records (whose fourth header word stays 0) and status words."""
    j = lib()
    L = j.lib
    for name, (W, H, _) in sorted(GOLDEN_STREAMS.items()):
        data = np.fromfile(os.path.join(GOLDEN, name + ".mjpeg"), dtype=np.uint8)
        old = j.index(data)
        new = j.index_s(data)
        assert new[5] == 0 and old[:3] == new[:3] and np.array_equal(old[3], new[3]) \
            and np.array_equal(old[4], new[4])
        offs, lens = old[3], old[4]
        n = offs.size
        mw, mh, rb = mjpeg.geometry(W, H)
        rec_old = np.zeros(n * rb, dtype=np.uint8)
        rec_new = np.full(n * rb, 0x5A, dtype=np.uint8)
        assert L.rnb_jpeg_decode_frames(data.ctypes.data, data.size, offs.ctypes.data,
                                        lens.ctypes.data, n, rec_old.ctypes.data, rb, 1) == 0
        assert L.rnb_jpeg_decode_frames_s(data.ctypes.data, data.size, offs.ctypes.data,
                                          lens.ctypes.data, n, rec_new.ctypes.data, rb, 1, 0) == 0
        assert np.array_equal(rec_old, rec_new)
        cap = sum(mjpeg.scan_record_bound(mw, mh, int(x)) for x in lens)
        s_old, s_new = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
        o_old, o_new = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        info = (ctypes.c_int * 3)()
        got_old = L.rnb_jpeg_pack_scans(data.ctypes.data, data.size, offs.ctypes.data,
                                        lens.ctypes.data, n, s_old.ctypes.data, cap,
                                        o_old.ctypes.data, 0, 0, info)
        got_new = L.rnb_jpeg_pack_scans_s(data.ctypes.data, data.size, offs.ctypes.data,
                                          lens.ctypes.data, n, s_new.ctypes.data, cap,
                                          o_new.ctypes.data, 0, 0, info, 0)
        assert got_old == got_new > 0 and np.array_equal(o_old, o_new)
        assert np.array_equal(s_old, s_new)
        for i in range(n):
            assert not s_old[int(o_old[i]) + 2028:int(o_old[i]) + 2032].any()
        for S in (0, 48):
            outs = []
            for suffix in ("", "_s"):
                out = np.zeros(n * rb, dtype=np.uint8)
                st = np.full(n, 7, dtype=np.int32)
                rounds = np.zeros(n, dtype=np.int32)
                args = [s_old.ctypes.data, got_old, o_old.ctypes.data, n, mw, mh, out.ctypes.data,
                        out.size, rb, st.ctypes.data]
                fn = "rnb_jpeg_decode_scans_subseq_host" if S else "rnb_jpeg_decode_scans_host"
                if S:
                    args += [S, rounds.ctypes.data]
                if suffix:
                    args.append(0)
                assert getattr(L, fn + suffix)(*args) == 0
                outs.append((out, st, rounds))
            for a, b in zip(outs[0], outs[1]):
                assert np.array_equal(a, b)
            assert np.array_equal(outs[0][0], rec_old) and not outs[0][1].any()


# -- IDCT mirror -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w422_r3", "w444_r2", "w444_7x9", "w422_7x9"])
def test_idct_mirror_against_fp64(written, name):
    idx, want, _, _ = stream_case(written, name)
    surf = vops.jpeg_idct(torch.from_numpy(want), 2, idx.mw, idx.mh, sampling=idx.sampling).numpy()
    fbytes = vops.jpeg_frame_bytes(idx.mw, idx.mh, idx.sampling)[1]
    assert surf.size == 2 * fbytes
    for i in range(2):
        coefs, qt = mjpeg.unpack_record(want[i * idx.record_bytes:(i + 1) * idx.record_bytes],
                                        idx.mw, idx.mh, idx.sampling)
        ideal = mjpeg.idct_planes_f64(coefs, qt, idx.mw, idx.mh, idx.sampling)
        hs, vs = mjpeg.SAMPLING_FACTORS[idx.sampling]
        assert ideal[0].shape == (8 * vs * idx.mh, 8 * hs * idx.mw) and \
            ideal[1].shape == (8 * idx.mh, 8 * idx.mw)
        check_band(surf[i * fbytes:(i + 1) * fbytes], ideal, "%s frame %d" % (name, i))


# -- MjpegDecoder -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN_CHROMA))
def test_golden_files_are_small_and_of_their_sampling(name):
    W, H, sampling = GOLDEN_CHROMA[name][:3]
    path = os.path.join(GOLDEN, name + ".mjpeg")
    assert os.path.getsize(path) < 16384
    idx = mjpeg.read_index(path)
    assert (idx.width, idx.height, idx.sampling, idx.num_frames) == (W, H, sampling, 2)
    assert (idx.restart_interval > 0) == ("restart_marker_rows" in GOLDEN_CHROMA[name][3]
                                          or "restart_marker_blocks" in GOLDEN_CHROMA[name][3])
    if name == "noise_q95_444_blocks":
        assert idx.restart_interval == 3 and idx.mw % 3 != 0


@pytest.mark.parametrize("args", [dict(), dict(entropy="gpu", subseq_bytes=0),
                                  dict(entropy="gpu", subseq_bytes=48)],
                         ids=["host", "gpu", "subseq"])
@pytest.mark.parametrize("name", sorted(GOLDEN_CHROMA))
def test_cpu_decoder_against_pils_rgb(name, args):
    pytest.importorskip("PIL")
    lib()
    check_pil_rgb(name, CPU, **args)


def test_one_decoder_serves_files_of_every_sampling(written):
    """Buffers are sized per request: 4:4:4, then 4:2:0, then 4:2:2 through one
    instance, each equal to a fresh decoder's result."""
    names = ["noise_q95_444_blocks", None, "noise_q90_422_rows"]
    paths = [os.path.join(GOLDEN, (n or "noise_q75_opt") + ".mjpeg") for n in names]
    for args in (dict(), dict(entropy="gpu")):
        one = MjpegDecoder(CPU, clip_length=2, height=20, width=24, dtype=torch.float32, **args)
        for p in paths + paths[::-1]:
            vid, n = one.probe(p)
            fresh = MjpegDecoder(CPU, clip_length=2, height=20, width=24, dtype=torch.float32,
                                 **args)
            assert torch.equal(one.decode(vid, [0]), fresh.decode(fresh.probe(p)[0], [0]))


# -- Y4M ---------------------------------------------------------------------------------------------
def y4m_planes(W, H, frames, seed, sampling):
    return [tuple(p[f] for p in occ.noise_planes(W, H, frames, seed, "bt601", sampling))
            for f in range(frames)]


@pytest.mark.parametrize("W,H,sampling", [(46, 33, "422"), (45, 33, "444"), (46, 34, "420")])
def test_y4m_header_and_decoder(tmp_path, W, H, sampling):
    fr = y4m_planes(W, H, 5, 3, sampling)
    path = str(tmp_path / ("a%s.y4m" % sampling))
    y4m.write_y4m(path, fr, sampling=sampling)
    h = y4m.read_header(path)
    hs, vs = y4m.SAMPLING_FACTORS[sampling]
    payload = W * H + 2 * (W // hs) * (H // vs)
    assert (h.width, h.height, h.sampling, h.num_frames) == (W, H, sampling, 5)
    assert h.colourspace == ("420jpeg" if sampling == "420" else sampling)
    assert h.frame_bytes == payload and h.frame_stride == 6 + payload
    assert h.frame_offset(3) == h.data_offset + 3 * (6 + payload)
    assert os.path.getsize(path) == h.data_offset + 5 * (6 + payload)
    for filt, (ow, oh) in (("bilinear", (24, 16)), ("antialias", (16, 12))):
        dec = Y4mDecoder(CPU, clip_length=2, height=oh, width=ow, dtype=torch.float32,
                         filter=filt)
        vid, n = dec.probe(path)
        assert n == 5
        got = dec.decode(vid, [3, 0]).numpy()
        for c, s in enumerate((3, 0)):
            y, u, v = (np.stack([fr[s + f][p] for f in range(2)]) for p in range(3))
            ref, _, d, tol = occ.tolerance(y, u, v, ow, oh, None, "bt601", sampling, filt)
            assert tol <= orc.TOL_CEILING
            assert np.abs(got[c][..., :3].astype(np.float64) - ref).max() <= tol


def test_y4m_refusals_name_file_and_field(tmp_path):
    def raw(W, H, tokens, payload):
        return b"YUV4MPEG2 W%d H%d %s\n" % (W, H, tokens.encode()) + (b"FRAME\n" + b"\0" * payload)
    for W, H, tokens, payload, field in (
            (45, 33, "F25:1 C422", 45 * 33 * 2, "'W'"),          # Hs = 2: even width
            (46, 33, "F25:1 C420jpeg", 46 * 33 * 3 // 2, "'H'"),  # Vs = 2: even height
            (46, 34, "F25:1 C440", 46 * 34 * 2, "'C'"),
            (46, 34, "F25:1 C411", 46 * 34 * 3 // 2, "'C'"),
            (46, 34, "F25:1 Cmono", 46 * 34, "'C'"),
            (46, 34, "F25:1 C444p10", 46 * 34 * 6, "'C'"),
            (46, 34, "F25:1 C422", 46 * 34 * 3 // 2, "'FRAME'")):  # a 4:2:0 payload
        p = tmp_path / "bad.y4m"
        p.write_bytes(raw(W, H, tokens, payload))
        for call in (y4m.read_header, Y4mDecoder(CPU).probe):
            with pytest.raises(ValueError) as e:
                call(str(p))
            assert "bad.y4m" in str(e.value) and field in str(e.value), str(e.value)
            if field == "'C'":                       # names the format found and what is read
                assert tokens.split()[1] in str(e.value) and "C422" in str(e.value) \
                    and "C444" in str(e.value)
    # odd sizes where the sampling allows them
    (tmp_path / "ok.y4m").write_bytes(raw(46, 33, "F25:1 C422", 46 * 33 * 2))
    assert y4m.read_header(str(tmp_path / "ok.y4m")).num_frames == 1
    (tmp_path / "ok4.y4m").write_bytes(raw(45, 33, "F25:1 C444", 45 * 33 * 3))
    assert y4m.read_header(str(tmp_path / "ok4.y4m")).frame_stride == 6 + 45 * 33 * 3


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        write_golden()
    if "--measure-pil" in sys.argv:
        for g in sorted(GOLDEN_CHROMA):
            print(g, pil_oracle(g)[1])
