"""Motion-JPEG streams on the CPU: the host entropy decoder (librnb_jpeg.so)
against the encoder's own coefficients, the numpy reference decoder and an
independent encoder (PIL), its refusals and its robustness, the IDCT and JFIF
colour mirrors against fp64, and MjpegDecoder / the loader on a CPU device.

``python tests/test_mjpeg_cpu.py --write-golden`` (needs PIL) rewrites the
fixtures under tests/golden/mjpeg/."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rnb_amd.models.r2p1d.decoder import MjpegDecoder, make_decoder  # noqa: E402
from rnb_amd.ops import native  # noqa: E402
from rnb_amd.ops import video as vops  # noqa: E402
from rnb_amd.timecard import TimeCard  # noqa: E402
from rnb_amd.utils import mjpeg  # noqa: E402

CPU = torch.device("cpu")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mjpeg")
SHAPES = [(16, 16), (8, 8), (46, 34)]        # one MCU, one partial MCU, 3x3 padded both ways
ONES = np.ones((2, 64), dtype=np.uint16)
# name -> (W, H, PIL save options); two frames each
GOLDEN_STREAMS = {
    "noise_q75_opt": (46, 34, dict(quality=75, optimize=True)),
    "noise_q95_rows": (48, 32, dict(quality=95, restart_marker_rows=1)),
    "ramp_q30_blocks": (64, 48, dict(quality=30, restart_marker_blocks=2)),
}


def noise_frames(W, H, frames, seed):
    """Random 4:2:0 frames: [(Y [H, W], U, V [ceil(H/2), ceil(W/2)])]."""
    rng = np.random.default_rng(seed)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return [(rng.integers(0, 256, (H, W), dtype=np.uint8),
             rng.integers(0, 256, (ch, cw), dtype=np.uint8),
             rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(frames)]


def ramp_frames(W, H, frames, seed=0):
    """Smooth frames: diagonal ramps that move with the frame number."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:ch, 0:cw]
    out = []
    for f in range(frames):
        y = (xx * 3 + yy * 2 + 11 * f + seed) % 256
        u = (cx * 5 + 7 * f + seed) % 256 + 0 * cy
        v = (cy * 6 + 250 - 5 * f) % 256 + 0 * cx
        out.append(tuple(p.astype(np.uint8) for p in (y, u, v)))
    return out


def sparse_frames(W, H, frames):
    """Frames whose blocks hold little more than the highest-frequency
    coefficient (a different amplitude per block): long zero runs in front of
    a non-zero coefficient, i.e. ZRL codes, under an all-ones table."""
    mw, mh, _ = mjpeg.geometry(W, H)
    basis = np.outer(mjpeg.BASIS[7], mjpeg.BASIS[7])
    out = []
    for f in range(frames):
        planes = []
        for rows, cols, h, w in ((2 * mh, 2 * mw, H, W), (mh, mw, (H + 1) // 2, (W + 1) // 2),
                                 (mh, mw, (H + 1) // 2, (W + 1) // 2)):
            amp = 150.0 + 23.0 * ((np.arange(rows * cols) + 5 * f) % 13)
            p = 128.0 + (amp.reshape(rows, cols, 1, 1) * basis).transpose(0, 2, 1, 3)
            planes.append(np.clip(np.rint(p.reshape(rows * 8, cols * 8)), 0, 255)
                          .astype(np.uint8)[:h, :w])
        out.append(tuple(planes))
    return out


def has_zrl(coefs):
    """Some block has >= 16 zeros in zigzag order in front of a non-zero AC."""
    zz = coefs[:, mjpeg.ZIGZAG]
    for blk in zz:
        nz = np.nonzero(blk[1:])[0] + 1
        if len(nz) and np.max(np.diff(np.concatenate([[0], nz]))) > 16:
            return True
    return False


def native_records(data, idx, threads=1):
    """[(coefs, qt)] of every frame, from librnb_jpeg.so."""
    out = np.zeros(idx.num_frames * idx.record_bytes, dtype=np.uint8)
    mjpeg.entropy_decode(data, idx.offsets, idx.lengths, out, idx.record_bytes, threads)
    return [mjpeg.unpack_record(out[i * idx.record_bytes:(i + 1) * idx.record_bytes],
                                idx.mw, idx.mh) for i in range(idx.num_frames)]


def frame_bytes(data, idx, i):
    return bytes(data[int(idx.offsets[i]):int(idx.offsets[i] + idx.lengths[i])])


def check_band(got, planes_f64, what="", tie_only=False):
    """The IDCT band rule: every sample within 1 level of the rounded fp64
    value; every sample whose fp64 value is further than 1/64 from a
    half-integer equal to it; at most a quarter of the samples inside that
    band. ``got``: flat uint8 planes (Y, Cb, Cr); ``tie_only``: the <= 1 rule
    alone (inputs whose exact values are ties by construction)."""
    ideal = np.concatenate([p.reshape(-1) for p in planes_f64])
    want = np.clip(np.rint(ideal), 0, 255)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    frac = ideal - np.floor(ideal)
    band = np.abs(frac - 0.5) <= 1.0 / 64.0
    print("%s: max |got - round(fp64)| = %d, mismatches %d (all %s the band), band share %.3f"
          % (what, diff.max(), int((diff != 0).sum()),
             "inside" if not (diff[~band] != 0).any() else "NOT inside", band.mean()))
    assert diff.max() <= 1, what
    if tie_only:
        return
    assert not (diff[~band] != 0).any(), what
    assert band.mean() <= 0.25, what


def lib():
    if not native.available("librnb_jpeg.so"):
        pytest.fail("librnb_jpeg.so is not built")
    return native.jpeg()


# -- 1. entropy exactness against the encoder's own coefficients ---------------
@pytest.mark.parametrize("restart", [0, 1, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_entropy_decode_equals_the_encoders_coefficients(tmp_path, W, H, restart):
    lib()
    frames = noise_frames(W, H, 2, W + restart) + sparse_frames(W, H, 1)
    path = str(tmp_path / "n.mjpeg")
    truth = mjpeg.write_mjpeg(path, frames, restart_interval=restart, qtables=ONES)
    big = max(int(np.abs(c).max()) for c, _ in truth)
    # uniform noise gives coefficients of standard deviation 74 under an all-ones
    # table: amplitude categories 8 and up (|v| >= 128) among a few hundred of them
    assert big >= 128, big
    assert has_zrl(truth[2][0])                           # ZRL codes were written
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    mw, mh, rb = mjpeg.geometry(W, H)
    assert (idx.width, idx.height, idx.mw, idx.mh, idx.record_bytes, idx.num_frames) == \
        (W, H, mw, mh, rb, 3)
    assert idx.restart_interval == restart and rb % 16 == 0
    assert int(idx.offsets[0]) == 0 and int(idx.offsets[-1] + idx.lengths[-1]) == data.size
    for threads in (1, 4):
        for i, (coefs, qt) in enumerate(native_records(data, idx, threads)):
            assert np.array_equal(coefs, truth[i][0]), (i, threads)
            assert np.array_equal(qt, truth[i][1]) and qt.max() == 1
    for i in range(3):
        ref = mjpeg.decode_reference(frame_bytes(data, idx, i), planes=False)
        assert np.array_equal(ref["coefs"], truth[i][0]) and np.array_equal(ref["qt"], truth[i][1])
        assert (ref["width"], ref["height"]) == (W, H)


def test_quality_tables_and_per_frame_tables(tmp_path):
    lib()
    q = [np.stack([np.full(64, 1 + 3 * i), np.arange(1, 65) + i]).astype(np.uint16)
         for i in range(3)]
    path = str(tmp_path / "q.mjpeg")
    truth = mjpeg.write_mjpeg(path, ramp_frames(46, 34, 3), qtables=q)
    idx = mjpeg.read_index(path)
    for i, (coefs, qt) in enumerate(native_records(np.fromfile(path, dtype=np.uint8), idx)):
        assert np.array_equal(qt, q[i][[0, 1, 1]]) and np.array_equal(coefs, truth[i][0])
    assert mjpeg.quality_tables(50)[0].tolist() == mjpeg.QT_LUMA.tolist()
    assert mjpeg.quality_tables(100).max() == 1


# -- 2. an independent encoder -------------------------------------------------
def pil_stream(W, H, options, seed=0):
    """(stream bytes, [PIL's own luma plane per frame]) of two PIL-written
    4:2:0 frames; PIL's luma is channel 0 of a ``draft("YCbCr")`` load, its
    IDCT output without colour conversion."""
    import io
    from PIL import Image
    rng = np.random.default_rng(seed)
    data, lumas = b"", []
    for f in range(2):
        if "ramp" in options.get("_kind", ""):
            yy, xx = np.mgrid[0:H, 0:W]
            rgb = np.stack([(xx * 3 + yy + 9 * f) % 256, (yy * 4 + 40 * f) % 256,
                            (xx + yy * 2) % 256], axis=-1).astype(np.uint8)
        else:
            rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        fp = io.BytesIO()
        save = {k: v for k, v in options.items() if not k.startswith("_")}
        Image.fromarray(rgb).save(fp, "JPEG", subsampling="4:2:0", **save)
        one = fp.getvalue()
        im = Image.open(io.BytesIO(one))
        im.draft("YCbCr", (W, H))
        assert im.mode == "YCbCr" and im.size == (W, H)
        lumas.append(np.asarray(im)[:, :, 0].copy())
        data += one
    return data, lumas


def mirror_luma(coefs, qt, idx):
    rec = torch.from_numpy(mjpeg.pack_record(coefs, qt).copy())
    surf = vops.jpeg_idct(rec, 1, idx.mw, idx.mh).numpy()
    return surf[:256 * idx.mw * idx.mh].reshape(16 * idx.mh, 16 * idx.mw)[:idx.height, :idx.width]


@pytest.mark.parametrize("quality", [30, 75, 95])
@pytest.mark.parametrize("options", [dict(optimize=True), dict(restart_marker_rows=1),
                                     dict(restart_marker_blocks=2)],
                         ids=["optimize", "rst_rows", "rst_blocks"])
@pytest.mark.parametrize("W,H,kind", [(46, 34, "noise"), (48, 32, "ramp")])
def test_entropy_decode_of_pil_frames(tmp_path, W, H, kind, options, quality):
    pytest.importorskip("PIL")
    lib()
    data, lumas = pil_stream(W, H, dict(options, quality=quality, _kind=kind), seed=quality)
    path = str(tmp_path / "pil.mjpeg")
    open(path, "wb").write(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    assert (idx.width, idx.height, idx.num_frames) == (W, H, 2)
    if "optimize" not in options:
        assert idx.restart_interval > 0
    worst = 0
    for i, (coefs, qt) in enumerate(native_records(buf, idx)):
        ref = mjpeg.decode_reference(frame_bytes(buf, idx, i), planes=False)
        assert np.array_equal(coefs, ref["coefs"]) and np.array_equal(qt, ref["qt"])
        d = np.abs(mirror_luma(coefs, qt, idx).astype(int) - lumas[i].astype(int))
        worst = max(worst, int(d.max()))
    print("max |mirror luma - PIL luma| =", worst)
    # libjpeg's integer IDCT is within 1 of the rounded ideal IDCT (IEEE 1180),
    # the mirror within 1 of it (test_idct_mirror_against_fp64)
    assert worst <= 2, worst


@pytest.mark.parametrize("name", sorted(GOLDEN_STREAMS))
def test_golden_streams_decode_to_pils_luma(name):
    lib()
    W, H, _ = GOLDEN_STREAMS[name]
    path = os.path.join(GOLDEN, name + ".mjpeg")
    lumas = np.load(os.path.join(GOLDEN, name + "_luma.npy"))
    assert lumas.shape == (2, H, W) and os.path.getsize(path) < 16384
    buf = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    assert (idx.width, idx.height, idx.num_frames) == (W, H, 2)
    for i, (coefs, qt) in enumerate(native_records(buf, idx)):
        ref = mjpeg.decode_reference(frame_bytes(buf, idx, i), planes=False)
        assert np.array_equal(coefs, ref["coefs"])
        d = np.abs(mirror_luma(coefs, qt, idx).astype(int) - lumas[i].astype(int))
        print(name, i, "max |mirror luma - PIL luma| =", d.max(), "mean", d.mean())
        assert d.max() <= 2


# -- 3. refusals ----------------------------------------------------------------
def one_frame(W=46, H=34, restart=0, seed=3):
    frames = noise_frames(W, H, 1, seed)
    q = mjpeg.quality_tables(60)
    return mjpeg.encode_frame(*frames[0], q, restart)[0]


def patched(frame, marker, at, value):
    """``frame`` with the byte ``at`` bytes behind the first ``marker`` replaced."""
    pos = frame.index(marker) + at
    return frame[:pos] + bytes([value]) + frame[pos + 1:]


def refusal_cases():
    f = one_frame()
    sos = f.index(b"\xff\xda")
    scan = f[sos:-2]                                   # SOS segment + entropy-coded data
    return [
        ("progressive", patched(f, b"\xff\xc0", 1, 0xC2), "'SOF'"),
        ("extended", patched(f, b"\xff\xc0", 1, 0xC1), "'SOF'"),
        ("lossless", patched(f, b"\xff\xc0", 1, 0xC3), "'SOF'"),
        ("arithmetic", patched(f, b"\xff\xc0", 1, 0xC9), "'arithmetic'"),
        ("arithmetic_progressive", patched(f, b"\xff\xc0", 1, 0xCA), "'arithmetic'"),
        ("twelve_bit", patched(f, b"\xff\xc0", 4, 12), "'precision'"),
        ("dqt16", patched(f, b"\xff\xdb", 4, 0x10), "'DQT precision'"),
        ("grayscale", patched(f, b"\xff\xc0", 9, 1), "'components'"),
        ("four_components", patched(f, b"\xff\xc0", 9, 4), "'components'"),
        ("s422", patched(f, b"\xff\xc0", 11, 0x21), "'sampling'"),
        ("s444", patched(f, b"\xff\xc0", 11, 0x11), "'sampling'"),
        ("chroma_2x1", patched(f, b"\xff\xc0", 14, 0x21), "'sampling'"),
        ("two_scans", f[:-2] + scan + b"\xff\xd9", "'scans'"),
        ("one_component_scan", patched(f, b"\xff\xda", 4, 1), "'scans'"),
        ("spectral_selection", patched(f, b"\xff\xda", 12, 5), "'scans'"),
        ("no_eoi", f[:-2], "'EOI'"),
        ("no_soi", b"\x00" + f[1:], "'SOI'"),
        ("zero_height", patched(patched(f, b"\xff\xc0", 5, 0), b"\xff\xc0", 6, 0), "'dimensions'"),
    ]


@pytest.mark.parametrize("name,data,field", refusal_cases(), ids=[c[0] for c in refusal_cases()])
def test_unsupported_frames_are_refused_naming_file_and_field(tmp_path, name, data, field):
    lib()
    path = str(tmp_path / "bad.mjpeg")
    open(path, "wb").write(data)
    for call in (mjpeg.read_index, MjpegDecoder(CPU).probe):
        with pytest.raises(ValueError) as e:
            call(path)
        assert "bad.mjpeg" in str(e.value) and field in str(e.value), str(e.value)
    # the decoder refuses the frame by itself too, with a negative code
    buf = np.frombuffer(data, dtype=np.uint8)
    rec = np.zeros(mjpeg.geometry(46, 34)[2], dtype=np.uint8)
    assert lib().decode_frames_rc(buf, [0], [buf.size], rec, rec.size) < 0


def test_refusal_codes_are_distinct():
    j = lib()
    names = [j.error_name(c) for c in range(-20, 0)]
    assert len(set(names)) == 20 and "unknown" not in names
    codes = {}
    for name, data, field in refusal_cases():
        buf = np.frombuffer(data, dtype=np.uint8)
        codes[name] = j.lib.rnb_mjpeg_index(buf.ctypes.data, buf.size, None, None, 0,
                                            (native.ctypes.c_int * 4)())
    print(codes)
    assert all(c < 0 for c in codes.values())
    # one code per reason the issue lists
    assert len({codes[k] for k in ("progressive", "arithmetic", "twelve_bit", "dqt16", "grayscale",
                                   "s422", "two_scans", "no_eoi")}) == 8


def test_stream_level_refusals(tmp_path):
    lib()
    a, b = one_frame(16, 16), one_frame(8, 8)
    path = str(tmp_path / "mixed.mjpeg")
    open(path, "wb").write(a + a + b)
    with pytest.raises(ValueError, match=r"mixed\.mjpeg: frame 2 .*'size'"):
        mjpeg.read_index(path)
    with pytest.raises(ValueError, match=r"mixed\.mjpeg: frame 2 .*'size'"):
        MjpegDecoder(CPU).probe(path)
    path = str(tmp_path / "cut.mjpeg")
    open(path, "wb").write((a + a + a)[:-2])              # last frame without its EOI
    with pytest.raises(ValueError, match=r"cut\.mjpeg: frame 2 .*'EOI'"):
        MjpegDecoder(CPU).probe(path)
    path = str(tmp_path / "empty.mjpeg")
    open(path, "wb").write(b"")
    with pytest.raises(ValueError, match=r"empty\.mjpeg.*'SOI'"):
        MjpegDecoder(CPU).probe(path)
    # a frame of another size among the sampled ones is refused by the decoder too
    buf = np.frombuffer(a + b, dtype=np.uint8)
    rec = np.zeros(2 * 1152, dtype=np.uint8)
    rc = lib().decode_frames_rc(buf, [0, len(a)], [len(a), len(b)], rec, 1152)
    assert lib().error_name(rc) == "size"
    # a clip outside the frame count
    path = str(tmp_path / "ok.mjpeg")
    open(path, "wb").write(a * 10)
    dec = MjpegDecoder(CPU, clip_length=4, dtype=torch.float32)
    vid, n = dec.probe(path)
    assert n == 10 and dec.probe(path) == (vid, 10)
    assert dec.decode(vid, [0, 6]).shape == (2, 4, 112, 112, 4)
    for starts in ([7], [-1], [0, 10]):
        with pytest.raises(ValueError, match=r"ok\.mjpeg.*outside"):
            dec.decode(vid, starts)
    with pytest.raises(KeyError):
        dec.decode(99, [0])


def test_restart_markers_are_checked():
    j = lib()
    f = one_frame(46, 34, restart=2)
    buf = np.frombuffer(f, dtype=np.uint8)
    rec = np.zeros(mjpeg.geometry(46, 34)[2], dtype=np.uint8)
    assert j.decode_frames_rc(buf, [0], [buf.size], rec, rec.size) == 0
    pos = f.index(b"\xff\xd1")
    wrong = np.frombuffer(f[:pos + 1] + b"\xd3" + f[pos + 2:], dtype=np.uint8)    # RST1 -> RST3
    assert j.error_name(j.decode_frames_rc(wrong, [0], [wrong.size], rec, rec.size)) == "RST"
    missing = np.frombuffer(f[:pos] + f[pos + 2:], dtype=np.uint8)
    assert j.decode_frames_rc(missing, [0], [missing.size], rec, rec.size) < 0
    short = np.zeros(rec.size - 16, dtype=np.uint8)
    assert j.error_name(j.decode_frames_rc(buf, [0], [buf.size], short, short.size)) == "record"


# -- 4. corrupt input never crashes ------------------------------------------------
def test_truncated_and_corrupted_frames_return_a_code():
    j = lib()
    f = one_frame(46, 34, restart=3, seed=8)
    rb = mjpeg.geometry(46, 34)[2]
    rec = np.zeros(rb, dtype=np.uint8)
    ok = refused = 0
    for i in range(64):
        cut = np.frombuffer(f[:len(f) * i // 64], dtype=np.uint8).copy()
        rc = j.decode_frames_rc(cut, [0], [cut.size], rec, rb)
        assert rc < 0, (i, rc)                      # every truncation loses the EOI at least
        info = (native.ctypes.c_int * 4)()
        assert j.lib.rnb_mjpeg_index(cut.ctypes.data, cut.size, None, None, 0, info) <= 0
    rng = np.random.default_rng(1234)
    for i in range(500):
        bad = np.frombuffer(f, dtype=np.uint8).copy()
        bad[rng.integers(0, bad.size)] ^= rng.integers(1, 256)
        rc = j.decode_frames_rc(bad, [0], [bad.size], rec, rb)
        assert rc <= 0, (i, rc)
        ok += rc == 0
        refused += rc < 0
    print("500 corruptions: %d decoded, %d refused" % (ok, refused))
    assert ok + refused == 500 and refused > 0


def test_standalone_check_program_under_sanitizers(tmp_path):
    """csrc/bench/jpeg_entropy_check.cpp + jpeg_entropy.cpp built with
    -fsanitize=address,undefined and run directly (never loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_entropy_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "csrc", "jpeg_entropy.cpp"),
                            os.path.join(ROOT, "csrc", "bench", "jpeg_entropy_check.cpp"),
                            "-pthread", "-o", exe], capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr
                                  or "clang_rt" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    path = str(tmp_path / "s.mjpeg")
    mjpeg.write_mjpeg(path, noise_frames(46, 34, 2, 21), quality=80, restart_interval=3)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(run.stdout[-500:], run.stderr[-3000:])
    assert run.returncode == 0 and "no fault" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr


# -- 5. the IDCT mirror against fp64 -------------------------------------------------
def idct_inputs(W, H):
    """name -> [(coefs, qt)] x 6 frames, a different table on every frame:
    encoder output of noise and ramp images, and hand-made blocks."""
    mw, mh, _ = mjpeg.geometry(W, H)
    nb = 6 * mw * mh
    tables = [np.stack([np.clip(mjpeg.QT_LUMA * (i + 1) // 3, 1, 255),
                        np.clip(mjpeg.QT_CHROMA * (i + 2) // 4, 1, 255)]).astype(np.uint16)
              for i in range(6)]
    out = {}
    for kind, frames in (("noise", noise_frames(W, H, 6, 40 + W)), ("ramp", ramp_frames(W, H, 6))):
        out[kind] = [(mjpeg.encode_frame(*f, tables[i])[1], tables[i][[0, 1, 1]])
                     for i, f in enumerate(frames)]
    rng = np.random.default_rng(W * H)
    single, clamp, dc = [], [], []
    for i in range(6):
        qt = tables[i][[0, 1, 1]]
        c = np.zeros((nb, 64), dtype=np.int16)            # one AC coefficient at its extremes
        pos = rng.integers(1, 64, nb)
        c[np.arange(nb), pos] = np.where(rng.integers(0, 2, nb) == 1, 1023, -1023)
        c[:, 0] = rng.integers(-60, 60, nb)
        single.append((c, qt))
        c = rng.integers(-1023, 1024, (nb, 64)).astype(np.int16)    # far outside [0, 255]
        c[:, 0] = np.where(np.arange(nb) % 2 == 0, 1016, -1024)
        clamp.append((c, qt))
        c = np.zeros((nb, 64), dtype=np.int16)            # DC only: flat blocks, exact ties
        c[:, 0] = rng.integers(-1024, 1017, nb)
        dc.append((c, np.full((3, 64), 4 * (i + 1), dtype=np.uint16)))
    out.update(single_ac=single, clamp=clamp, dc_only=dc)
    return out


def records_tensor(frames):
    return torch.from_numpy(np.concatenate([mjpeg.pack_record(c, q) for c, q in frames]))


def ideal_planes(frames, mw, mh):
    """fp64 planes of all frames: a flat list (Y0, Cb0, Cr0, Y1, ...)."""
    return [p for c, q in frames for p in mjpeg.idct_planes_f64(c, q, mw, mh)]


@pytest.mark.parametrize("W,H", SHAPES)
def test_idct_mirror_against_fp64(W, H):
    mw, mh, rb = mjpeg.geometry(W, H)
    for kind, frames in idct_inputs(W, H).items():
        got = vops.jpeg_idct(records_tensor(frames), 6, mw, mh).numpy()
        assert got.shape == (6 * 384 * mw * mh,)
        check_band(got, ideal_planes(frames, mw, mh), "%dx%d %s" % (W, H, kind),
                   tie_only=kind == "dc_only")
        if kind == "clamp":
            assert (got == 0).any() and (got == 255).any()
    with pytest.raises(ValueError, match="outside"):
        vops.jpeg_idct(torch.zeros(rb - 16, dtype=torch.uint8), 1, mw, mh)
    with pytest.raises(ValueError, match="out must be"):
        vops.jpeg_idct(torch.zeros(rb, dtype=torch.uint8), 1, mw, mh,
                       out=torch.zeros(384 * mw * mh, dtype=torch.int8))


# -- 6. the JFIF matrix ----------------------------------------------------------------
def parent_planes_to_clip(y_plane, u_plane, v_plane, shape, crop):
    """The clip mirror's BT.601 arithmetic as it stood before ``matrix=`` was
    added (fp32 result, Kinetics normalisation)."""
    out_h, out_w = shape[-3], shape[-2]
    ox = torch.arange(out_w, dtype=torch.float32)
    oy = torch.arange(out_h, dtype=torch.float32)
    sx = crop[0] + (ox + 0.5) * (crop[2] / out_w) - 0.5
    sy = crop[1] + (oy + 0.5) * (crop[3] / out_h) - 0.5
    yv = vops._bilinear_torch(y_plane, sx, sy)
    cx, cy = (sx + 0.5) * 0.5 - 0.5, (sy + 0.5) * 0.5 - 0.5
    u = vops._bilinear_torch(u_plane, cx, cy) - 128.0
    v = vops._bilinear_torch(v_plane, cx, cy) - 128.0
    yy = 1.164 * (yv - 16.0)
    rgb = torch.stack([yy + 1.596 * v, yy - 0.392 * u - 0.813 * v, yy + 2.017 * u], dim=-1)
    scale, shift = vops._norm32(vops.KINETICS_MEAN, vops.KINETICS_STD)
    rgb = rgb.clamp(0.0, 255.0) * scale + shift
    res = torch.zeros(shape, dtype=torch.float32)
    res.view(-1, out_h, out_w, shape[-1])[..., :3] = rgb
    return res


@pytest.mark.parametrize("crop", [None, (6.0, 0.0, 34.0, 34.0)])
def test_bt601_is_what_it_was(crop):
    """The inputs of test_cpu_decode_equals_the_nv12_mirror: the default and
    the explicit ``matrix="bt601"`` equal the arithmetic before this option."""
    from test_y4m_cpu import planes
    W, H, F = 46, 34, 8
    fr = planes(W, H, 20, 5)
    sel = [fr[s + f] for s in (0, 5, 12) for f in range(F)]
    buf = torch.from_numpy(np.concatenate([np.concatenate([p.reshape(-1) for p in f])
                                           for f in sel]))
    fb = W * H * 3 // 2
    offs = [0, F * fb, 2 * F * fb]
    a = vops.yuv420_to_clip(buf, offs, F, W, H, fb, vops.i420_planes(W, H), crop=crop)
    b = vops.yuv420_to_clip(buf, offs, F, W, H, fb, vops.i420_planes(W, H), crop=crop,
                            matrix="bt601")
    box = crop or (0.0, 0.0, float(W), float(H))
    old = parent_planes_to_clip(torch.from_numpy(np.stack([f[0] for f in sel])).float(),
                                torch.from_numpy(np.stack([f[1] for f in sel])).float(),
                                torch.from_numpy(np.stack([f[2] for f in sel])).float(),
                                (3, F, 112, 112, 4), box)
    assert torch.equal(a, old) and torch.equal(b, old)
    with pytest.raises(ValueError, match="matrix"):
        vops.yuv420_to_clip(buf, offs, F, W, H, fb, vops.i420_planes(W, H), matrix="bt709")


@pytest.mark.parametrize("W,H", [(46, 34), (45, 33)])
def test_jfif_mirror_against_the_formula_in_fp64(W, H):
    """Random planes (odd sizes too: chroma planes round up) through the
    mirror in fp32 against the mirror's own sampler (``_bilinear_torch``) and
    coordinate expressions evaluated in fp64, followed by the JFIF formula:
    a check of the mirror's fp32 arithmetic, of the matrix as written here and
    of the clamp, NOT of the mapping, the chroma siting or the tap selection,
    which both sides share. Those are checked against an independent
    reference in test_decode_oracle_cpu.py."""
    rng = np.random.default_rng(W)
    cw, ch = (W + 1) // 2, (H + 1) // 2
    F = 2
    y = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    u = rng.integers(0, 256, (F, ch, cw), dtype=np.uint8)
    v = rng.integers(0, 256, (F, ch, cw), dtype=np.uint8)
    fb = W * H + 2 * cw * ch
    buf = torch.from_numpy(np.concatenate([np.concatenate([y[f].reshape(-1), u[f].reshape(-1),
                                                           v[f].reshape(-1)]) for f in range(F)]))
    pl = vops.YuvPlanes(0, W * H, W * H + cw * ch, W, cw, cw, 1)
    crop = (1.0, 2.0, W - 3.0, H - 4.0)
    got = vops.yuv420_to_clip(buf, [0], F, W, H, fb, pl, 24, 16, crop=crop, matrix="jfif")
    assert got.shape == (1, F, 16, 24, 4) and torch.all(got[..., 3] == 0)
    ox, oy = torch.arange(24, dtype=torch.float64), torch.arange(16, dtype=torch.float64)
    sx = crop[0] + (ox + 0.5) * (crop[2] / 24) - 0.5
    sy = crop[1] + (oy + 0.5) * (crop[3] / 16) - 0.5

    def sample(plane, px, py):
        return vops._bilinear_torch(torch.from_numpy(plane).double(), px, py)
    Y = sample(y, sx, sy)
    Cb = sample(u, (sx + 0.5) * 0.5 - 0.5, (sy + 0.5) * 0.5 - 0.5) - 128.0
    Cr = sample(v, (sx + 0.5) * 0.5 - 0.5, (sy + 0.5) * 0.5 - 0.5) - 128.0
    rgb = torch.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], dim=-1)
    mean = torch.tensor(vops.KINETICS_MEAN, dtype=torch.float64)
    std = torch.tensor(vops.KINETICS_STD, dtype=torch.float64)
    ref = (rgb.clamp(0, 255) / 255.0 - mean) / std
    err = (got[0, ..., :3].double() - ref).abs().max().item()
    print("max |jfif mirror - fp64 formula| =", err)
    # fp32 arithmetic on values below 2^10, normalised by 1 / (255 * 0.217): ~1e-5
    assert err <= 1e-4, err
    assert (rgb < 0).any() and (rgb > 255).any()          # the clamp is exercised
    with pytest.raises(ValueError, match="even"):
        vops.yuv420_to_clip(buf, [0], F, 45, 33, fb, pl, 24, 16)      # bt601 needs even sizes


# -- 7. decoder, loader, factory ----------------------------------------------------------
def test_cpu_decode_equals_reference_planes_through_the_clip_mirror(tmp_path):
    """MjpegDecoder on a CPU device against decode_reference's planes fed to
    the clip mirror at the frame's true size."""
    W, H, F = 46, 34, 3
    path = str(tmp_path / "v.mjpeg")
    mjpeg.write_mjpeg(path, ramp_frames(W, H, 9), quality=85, restart_interval=2)
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    for crop, box in (("full", None), ("center", (6.0, 0.0, 34.0, 34.0))):
        dec = MjpegDecoder(CPU, clip_length=F, height=16, width=24, dtype=torch.float32,
                           crop=crop, threads=2)
        vid, n = dec.probe(path)
        assert n == 9
        got = dec.decode(vid, [0, 5])
        assert got.shape == (2, F, 16, 24, 4)
        surf = np.concatenate([np.concatenate([p.reshape(-1) for p in mjpeg.decode_reference(
            frame_bytes(data, idx, s + f))["planes_u8"]]) for s in (0, 5) for f in range(F)])
        fbytes = 384 * idx.mw * idx.mh
        ref = vops.yuv420_to_clip(torch.from_numpy(surf), [0, F * fbytes], F, W, H, fbytes,
                                  vops.jpeg_surface_planes(idx.mw, idx.mh), 24, 16, crop=box,
                                  matrix="jfif")
        # the mirror IDCT may differ from the fp64 one by a level at a tie, in Y and in
        # a chroma plane at once: (1 + 1.772) levels of 1 / (255 * 0.217) each
        assert (got - ref).abs().max().item() <= 0.051
    assert dec.decode(vid, []).shape == (0, F, 16, 24, 4)
    slot = torch.full((4, F, 16, 24, 8), 7.0, dtype=torch.bfloat16)
    d16 = MjpegDecoder(CPU, clip_length=F, height=16, width=24, dtype=torch.bfloat16)
    v16, _ = d16.probe(path)
    out = d16.decode(v16, [6], out=slot[:1])
    assert out.data_ptr() == slot.data_ptr() and torch.all(slot[1:] == 7.0)
    assert torch.all(slot[0, ..., 3:] == 0)


def test_loader_with_mjpeg_decoder(tmp_path):
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    pa, pb = str(tmp_path / "a.mjpeg"), str(tmp_path / "b.mjpg")
    mjpeg.write_mjpeg(pa, ramp_frames(46, 34, 40), quality=80)
    mjpeg.write_mjpeg(pb, ramp_frames(64, 48, 30, seed=9), quality=60, restart_interval=4)
    loader = R2P1DLoader(CPU, decoder="mjpeg", num_clips_population=[2], num_clips_weights=[1],
                         seed=0, dtype="fp32", decoder_args={"depth": 2, "threads": 2})
    dec = loader.decoder
    assert isinstance(dec, MjpegDecoder) and dec.depth == 2 and dec.threads == 2
    (va, na), (vb, nb) = dec.probe(pa), dec.probe(pb)
    assert (na, nb) == (40, 30) and va != vb
    tc = TimeCard(13)
    (frames,), _, tc = loader((None,), pb, tc)
    assert frames.shape == (2, 8, 112, 112, 4) and tc.num_clips == 2
    _, starts = tc.extra["clip_src"]
    assert torch.equal(frames, dec.decode(vb, starts))
    assert not torch.equal(frames, dec.decode(va, starts))
    assert torch.isfinite(frames).all() and frames[..., :3].abs().max() > 0.5


def test_make_decoder_mjpeg():
    dec = make_decoder("mjpeg", CPU, dtype=torch.float32,
                       decoder_args={"crop": "center", "threads": 16, "depth": 3})
    assert isinstance(dec, MjpegDecoder) and (dec.crop, dec.threads, dec.depth) == ("center", 16, 3)
    assert make_decoder("mjpeg", CPU).threads == 4
    for bad in ({"crop": "left"}, {"threads": 0}, {"threads": 17}, {"threads": 2.5},
                {"threads": "4"}, {"depth": 0}, {"depth": -1}, {"depth": 1.5}):
        with pytest.raises(ValueError):
            make_decoder("mjpeg", CPU, decoder_args=bad)
    with pytest.raises(RuntimeError, match="'mjpeg'"):
        make_decoder("rocdecode", CPU)
    dec.warmup(2)                                         # needs no file


def pil_rgb(path):
    """PIL's own RGB of every frame of a stream: uint8 [frames, H, W, 3]
    (libjpeg's IDCT, its "fancy" chroma upsampling and its colour conversion)."""
    import io
    from PIL import Image
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    return np.stack([np.asarray(Image.open(io.BytesIO(frame_bytes(data, idx, i))).convert("RGB"))
                     for i in range(idx.num_frames)])


def write_golden():
    """Streams and PIL's luma as PIL writes and reads them here; a stream that
    is already there and that this PIL version would encode differently is
    kept (with its luma), and only PIL's RGB of it is written."""
    os.makedirs(GOLDEN, exist_ok=True)
    for name, (W, H, options) in GOLDEN_STREAMS.items():
        kind = "ramp" if name.startswith("ramp") else "noise"
        data, lumas = pil_stream(W, H, dict(options, _kind=kind), seed=len(name))
        path = os.path.join(GOLDEN, name + ".mjpeg")
        if os.path.exists(path) and open(path, "rb").read() != data:
            print(name, "kept: this PIL version encodes it differently")
        else:
            open(path, "wb").write(data)
            np.save(os.path.join(GOLDEN, name + "_luma.npy"), np.stack(lumas))
        rgb = pil_rgb(path)
        assert rgb.shape == (2, H, W, 3) and rgb.dtype == np.uint8
        np.save(os.path.join(GOLDEN, name + "_rgb.npy"), rgb)
        print(name, len(data), "bytes")


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        write_golden()
