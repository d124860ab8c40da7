"""Restart-less MJPEG scans decoded by synchronised subsequences
(csrc/jpeg_huff.h), through the kernel's host emulation
rnb_jpeg_decode_scans_subseq_host: byte-for-byte equality with the serial
decoders in records and status on clean, damaged, truncated and corrupted
scans, the round counts' bounds, the stand-alone sanitizer program, and
subseq_bytes through the op, MjpegDecoder, make_decoder and the config on a
CPU device. The helpers here also serve tests/test_gpu_mjpeg_subseq.py.
"""
import json
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

from rnb_amd.config import load_pipeline  # noqa: E402
from rnb_amd.models.r2p1d.decoder import MjpegDecoder, make_decoder  # noqa: E402
from rnb_amd.ops import video as vops  # noqa: E402
from rnb_amd.utils import mjpeg  # noqa: E402
from test_mjpeg_cpu import lib, noise_frames, one_frame  # noqa: E402
from test_mjpeg_scan_cpu import build_matrix, corrupt_one_frame, host_records, packed  # noqa: E402

CPU = torch.device("cpu")
SIZES = (16, 64, 256)
# restart-less streams, then two with restart markers (one lane per interval, as before)
STREAMS = ("one_mcu", "partial_mcu", "r0", "noise_q75_opt", "noise_144", "noise_144_q95", "r2",
           "two_passes")
BODY = 2032 + 8                      # where a one-interval scan record's scan bytes start


def build_streams(d):
    """build_matrix's streams plus ``noise_144``: one 144x128 noise frame at
    quality 75 without restart markers, ~920 subsequences at S = 16 (more than
    one per lane), and ``noise_144_q95``, the same at quality 95: a scan of
    more than 16 KB, for which S = 16 is raised so that 1024 subsequences
    cover it."""
    out = build_matrix(d)
    for name, quality in (("noise_144", 75), ("noise_144_q95", 95)):
        path = os.path.join(str(d), name + ".mjpeg")
        out[name] = (path, mjpeg.write_mjpeg(path, noise_frames(144, 128, 1, 5), quality=quality))
    return out


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    return build_streams(tmp_path_factory.mktemp("subseq"))


def span_of(rec):
    """(n_intervals, begin, end) of the first span of one scan record."""
    return tuple(int(x) for x in (rec[2016:2020].view(np.uint32)[0],
                                  rec[2032:2036].view(np.uint32)[0],
                                  rec[2036:2040].view(np.uint32)[0]))


def subsequences(rec, S):
    """Subsequences the decoders cut the record's scan into (1: not split)."""
    n_int, begin, end = span_of(rec)
    if n_int != 1 or end <= begin:
        return 1
    n = -(-(end - begin) // S)
    if n > 1024:                                         # the raised effective S
        S = (-(-(end - begin) // 1024) + 15) // 16 * 16
        n = -(-(end - begin) // S)
    return n


def boundaries_on_stuffing(rec, S):
    """Boundaries of the record's subsequences that fall on the 00 of an FF 00 pair."""
    _, begin, end = span_of(rec)
    scan = rec[BODY:]
    return sum(1 for b in range(begin + S, end, S) if scan[b] == 0x00 and scan[b - 1] == 0xFF)


def stream_case(streams, name):
    """(idx, serial host records, scan records, offsets) of a stream."""
    path, _ = streams[name]
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    scans, offs = packed(data, idx)
    return idx, host_records(data, idx), scans, offs


def check_rounds(name, S, idx, scans, offs, rounds):
    """The bounds every round count obeys."""
    for i in range(idx.num_frames):
        n_sub = subsequences(scans[int(offs[i]):int(offs[i + 1])], S)
        assert 0 <= rounds[i] <= max(n_sub - 1, 0), (name, S, i, rounds[i], n_sub)
        if n_sub == 1 or idx.restart_interval:
            assert rounds[i] == 0, (name, S, i)
    if name == "r0" and S == 16:
        assert min(rounds) >= 2, rounds
    if name == "noise_144" and S == 16:
        assert 256 < subsequences(scans, 16) < 1024       # lanes own several subsequences
    if name == "noise_144_q95" and S == 16:
        _, begin, end = span_of(scans)                    # S is raised: 32-byte subsequences
        assert end - begin > 16 * 1024 and subsequences(scans, 16) == -(-(end - begin) // 32)


def dc_range_record(streams):
    """A hand-built 144x128 scan record (tables and header of the noise_144
    stream, the scan from the encoder's bit writer) whose luma DC differences
    are all +2047 and whose other symbols are EOB: the luma predictor leaves
    int16 at the 17th luma block, which only a decode from the true predictors
    can see."""
    idx, _, scans, offs = stream_case(streams, "noise_144")
    assert (idx.mw, idx.mh) == (9, 8) and span_of(scans)[0] == 1
    dcl, acl = mjpeg._codes(*mjpeg.HUFF_DC_LUMA), mjpeg._codes(*mjpeg.HUFF_AC_LUMA)
    dcc, acc = mjpeg._codes(*mjpeg.HUFF_DC_CHROMA), mjpeg._codes(*mjpeg.HUFF_AC_CHROMA)
    bw = mjpeg._BitWriter()
    for _ in range(idx.mw * idx.mh):
        for _ in range(4):
            bw.put(*dcl[11])
            bw.put(2047, 11)
            bw.put(*acl[0x00])
        for _ in range(2):
            bw.put(*dcc[0])
            bw.put(*acc[0x00])
    bw.flush()
    body = np.frombuffer(bytes(bw.out), dtype=np.uint8)
    rec = np.zeros((BODY + body.size + 15) // 16 * 16, dtype=np.uint8)
    rec[:BODY] = scans[:BODY]
    rec[BODY:BODY + body.size] = body
    rec[2024:2028].view(np.uint32)[0] = body.size
    rec[2032:2040].view(np.uint32)[:] = (0, body.size)
    return idx, rec


def damaged_subseq_records(streams):
    """(idx, clean scan record, {name: damaged copy}) of frame 0 of the
    restart-less 46x34 stream ``r0``: the fixed list that the emulation, the
    sanitizer program and then the GPU kernel are given."""
    idx, _, scans, offs = stream_case(streams, "r0")
    clean = scans[:int(offs[1])].copy()
    n_int, begin, end = span_of(clean)
    scan_len = int(clean[2024:2028].view(np.uint32)[0])
    assert n_int == 1 and begin == 0 and end > 1200
    out = {}

    def case(name, at=None, xor=None, u32=None, value=None):
        bad = clean.copy()
        if u32 is not None:
            bad[at:at + 4].view(np.uint32)[0] = u32
        elif value is not None:
            bad[at] = value
        else:
            bad[at] ^= xor
        assert not np.array_equal(bad, clean), name
        out[name] = bad
    # 8 single flipped bytes spread over the scan; 129 and 1023 lie within 2
    # bytes of a boundary of both S = 16 and S = 128. The serial decoder reads
    # on through the flips at 129 and 770 without a code (other coefficients,
    # status 0) and refuses the other six: both outcomes are in the list.
    for at, xor in ((3, 0x55), (129, 0x80), (300, 0x3C), (517, 0xAA), (770, 0xAA), (1023, 0x55),
                    (end - 40, 0x80), (end - 2, 0x11)):
        case("flip_%04d" % at, BODY + at, xor=xor)
    for cut in (1, 7, 100):
        case("end_minus_%d" % cut, 2036, u32=end - cut)
    case("begin_past_end", 2032, u32=end + 1)
    case("luma_ac_count_raised", 384 + 272 + 15, value=int(clean[384 + 272 + 15]) + 40)
    case("two_intervals", 2016, u32=2)
    # 40 bytes of A5 behind the last block: the scan and its span grow
    grown = np.zeros((BODY + scan_len + 40 + 15) // 16 * 16, dtype=np.uint8)
    grown[:BODY + scan_len] = clean[:BODY + scan_len]
    grown[BODY + scan_len:BODY + scan_len + 40] = 0xA5
    grown[2024:2028].view(np.uint32)[0] = scan_len + 40
    grown[2036:2040].view(np.uint32)[0] = end + 40
    out["a5_behind_the_last_block"] = grown
    return idx, clean, out


def both_decoders(rec, mw, mh, S):
    """((serial records, status), (emulation records, status, rounds)) of one record."""
    offs = np.array([0, rec.size], dtype=np.int64)
    return (mjpeg.decode_scans_host(rec, offs, 1, mw, mh),
            mjpeg.decode_scans_host(rec, offs, 1, mw, mh, subseq_bytes=S, return_rounds=True))


# -- 1. equality on clean streams ------------------------------------------------------
@pytest.mark.parametrize("name", STREAMS)
def test_emulation_records_equal_the_serial_decoders(streams, name):
    lib()
    idx, want, scans, offs = stream_case(streams, name)
    n = idx.num_frames
    serial, serial_status = mjpeg.decode_scans_host(scans, offs, n, idx.mw, idx.mh)
    assert (serial == want).all() and not serial_status.any()
    for S in SIZES:
        out = np.full(want.size + 16, 0x5A, dtype=np.uint8)
        got, status, rounds = mjpeg.decode_scans_host(scans, offs, n, idx.mw, idx.mh, out=out,
                                                      subseq_bytes=S, return_rounds=True)
        assert status.tolist() == [0] * n, (name, S)
        assert (out[:want.size] == want).all(), (name, S)
        assert (out[want.size:] == 0x5A).all()
        print(name, "S = %d: rounds %s, subsequences %s"
              % (S, rounds.tolist(), [subsequences(scans[int(offs[i]):int(offs[i + 1])], S)
                                      for i in range(n)]))
        check_rounds(name, S, idx, scans, offs, rounds.tolist())
    # the CPU op is the same emulation
    rounds_t = torch.full((n,), -1, dtype=torch.int32)
    rec, status = vops.jpeg_huff(torch.from_numpy(scans), offs, n, idx.mw, idx.mh,
                                 subseq_bytes=64, rounds=rounds_t)
    assert (rec.numpy() == want).all() and status.tolist() == [0] * n
    assert rounds_t.min() >= 0
    assert (rounds_t.max() > 0) == (name not in ("r2", "two_passes"))


def test_r0_boundaries_fall_on_stuffing_bytes(streams):
    """The stuffing case is in the inputs: some S = 16 boundary of r0 frame 0
    falls on the 00 of an FF 00 pair (and is decoded right, above)."""
    _, _, scans, offs = stream_case(streams, "r0")
    count = boundaries_on_stuffing(scans[:int(offs[1])], 16)
    print("r0 frame 0: %d boundaries on a stuffing byte at S = 16" % count)
    assert count >= 1


# -- 2. damaged records ------------------------------------------------------------------
def test_damaged_records_equal_the_serial_decoder(streams):
    lib()
    idx, clean, cases = damaged_subseq_records(streams)
    refused = 0
    for name, bad in [("clean", clean)] + sorted(cases.items()):
        (want, ws), _ = both_decoders(bad, idx.mw, idx.mh, 16)
        refused += int(ws[0] < 0)
        for S in (16, 128):
            _, (got, gs, rounds) = both_decoders(bad, idx.mw, idx.mh, S)
            assert gs[0] == ws[0], (name, S, int(gs[0]), int(ws[0]))
            assert (got == want).all(), (name, S)
        print(name, int(ws[0]), mjpeg.status_field(int(ws[0])) if ws[0] else "ok")
    assert refused >= 8                                   # on the serial result alone
    big, rec = dc_range_record(streams)
    (want, ws), _ = both_decoders(rec, big.mw, big.mh, 16)
    assert mjpeg.status_field(int(ws[0])) == "dc_range"
    coefs, _ = mjpeg.unpack_record(want, big.mw, big.mh)
    # 16 luma blocks = MCUs 0..3 hold 2047, 4094, ...; the 17th and everything behind is zero
    assert coefs[[0, 1, 18, 19], 0].tolist() == [2047, 4094, 6141, 8188]
    assert coefs[25, 0] == 16 * 2047 and not coefs[8:18].any() and not coefs[26:].any()
    for S in (16, 128):
        _, (got, gs, rounds) = both_decoders(rec, big.mw, big.mh, S)
        assert gs[0] == ws[0] and (got == want).all(), S


def test_truncated_and_corrupted_restartless_frames_equal_the_serial_mirror():
    """The 64 truncations and the 500 seeded single-byte corruptions of
    test_truncated_and_corrupted_frames_same_decision_as_the_host_decoder on a
    frame without restart markers: wherever the packer accepts, the emulation
    gives the serial mirror's status and record at S = 16 and S = 128."""
    j = lib()
    f = one_frame(46, 34, restart=0, seed=8)
    mw, mh, rb = mjpeg.geometry(46, 34)
    frames = [f[:len(f) * i // 64] for i in range(64)]
    rng = np.random.default_rng(1234)
    for i in range(500):
        bad = np.frombuffer(f, dtype=np.uint8).copy()
        bad[rng.integers(0, bad.size)] ^= rng.integers(1, 256)
        frames.append(bad.tobytes())
    packed_ok = refused = 0
    for i, frame in enumerate(frames):
        buf = np.frombuffer(frame, dtype=np.uint8).copy()
        out = np.zeros(mjpeg.scan_record_bound(mw, mh, buf.size), dtype=np.uint8)
        n, _ = j.pack_scans(buf, [0], [buf.size], out, 46, 34) if buf.size else (-2, 0)
        if n < 0:
            continue
        packed_ok += 1
        (want, ws), _ = both_decoders(out[:n], mw, mh, 16)
        refused += int(ws[0] < 0)
        for S in (16, 128):
            _, (got, gs, _) = both_decoders(out[:n], mw, mh, S)
            assert gs[0] == ws[0] and (got == want).all(), (i, S, int(gs[0]), int(ws[0]))
    print("%d of %d frames packed; the serial mirror refuses %d of them"
          % (packed_ok, len(frames), refused))
    assert packed_ok >= 300 and 0 < refused < packed_ok


# -- 3. the stand-alone program under sanitizers -------------------------------------------
def test_standalone_subseq_check_program_under_sanitizers(tmp_path, streams):
    """csrc/bench/jpeg_subseq_check.cpp + jpeg_entropy.cpp built with
    -fsanitize=address,undefined by the host compiler and run directly (never
    loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_subseq_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "csrc", "jpeg_entropy.cpp"),
                            os.path.join(ROOT, "csrc", "bench", "jpeg_subseq_check.cpp"),
                            "-pthread", "-o", exe], capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr
                                  or "clang_rt" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtime: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe] + [streams[k][0] for k in ("r0", "partial_mcu", "noise_q75_opt",
                                                          "r2")],
                         capture_output=True, text=True, timeout=300, env=env)
    print(run.stdout[-500:], run.stderr[-3000:])
    assert run.returncode == 0 and "no fault" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
    # the fixed damaged records that test_gpu_mjpeg_subseq.py gives the kernel: clean here
    # first, with the statuses the Python-loaded serial mirror gives
    idx, _, cases = damaged_subseq_records(streams)
    big, dc_rec = dc_range_record(streams)
    for geom, group in (((46, 34, idx), cases), ((144, 128, big), {"dc_range": dc_rec})):
        files = []
        for name, bad in group.items():
            files.append(str(tmp_path / (name + ".bin")))
            bad.tofile(files[-1])
        run = subprocess.run([exe, "--records", str(geom[0]), str(geom[1])] + files,
                             capture_output=True, text=True, timeout=300, env=env)
        print(run.stdout[-2000:], run.stderr[-3000:])
        assert run.returncode == 0 and "%d scan records, no fault" % len(group) in run.stdout
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
        for name, bad in group.items():
            (_, ws), _ = both_decoders(bad, geom[2].mw, geom[2].mh, 16)
            assert "%s.bin: status %d\n" % (name, ws[0]) in run.stdout


# -- 4. arguments, decoder, factory, config on a CPU device -----------------------------------
def test_subseq_bytes_refusals(streams):
    idx, want, scans, offs = stream_case(streams, "r0")
    rec = np.full(want.size, 9, dtype=np.uint8)
    for bad in (8, 15, 24, 100, 4112, 8192, -16, 16.0, True, "64"):
        with pytest.raises(ValueError, match="subseq_bytes"):
            mjpeg.decode_scans_host(scans, offs, 2, idx.mw, idx.mh, out=rec, subseq_bytes=bad)
        with pytest.raises(ValueError, match="subseq_bytes"):
            vops.jpeg_huff(torch.from_numpy(scans), offs, 2, idx.mw, idx.mh,
                           out=torch.from_numpy(rec), subseq_bytes=bad)
        with pytest.raises(ValueError, match="subseq_bytes"):
            MjpegDecoder(CPU, entropy="gpu", subseq_bytes=bad)
    assert (rec == 9).all()
    with pytest.raises(ValueError, match="rounds must be"):
        vops.jpeg_huff(torch.from_numpy(scans), offs, 2, idx.mw, idx.mh, subseq_bytes=64,
                       rounds=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="subseq_bytes"):
        MjpegDecoder(CPU, entropy="host", subseq_bytes=64)
    with pytest.raises(ValueError, match="subseq_bytes"):
        MjpegDecoder(CPU, subseq_bytes=0)                 # entropy defaults to "host"
    # the buffer-level refusals of the emulation are the serial mirror's
    with pytest.raises(mjpeg.JpegError):
        mjpeg.decode_scans_host(scans, np.array([0, offs[1], offs[2] + 16]), 2, idx.mw, idx.mh,
                                out=rec, subseq_bytes=64)
    assert (rec == 9).all()
    # 0 is the serial path; 16 and 4096 are the ends of the range
    for S in (0, 16, 4096):
        got, status = mjpeg.decode_scans_host(scans, offs, 2, idx.mw, idx.mh, subseq_bytes=S)
        assert (got == want).all() and not status.any()


def test_cpu_decoder_with_subseq_bytes_equals_host_entropy(tmp_path):
    W, H, F = 46, 34, 3
    kw = dict(clip_length=F, height=16, width=24, dtype=torch.float32)
    for restart in (0, 2):
        path = str(tmp_path / ("v%d.mjpeg" % restart))
        mjpeg.write_mjpeg(path, noise_frames(W, H, 9, 3 + restart), quality=85,
                          restart_interval=restart)
        a = MjpegDecoder(CPU, entropy="host", **kw)
        b = MjpegDecoder(CPU, entropy="gpu", subseq_bytes=64, **kw)
        (va, _), (vb, _) = a.probe(path), b.probe(path)
        assert torch.equal(a.decode(va, [0, 5]), b.decode(vb, [0, 5]))
    assert b.subseq_bytes == 64 and MjpegDecoder(CPU, entropy="gpu", subseq_bytes=0).subseq_bytes == 0
    assert MjpegDecoder(CPU).subseq_bytes == 0
    assert MjpegDecoder(CPU, entropy="gpu").subseq_bytes == MjpegDecoder.SUBSEQ_BYTES
    # a restart-less frame only the Huffman decode can refuse raises from decode on a CPU
    # device, naming file and frame; the next clean request is served
    src = str(tmp_path / "r.mjpeg")
    mjpeg.write_mjpeg(src, noise_frames(W, H, 9, 11), quality=85, restart_interval=2)
    bad = str(tmp_path / "bad.mjpeg")
    corrupt_one_frame(src, bad, 4)
    c = MjpegDecoder(CPU, entropy="gpu", subseq_bytes=64, **kw)
    h = MjpegDecoder(CPU, **kw)
    (vc, _), (vh, _) = c.probe(bad), h.probe(bad)
    with pytest.raises(mjpeg.JpegError, match=r"bad\.mjpeg: frame 4 "):
        c.decode(vc, [3])
    assert torch.equal(c.decode(vc, [5]), h.decode(vh, [5]))


def test_make_decoder_forwards_subseq_bytes():
    dec = make_decoder("mjpeg", CPU, dtype=torch.float32,
                       decoder_args={"entropy": "gpu", "subseq_bytes": 128})
    assert isinstance(dec, MjpegDecoder) and dec.entropy == "gpu" and dec.subseq_bytes == 128
    with pytest.raises(ValueError, match="subseq_bytes"):
        make_decoder("mjpeg", CPU, decoder_args={"entropy": "gpu", "subseq_bytes": 20})
    with pytest.raises(ValueError, match="subseq_bytes"):
        make_decoder("mjpeg", CPU, decoder_args={"subseq_bytes": 64})


def test_subseq_config_loads():
    """configs/r2p1d-whole-mjpeg-gpu-subseq.json is the mjpeg-gpu config plus the key."""
    base = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-mjpeg-gpu.json")))
    path = os.path.join(ROOT, "configs", "r2p1d-whole-mjpeg-gpu-subseq.json")
    cfg = json.load(open(path))
    args = cfg["pipeline"][0]["decoder_args"]
    assert args["entropy"] == "gpu" and mjpeg.check_subseq_bytes(args["subseq_bytes"], "x") > 0
    cfg["pipeline"][0]["decoder_args"] = {"entropy": "gpu"}
    assert cfg == base
    spec = load_pipeline(path)
    assert spec.steps[0].kwargs["decoder"] == "mjpeg"
    assert spec.steps[0].kwargs["decoder_args"] == args
    dec = make_decoder("mjpeg", CPU, decoder_args=spec.steps[0].kwargs["decoder_args"])
    assert dec.subseq_bytes == args["subseq_bytes"]
