"""jpeg_huff_kernel (csrc/jpeg_huff.hip) on the GPU against the host entropy
decoder and the kernel's host mirror, byte for byte; the launcher's refusals; a
fixed list of damaged scan records (each run under the sanitizer program on the
host first, tests/test_mjpeg_scan_cpu.py); MjpegDecoder(entropy="gpu") with its
deferred errors; and configs/r2p1d-whole-mjpeg-gpu.json end to end."""
import json
import os

import numpy as np
import pytest
import torch

from rnb_amd.ops import video as vops
from rnb_amd.utils import mjpeg
from test_mjpeg_cpu import noise_frames, ramp_frames
from test_mjpeg_scan_cpu import (GOLDEN_STREAMS, MATRIX, build_matrix, corrupt_one_frame,
                                 damaged_scan_records, host_records, packed)
from test_pipeline_e2e import ROOT, run_cfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    return build_matrix(tmp_path_factory.mktemp("scan_gpu"))


@pytest.mark.parametrize("name", sorted(MATRIX) + sorted(GOLDEN_STREAMS))
def test_huff_kernel_records_equal_host_records(matrix, name):
    path, _ = matrix[name]
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    assert 2 <= idx.num_frames <= 3
    want = host_records(data, idx)
    scans, offs = packed(data, idx)
    rec = torch.full((idx.num_frames * idx.record_bytes + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    got, status = vops.jpeg_huff(torch.from_numpy(scans).to(DEV), offs, idx.num_frames, idx.mw,
                                 idx.mh, out=rec)
    torch.cuda.synchronize()
    assert status.tolist() == [0] * idx.num_frames
    assert got.data_ptr() == rec.data_ptr() and got.numel() == want.size
    assert (got.cpu().numpy() == want).all()
    assert torch.all(rec[want.size:] == 0x5A)             # nothing behind the last record
    # the host mirror (what a CPU tensor gets) agrees too
    m, ms = vops.jpeg_huff(torch.from_numpy(scans), offs, idx.num_frames, idx.mw, idx.mh)
    assert ms.tolist() == status.tolist() and torch.equal(m, got.cpu())


def test_jpeg_huff_launcher_refusals(matrix):
    path, _ = matrix["r2"]
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    mw, mh, rb = idx.mw, idx.mh, idx.record_bytes
    scans_np, offs = packed(data, idx)
    scans = torch.zeros(scans_np.size + 16, dtype=torch.uint8, device=DEV)
    scans[:scans_np.size] = torch.from_numpy(scans_np).to(DEV)
    n = scans_np.size
    rec = torch.full((2 * rb,), 9, dtype=torch.uint8, device=DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)

    def run(s=None, o=None, out=None, st=None, geom=(mw, mh), record_bytes=None):
        return vops.jpeg_huff(scans[:n] if s is None else s, offs if o is None else o, 2,
                              geom[0], geom[1], out=rec if out is None else out,
                              status=status if st is None else st, record_bytes=record_bytes)
    past = offs.copy()
    past[2] += 16
    negative = offs.copy()
    negative[0] = -16
    odd = offs.copy()
    odd[1] += 8
    tiny = offs.copy()
    tiny[1] = offs[0] + 1024
    for kw in (dict(o=past),                              # a scan record past the buffer
               dict(s=scans[:n - 16]),                    # ... a shorter buffer
               dict(o=negative), dict(o=tiny),            # in front of it / no room for a header
               dict(o=odd),                               # a misaligned record
               dict(s=scans[8:n + 8]),                    # misaligned scans
               dict(out=rec[:2 * rb - 16]),               # records too small
               dict(out=rec[8:]),                         # misaligned records
               dict(geom=(mw + 1, mh)),                   # a larger geometry
               dict(record_bytes=rb - 16)):               # records closer than a record
        with pytest.raises(RuntimeError, match="contract"):
            run(**kw)
    with pytest.raises(ValueError, match="out must be"):
        run(out=rec.cpu())
    with pytest.raises(ValueError, match="status must be"):
        run(st=status[:1])
    with pytest.raises(ValueError, match="offsets"):
        run(o=offs[:2])
    with pytest.raises(ValueError, match="scans must be"):
        run(s=scans[:n].view(2, -1))
    torch.cuda.synchronize()
    assert torch.all(rec == 9) and torch.all(status == 77)       # nothing was launched
    got, st = run()
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0] and (got.cpu().numpy() == host_records(data, idx)).all()


def test_damaged_scan_records_equal_the_host_mirror(matrix):
    """The fixed list of damaged records (flipped data bytes, shortened and
    inverted spans, raised table counts, a wrong header) plus the clean one:
    the host mirror first, then all of them in ONE launch, one frame each.
    Status and records equal the mirror's exactly."""
    idx, clean, cases = damaged_scan_records(matrix)
    names = ["clean"] + sorted(cases)
    recs = [clean] + [cases[k] for k in names[1:]]
    assert len({r.size for r in recs}) == 1 and 12 <= len(cases) <= 20
    scans = np.concatenate(recs)
    offs = np.arange(len(recs) + 1, dtype=np.int64) * clean.size
    want, want_status = mjpeg.decode_scans_host(scans, offs, len(recs), idx.mw, idx.mh)
    assert want_status[0] == 0 and (want_status[1:] < 0).sum() >= 11
    got, status = vops.jpeg_huff(torch.from_numpy(scans).to(DEV), offs, len(recs), idx.mw, idx.mh)
    torch.cuda.synchronize()
    print(dict(zip(names, status.tolist())))
    assert status.tolist() == want_status.tolist()
    got = got.cpu().numpy().reshape(len(recs), -1)
    want = want.reshape(len(recs), -1)
    for k, name in enumerate(names):
        assert (got[k] == want[k]).all(), name


@pytest.fixture(scope="module")
def two_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mjpeg_gpu")
    mjpeg.write_mjpeg(str(d / "a.mjpeg"), ramp_frames(46, 34, 30), quality=85, restart_interval=2)
    mjpeg.write_mjpeg(str(d / "b.mjpeg"), noise_frames(64, 48, 24, 12), quality=70)
    corrupt_one_frame(str(d / "a.mjpeg"), str(d / "bad.mjpeg"), 12)
    return str(d / "a.mjpeg"), str(d / "b.mjpeg"), str(d / "bad.mjpeg")


@pytest.mark.parametrize("crop", ["full", "center"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decoder_gpu_entropy_equals_host_entropy(two_files, dtype, crop):
    """Restart interval 2 (a.mjpeg) and 0 (b.mjpeg); the records are equal byte
    for byte, so the clips are too."""
    from rnb_amd.models.r2p1d.decoder import MjpegDecoder
    host = MjpegDecoder(DEV, dtype=dtype, crop=crop)
    gpu = MjpegDecoder(DEV, dtype=dtype, crop=crop, entropy="gpu")
    for path, starts in ((two_files[0], [0, 9, 22]), (two_files[1], [3, 16])):
        (vh, _), (vg, _) = host.probe(path), gpu.probe(path)
        a, b = host.decode(vh, starts), gpu.decode(vg, starts)
        torch.cuda.synchronize()
        assert a.shape == b.shape == (len(starts), 8, 112, 112, 4 if dtype == torch.float32 else 8)
        assert torch.equal(a, b), path
    gpu.drain()
    assert gpu.stats["requests"] == host.stats["requests"] == 2
    assert gpu.stats["uploaded_bytes"] < host.stats["uploaded_bytes"]


def test_decoder_gpu_entropy_ring_reuse_and_uploaded_bytes(two_files):
    from rnb_amd.models.r2p1d.decoder import MjpegDecoder
    host = MjpegDecoder(DEV, dtype=torch.float32)
    dec = MjpegDecoder(DEV, dtype=torch.float32, depth=2, entropy="gpu")
    va, _ = dec.probe(two_files[0])
    vb, _ = dec.probe(two_files[1])
    ha, _ = host.probe(two_files[0])
    hb, _ = host.probe(two_files[1])
    # ramp frames at 46x34: ~2.4 KB of scan record per frame against a 7296-byte record
    dec.decode(va, [0, 9])
    host.decode(ha, [0, 9])
    per_frame = dec.stats["uploaded_bytes"] / 16.0
    print("uploaded per frame: gpu entropy %.0f B, host entropy %d B"
          % (per_frame, host.stats["uploaded_bytes"] // 16))
    assert host.stats["uploaded_bytes"] == 16 * 7296
    assert 2032 < per_frame < 7296 / 2
    # 10 requests back to back on alternating files through a ring of 2, no host
    # synchronisation in between; every result equals the host-entropy decoder's
    outs = torch.zeros((10, 2, 8, 112, 112, 4), device=DEV)
    reqs = [(k % 2, [k % 7, 8 + k % 8]) for k in range(10)]
    for k, (f, starts) in enumerate(reqs):
        dec.decode((va, vb)[f], starts, out=outs[k])
    assert len(dec._ring) == 2
    dec.drain()
    for k, (f, starts) in enumerate(reqs):
        assert torch.equal(host.decode((ha, hb)[f], starts), outs[k]), k
    # a slot is written in place and nothing else
    slot = torch.full((3, 8, 112, 112, 4), 7.0, device=DEV)
    y = dec.decode(va, [3], out=slot[1:2])
    torch.cuda.synchronize()
    assert y.data_ptr() == slot[1:2].data_ptr()
    assert torch.all(slot[0] == 7.0) and torch.all(slot[2] == 7.0)
    assert torch.equal(y, host.decode(ha, [3]))


def test_decoder_gpu_entropy_defers_huffman_errors(two_files):
    """Frame 12 of bad.mjpeg passes the packer and fails in the Huffman decode:
    decode returns, drain() raises naming file and frame, and the decoder
    serves the next clean request; without drain() the entry's next
    acquisition raises."""
    from rnb_amd.models.r2p1d.decoder import MjpegDecoder
    host = MjpegDecoder(DEV, dtype=torch.float32)
    dec = MjpegDecoder(DEV, dtype=torch.float32, depth=2, entropy="gpu")
    vbad, _ = dec.probe(two_files[2])
    vok, _ = host.probe(two_files[0])
    got = dec.decode(vbad, [0, 8])                        # frames 8..15 hold the bad one
    assert got.shape == (2, 8, 112, 112, 4)
    with pytest.raises(mjpeg.JpegError, match=r"bad\.mjpeg: frame 12 ") as e:
        dec.drain()
    assert e.value.field in ("huffman", "run", "RST", "truncated", "dc_range")
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert torch.equal(got[0], host.decode(vok, [0])[0])  # the clean clip of that request
    dec.drain()                                           # cleared
    assert torch.equal(dec.decode(vbad, [16]), host.decode(vok, [16]))
    # not drained: entry 0 carries the error until request 3 acquires it again
    dec = MjpegDecoder(DEV, dtype=torch.float32, depth=2, entropy="gpu")
    vbad, _ = dec.probe(two_files[2])
    dec.decode(vbad, [10])
    dec.decode(vbad, [20])
    with pytest.raises(mjpeg.JpegError, match=r"bad\.mjpeg: frame 12 "):
        dec.decode(vbad, [0])
    assert torch.equal(dec.decode(vbad, [0]), host.decode(vok, [0]))
    dec.drain()
    # what the packer refuses still raises from decode
    cut = two_files[2] + ".cut.mjpeg"
    data = open(two_files[0], "rb").read()
    idx = mjpeg.read_index(two_files[0])
    a = int(idx.offsets[2])
    pos = a + data[a:].index(b"\xff\xd1")
    open(cut, "wb").write(data[:pos] + data[pos + 2:])    # frame 2 without its RST1
    vcut, _ = dec.probe(cut)
    with pytest.raises(mjpeg.JpegError, match=r"cut\.mjpeg: frame 2 .*'RST'"):
        dec.decode(vcut, [0])
    assert torch.equal(dec.decode(vcut, [8]), host.decode(vok, [8]))
    dec.drain()


def test_mjpeg_gpu_entropy_config_end_to_end(tmp_path):
    """configs/r2p1d-whole-mjpeg-gpu.json on a 3-file tree (64x48, 40 frames
    each, restart 0 / 3 / 12): 6 videos, bulk, in child processes."""
    root = tmp_path / "videos"
    for i in range(3):
        d = root / ("label%d" % (i % 2))
        d.mkdir(parents=True, exist_ok=True)
        mjpeg.write_mjpeg(str(d / ("v%d.mjpeg" % i)), ramp_frames(64, 48, 40, seed=20 + i),
                          quality=75, restart_interval=(0, 3, 12)[i])
    check = tmp_path / "check"
    check.mkdir()
    cfg = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-mjpeg-gpu.json")))
    assert cfg["pipeline"][0]["decoder"] == "mjpeg"
    assert cfg["pipeline"][0]["decoder_args"] == {"entropy": "gpu"}
    proc, res, _ = run_cfg(tmp_path, cfg, "-v", "6", "-mi", "0", "--set", "depth=18",
                           "--set", "warmup=1", timeout=600,
                           env={"RNB_VIDEO_ROOT": str(root), "RNB_CHECK_DIR": str(check),
                                "RNB_CHECK_EVERY": "1", "RNB_CHECK_MAX": "64"})
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert res["ok"] and res["videos_done"] >= 6, res
    samples = [np.load(f) for f in sorted(check.glob("runner_v*.npz"))]
    assert len(samples) >= 6, len(samples)
    for s in samples:
        assert 1 <= len(s["starts"]) <= 5 and s["logits"].shape == (len(s["starts"]), 400)
        assert 0 <= int(s["vid"]) < 3 and np.isfinite(s["logits"]).all()
