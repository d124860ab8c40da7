"""jpeg_huff_subseq_kernel (csrc/jpeg_huff.hip) on the GPU: restart-less scans
decoded by synchronised subsequences give the serial host decoder's records
and the host emulation's round counts, byte for byte and for S = 16, 64 and
256; frames with restart markers pass through unchanged; the fixed damaged
records (each run under the sanitizer program on the host first,
tests/test_mjpeg_subseq_cpu.py) give the serial mirror's status and records;
the launcher's refusals; and MjpegDecoder(entropy="gpu", subseq_bytes=64)
with its deferred errors."""
import numpy as np
import pytest
import torch

from rnb_amd.models.r2p1d.decoder import MjpegDecoder
from rnb_amd.ops import native
from rnb_amd.ops import video as vops
from rnb_amd.utils import mjpeg
from test_mjpeg_cpu import noise_frames
from test_mjpeg_subseq_cpu import (SIZES, STREAMS, build_streams, check_rounds,
                                   damaged_subseq_records, dc_range_record, stream_case)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    return build_streams(tmp_path_factory.mktemp("subseq_gpu"))


@pytest.mark.parametrize("name", STREAMS)
def test_subseq_kernel_records_and_rounds_equal_the_host(streams, name):
    """Serial host records == emulation records == GPU records, status 0, GPU
    rounds == emulation rounds inside their bounds, nothing written behind the
    last record: one launch per S."""
    idx, want, scans, offs = stream_case(streams, name)
    n = idx.num_frames
    scans_dev = torch.from_numpy(scans).to(DEV)
    for S in SIZES:
        emu, emu_status, emu_rounds = mjpeg.decode_scans_host(scans, offs, n, idx.mw, idx.mh,
                                                              subseq_bytes=S, return_rounds=True)
        assert (emu == want).all() and not emu_status.any()
        rec = torch.full((want.size + 16,), 0x5A, dtype=torch.uint8, device=DEV)
        rounds = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        got, status = vops.jpeg_huff(scans_dev, offs, n, idx.mw, idx.mh, out=rec, subseq_bytes=S,
                                     rounds=rounds)
        torch.cuda.synchronize()
        print(name, "S = %d: rounds %s (emulation %s)" % (S, rounds.tolist(), emu_rounds.tolist()))
        assert status.tolist() == [0] * n, (name, S)
        assert got.data_ptr() == rec.data_ptr() and got.numel() == want.size
        assert (got.cpu().numpy() == want).all(), (name, S)
        assert torch.all(rec[want.size:] == 0x5A)         # the 16 guard bytes
        assert rounds.tolist() == emu_rounds.tolist(), (name, S)
        check_rounds(name, S, idx, scans, offs, rounds.tolist())


@pytest.mark.parametrize("S", [16, 128])
def test_damaged_records_equal_the_serial_mirror(streams, S):
    """The fixed damage list on the restart-less r0 frame plus the clean
    record, all in ONE launch, one frame each; then the hand-built record
    whose luma predictor leaves int16 (144x128, a launch of its own). Status
    and every record byte equal decode_scans_host(subseq_bytes=0)."""
    idx, clean, cases = damaged_subseq_records(streams)
    names = ["clean"] + sorted(cases)
    recs = [clean] + [cases[k] for k in names[1:]]
    scans = np.concatenate(recs)
    offs = np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
    want, want_status = mjpeg.decode_scans_host(scans, offs, len(recs), idx.mw, idx.mh)
    big, dc_rec = dc_range_record(streams)
    dc_offs = np.array([0, dc_rec.size], dtype=np.int64)
    dc_want, dc_status = mjpeg.decode_scans_host(dc_rec, dc_offs, 1, big.mw, big.mh)
    assert want_status[0] == 0 and mjpeg.status_field(int(dc_status[0])) == "dc_range"
    assert (want_status < 0).sum() + 1 >= 8               # on the serial result alone
    got, status = vops.jpeg_huff(torch.from_numpy(scans).to(DEV), offs, len(recs), idx.mw, idx.mh,
                                 subseq_bytes=S)
    dc_got, dc_st = vops.jpeg_huff(torch.from_numpy(dc_rec).to(DEV), dc_offs, 1, big.mw, big.mh,
                                   subseq_bytes=S)
    torch.cuda.synchronize()
    print(dict(zip(names, status.tolist())), dc_st.tolist())
    assert status.tolist() == want_status.tolist()
    got = got.cpu().numpy().reshape(len(recs), -1)
    want = want.reshape(len(recs), -1)
    for k, name in enumerate(names):
        assert (got[k] == want[k]).all(), name
    assert dc_st.tolist() == dc_status.tolist() and (dc_got.cpu().numpy() == dc_want).all()


def test_subseq_launcher_refusals(streams):
    """A bad subseq_bytes, a missing rounds buffer and rnb_jpeg_huff's contract
    violations launch nothing: records, status and rounds stay pre-filled."""
    idx, want, scans_np, offs = stream_case(streams, "r0")
    mw, mh, rb = idx.mw, idx.mh, idx.record_bytes
    n = scans_np.size
    scans = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
    scans[:n] = torch.from_numpy(scans_np).to(DEV)
    offs_dev = torch.from_numpy(offs).to(DEV)
    rec = torch.full((2 * rb,), 9, dtype=torch.uint8, device=DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    rounds = torch.full((2,), 55, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def launch(S=64, s=None, o=None, out=None, geom=(mw, mh), record_bytes=rb, rounds_ptr=None):
        s = scans[:n] if s is None else s
        out = rec if out is None else out
        native.kernels().jpeg_huff_subseq(
            s.data_ptr(), s.numel(), offs if o is None else o, offs_dev.data_ptr(), 2, geom[0],
            geom[1], out.data_ptr(), out.numel(), record_bytes, status.data_ptr(), S,
            rounds.data_ptr() if rounds_ptr is None else rounds_ptr, stream)
    past = offs.copy()
    past[2] += 16
    odd = offs.copy()
    odd[1] += 8
    for kw in (dict(S=0), dict(S=8), dict(S=15), dict(S=24), dict(S=72), dict(S=4112),
               dict(S=8192), dict(S=-16),                 # subseq_bytes
               dict(rounds_ptr=0), dict(rounds_ptr=rounds.data_ptr() + 2),
               dict(o=past), dict(s=scans[:n - 16]), dict(o=odd), dict(s=scans[8:n + 8]),
               dict(out=rec[:2 * rb - 16]), dict(out=rec[8:]), dict(geom=(mw + 1, mh)),
               dict(record_bytes=rb - 16)):
        with pytest.raises(RuntimeError, match="contract"):
            launch(**kw)
    for bad in (8, 24, 4112):                             # the op refuses before the launcher
        with pytest.raises(ValueError, match="subseq_bytes"):
            vops.jpeg_huff(scans[:n], offs, 2, mw, mh, out=rec, status=status, subseq_bytes=bad)
    with pytest.raises(ValueError, match="rounds must be"):
        vops.jpeg_huff(scans[:n], offs, 2, mw, mh, out=rec, status=status, subseq_bytes=64,
                       rounds=rounds.cpu())
    torch.cuda.synchronize()
    assert torch.all(rec == 9) and torch.all(status == 77) and torch.all(rounds == 55)
    launch()
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and (rec.cpu().numpy() == want).all()
    assert rounds.min() >= 1


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("subseq_dec")
    plain, marked = str(d / "plain.mjpeg"), str(d / "marked.mjpeg")
    mjpeg.write_mjpeg(plain, noise_frames(64, 48, 24, 12), quality=70)
    mjpeg.write_mjpeg(marked, noise_frames(64, 48, 24, 13), quality=70, restart_interval=2)
    return plain, marked


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decoder_with_subseq_bytes_equals_host_entropy(files, dtype):
    """A restart-less and a restart-2 stream through a ring of depth 2 over 6
    back-to-back requests: every clip equals the host-entropy decoder's."""
    host = MjpegDecoder(DEV, dtype=dtype)
    dec = MjpegDecoder(DEV, dtype=dtype, depth=2, entropy="gpu", subseq_bytes=64)
    assert dec.subseq_bytes == 64
    vids = [dec.probe(p)[0] for p in files]
    hids = [host.probe(p)[0] for p in files]
    reqs = [(k % 2, [k, 8 + k]) for k in range(6)]
    outs = torch.zeros((6, 2, 8, 112, 112, 4 if dtype == torch.float32 else 8), dtype=dtype,
                       device=DEV)
    for k, (f, starts) in enumerate(reqs):
        dec.decode(vids[f], starts, out=outs[k])
    assert len(dec._ring) == 2
    dec.drain()
    for k, (f, starts) in enumerate(reqs):
        assert torch.equal(host.decode(hids[f], starts), outs[k]), k


def test_decoder_with_subseq_bytes_defers_huffman_errors(files, tmp_path):
    """One corrupted entropy byte in frame 12 of a restart-less stream: decode
    returns, drain() raises naming file and frame, the next clean request is
    served."""
    bad = str(tmp_path / "bad.mjpeg")
    data = np.fromfile(files[0], dtype=np.uint8)
    idx = mjpeg.read_index(files[0])
    a, n = int(idx.offsets[12]), int(idx.lengths[12])
    rec = np.zeros(idx.record_bytes, dtype=np.uint8)
    out = np.zeros(mjpeg.scan_record_bound(idx.mw, idx.mh, n), dtype=np.uint8)
    j = native.jpeg()
    for back in range(40, 400):                           # the first byte that only Huffman refuses
        trial = data.copy()
        trial[a + n - back] ^= 0x55
        if 0xFF in (int(trial[a + n - back]), int(data[a + n - back])):
            continue
        if j.pack_scans(trial, [a], [n], out)[0] > 0 and \
                j.decode_frames_rc(trial, [a], [n], rec, rec.size) < 0:
            trial.tofile(bad)
            break
    else:
        raise AssertionError("no byte of the scan makes the Huffman decode fail")
    host = MjpegDecoder(DEV, dtype=torch.float32)
    dec = MjpegDecoder(DEV, dtype=torch.float32, depth=2, entropy="gpu", subseq_bytes=64)
    vbad, _ = dec.probe(bad)
    vok, _ = host.probe(files[0])
    got = dec.decode(vbad, [0, 8])                        # frames 8..15 hold the bad one
    assert got.shape == (2, 8, 112, 112, 4)
    with pytest.raises(mjpeg.JpegError, match=r"bad\.mjpeg: frame 12 ") as e:
        dec.drain()
    assert e.value.field in ("huffman", "run", "truncated", "dc_range")
    assert torch.equal(got[0], host.decode(vok, [0])[0])  # the clean clip of that request
    dec.drain()                                           # cleared
    assert torch.equal(dec.decode(vbad, [16]), host.decode(vok, [16]))
