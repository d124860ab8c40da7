"""YUV4MPEG2 files: header parsing, the writer, and Y4mDecoder on the CPU.

The files are written here by plain byte concatenation (``raw_y4m``), not with
``write_y4m``, so a writer bug and a reader bug cannot cancel."""
import numpy as np
import pytest
import torch

from rnb_amd.models.r2p1d.decoder import Y4mDecoder, make_decoder
from rnb_amd.ops import video as vops
from rnb_amd.timecard import TimeCard
from rnb_amd.utils import y4m

CPU = torch.device("cpu")


def planes(W, H, frames, seed):
    """Random I420 frames: [(Y [H, W], U [H/2, W/2], V [H/2, W/2])]."""
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (H, W), dtype=np.uint8),
             rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8),
             rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)) for _ in range(frames)]


def raw_y4m(W, H, frames, tokens="F25:1 Ip A1:1 C420jpeg", markers=None):
    """The file's bytes; ``markers[i]`` replaces frame i's ``FRAME\\n``."""
    head = b"YUV4MPEG2 W%d H%d" % (W, H) + (b" " + tokens.encode() if tokens else b"") + b"\n"
    body = b""
    for i, (y, u, v) in enumerate(frames):
        body += (markers or {}).get(i, b"FRAME\n") + y.tobytes() + u.tobytes() + v.tobytes()
    return head + body


def to_nv12(frames):
    """The same pixels as NV12 [frames, H*3/2, W] (what nv12_to_clip reads)."""
    out = []
    for y, u, v in frames:
        uv = np.stack([u, v], axis=-1).reshape(u.shape[0], -1)
        out.append(np.concatenate([y, uv], axis=0))
    return torch.from_numpy(np.stack(out))


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("cs", [None, "C420", "C420jpeg", "C420mpeg2", "C420paldv"])
def test_accepted_colourspaces_parse(tmp_path, cs):
    fr = planes(46, 34, 3, 0)
    tokens = "F30000:1001 Ip A1:1" + (" " + cs if cs else "") + " XYSCSS=420JPEG"
    path = write(tmp_path, "a.y4m", raw_y4m(46, 34, fr, tokens))
    h = y4m.read_header(path)
    assert (h.width, h.height, h.fps, h.num_frames) == (46, 34, (30000, 1001), 3)
    assert h.colourspace == (cs[1:] if cs else "")
    assert h.frame_stride == 6 + 46 * 34 * 3 // 2 == 2352
    assert h.data_offset == len(raw_y4m(46, 34, [], tokens))
    assert h.frame_offset(2) == h.data_offset + 2 * 2352
    vid, n = Y4mDecoder(CPU).probe(path)
    assert (vid, n) == (0, 3)


@pytest.mark.parametrize("W,H,tokens,field", [
    (46, 34, "F25:1 C422", "'C'"),
    (46, 34, "F25:1 C420p10", "'C'"),
    (46, 34, "F25:1 C444", "'C'"),
    (46, 34, "F25:1 Cmono", "'C'"),
    (45, 34, "F25:1 C420", "'W'"),
    (46, 33, "F25:1", "'H'"),
])
def test_rejected_headers_name_file_and_field(tmp_path, W, H, tokens, field):
    fr = planes(46, 34, 2, 1)
    path = write(tmp_path, "bad.y4m", raw_y4m(W, H, fr, tokens))
    for call in (y4m.read_header, Y4mDecoder(CPU).probe):
        with pytest.raises(ValueError) as e:
            call(path)
        assert "bad.y4m" in str(e.value) and field in str(e.value)


def test_truncated_last_frame_and_frame_parameters_rejected(tmp_path):
    fr = planes(46, 34, 4, 2)
    good = raw_y4m(46, 34, fr)
    path = write(tmp_path, "cut.y4m", good[:-5])
    with pytest.raises(ValueError, match=r"cut\.y4m.*whole number.*'FRAME'"):
        Y4mDecoder(CPU).probe(path)
    # parameters in the first frame's marker: caught by the probe
    path = write(tmp_path, "p0.y4m", raw_y4m(46, 34, fr, markers={0: b"FRAME Ip\n"})[:-3])
    with pytest.raises(ValueError, match=r"p0\.y4m.*'FRAME'"):
        Y4mDecoder(CPU).probe(path)
    assert y4m.read_header(write(tmp_path, "ok.y4m", good)).num_frames == 4


def test_frame_parameters_on_a_sampled_frame_raise(tmp_path):
    """Frame 5 is ``FRAME Ip\\n`` + a payload 3 bytes short, so the file still
    holds whole frames and probes; decoding a clip over frame 5 raises, one
    that ends before it does not."""
    fr = planes(46, 34, 12, 3)
    data = b"YUV4MPEG2 W46 H34 F25:1\n"
    for i, (y, u, v) in enumerate(fr):
        payload = y.tobytes() + u.tobytes() + v.tobytes()
        data += (b"FRAME Ip\n" + payload[:-3]) if i == 5 else (b"FRAME\n" + payload)
    path = write(tmp_path, "ip.y4m", data)
    dec = Y4mDecoder(CPU, clip_length=4, dtype=torch.float32)
    vid, n = dec.probe(path)
    assert n == 12
    assert dec.decode(vid, [0]).shape == (1, 4, 112, 112, 4)
    with pytest.raises(ValueError, match=r"ip\.y4m: frame 5 .*'FRAME'"):
        dec.decode(vid, [0, 4])
    with pytest.raises(ValueError, match="outside"):
        dec.decode(vid, [9])


def test_write_y4m_is_byte_identical_to_the_hand_written_file(tmp_path):
    fr = planes(46, 34, 5, 4)
    path = tmp_path / "w.y4m"
    y4m.write_y4m(str(path), fr, fps=(25, 1))
    assert path.read_bytes() == raw_y4m(46, 34, fr, "F25:1 Ip A1:1 C420jpeg")
    with pytest.raises(ValueError):
        y4m.write_y4m(str(path), planes(46, 34, 1, 0) + planes(48, 34, 1, 0))


@pytest.mark.parametrize("crop", ["full", "center"])
def test_cpu_decode_equals_the_nv12_mirror(tmp_path, crop):
    W, H, N, F = 46, 34, 20, 8
    fr = planes(W, H, N, 5)
    path = write(tmp_path, "v.y4m", raw_y4m(W, H, fr))
    dec = Y4mDecoder(CPU, dtype=torch.float32, crop=crop)
    vid, n = dec.probe(path)
    assert n == N and dec.probe(path) == (vid, N)        # ids are per path
    starts = [0, 5, 12]                                   # the last clip ends on frame 19
    got = dec.decode(vid, starts)
    assert got.shape == (3, 8, 112, 112, 4) and got.dtype == torch.float32
    nv = to_nv12([fr[s + f] for s in starts for f in range(F)])
    box = None if crop == "full" else (6.0, 0.0, 34.0, 34.0)
    ref = vops.nv12_to_clip(nv, W, H, crop=box).view(3, 8, 112, 112, 4)
    assert torch.equal(got, ref)
    assert dec.decode(vid, []).shape == (0, 8, 112, 112, 4)
    # into a slot view, bf16 layout
    dec16 = Y4mDecoder(CPU, dtype=torch.bfloat16)
    v16, _ = dec16.probe(path)
    slot = torch.full((15, 8, 112, 112, 8), 7.0, dtype=torch.bfloat16)
    out = dec16.decode(v16, [12], out=slot[:1])
    assert out.data_ptr() == slot.data_ptr() and torch.all(slot[1:] == 7.0)
    assert torch.equal(slot[0], vops.nv12_to_clip(nv[16:], W, H, dtype=torch.bfloat16))
    with pytest.raises(KeyError):
        dec.decode(99, [0])


def test_yuv420_op_serves_interleaved_chroma_and_checks_its_arguments():
    """One op for planar and NV12 layouts; spans outside the buffer and a
    wrong ``out`` are refused."""
    W, H, F = 46, 34, 2
    fr = planes(W, H, 4, 6)
    nv = to_nv12(fr)
    buf = nv.reshape(-1)
    fb = vops.nv12_frame_bytes(W, H)
    got = vops.yuv420_to_clip(buf, [0, 2 * fb], F, W, H, fb, vops.nv12_planes(W, H), 24, 16)
    assert torch.equal(got.view(4, 16, 24, 4), vops.nv12_to_clip(nv, W, H, 24, 16))
    with pytest.raises(ValueError, match="outside"):
        vops.yuv420_to_clip(buf, [3 * fb], F, W, H, fb, vops.nv12_planes(W, H), 24, 16)
    with pytest.raises(ValueError, match="out must be"):
        vops.yuv420_to_clip(buf, [0], F, W, H, fb, vops.nv12_planes(W, H), 24, 16,
                            out=torch.empty((1, F, 16, 24, 8)))


def test_loader_with_y4m_decoder(tmp_path):
    """Two files of different resolutions: each request gets its own file's
    clips (what test_loader_with_npy_decoder checks for npy)."""
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    fa, fb = planes(46, 34, 40, 7), planes(64, 48, 30, 8)
    pa = write(tmp_path, "a.y4m", raw_y4m(46, 34, fa))
    pb = write(tmp_path, "b.y4m", raw_y4m(64, 48, fb, "F30:1"))
    loader = R2P1DLoader(CPU, decoder="y4m", num_clips_population=[2],
                         num_clips_weights=[1], seed=0, dtype="fp32",
                         decoder_args={"depth": 2})
    dec = loader.decoder
    assert isinstance(dec, Y4mDecoder) and dec.depth == 2
    va, na = dec.probe(pa)
    vb, nb = dec.probe(pb)
    assert (na, nb) == (40, 30) and va != vb
    got = dec.decode(va, [0, 8])                          # a, probed before b
    ref = vops.nv12_to_clip(to_nv12(fa[:16]), 46, 34).view(2, 8, 112, 112, 4)
    assert torch.equal(got, ref)
    tc = TimeCard(13)                                     # a tagged id: records its starts
    (frames,), _, tc = loader((None,), pb, tc)
    assert frames.shape == (2, 8, 112, 112, 4) and tc.num_clips == 2
    _, starts = tc.extra["clip_src"]
    nv = to_nv12([fb[s + f] for s in starts for f in range(8)])
    assert torch.equal(frames, vops.nv12_to_clip(nv, 64, 48).view(2, 8, 112, 112, 4))


def test_make_decoder_y4m():
    dec = make_decoder("y4m", CPU, dtype=torch.float32, decoder_args={"crop": "center"})
    assert isinstance(dec, Y4mDecoder) and dec.crop == "center"
    assert make_decoder("npy", CPU, decoder_args={"crop": "center"}) is not None
    with pytest.raises(ValueError):
        make_decoder("y4m", CPU, decoder_args={"crop": "left"})
    dec.warmup(2)                                         # needs no file
