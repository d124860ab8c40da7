"""Clips at a frame step or a target frame rate, on the CPU: the index
functions, the sampler's span and placement, the stepped decode of every
decoder against step-1 decodes of the same file, the loader keys and configs.

The oracle needs no reference implementation and is exact: frame ``f`` of a
stepped clip is, bit for bit, one frame of a step-1 decode of the same file on
the same decoder -- frame 0 of the clip that starts at that source frame, or,
in the file's last ``F - 1`` frames, the last frame of the clip that ends there.
"""
import glob
import json
import os
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

from rnb_amd.models.r2p1d.decoder import (MjpegDecoder, NpyDecoder, SyntheticDecoder,
                                          Y4mDecoder, make_decoder)
from rnb_amd.models.r2p1d.sampler import (R2P1DSampler, clip_frames, clip_span, step_of)
from rnb_amd.ops import video as vops
from rnb_amd.utils import mjpeg, y4m

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES, F = 46, 34, 40, 8
OUT_W, OUT_H = 16, 12
STEPS = [(2, 1), (5, 3), (1, 2)]
VIEW_CROP = {"short_side": 40, "views": 3}


# ------------------------------------------------------------------ shared helpers
def noise_frames(seed, frames=FRAMES, w=W, h=H):
    """Seeded 4:2:0 noise, every frame different: [(Y [h, w], U, V [h/2, w/2])]."""
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (h, w), dtype=np.uint8),
             rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
             rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)) for _ in range(frames)]


def write_files(d, restart_interval=0):
    """The 46x34, 40-frame files of these tests: (y4m at 25 fps, mjpeg, npy)."""
    ypath, mpath, npath = (os.path.join(str(d), "v." + e) for e in ("y4m", "mjpeg", "npy"))
    y4m.write_y4m(ypath, noise_frames(1), fps=(25, 1))
    mjpeg.write_mjpeg(mpath, noise_frames(2), quality=90, restart_interval=restart_interval)
    np.save(npath, np.random.default_rng(3).integers(0, 256, (FRAMES, 112, 112, 3),
                                                     dtype=np.uint8))
    return ypath, mpath, npath


def step1_frames(dec, vid, num_frames):
    """Every frame of the file by step-1 decodes: [num_frames, views, H, W, C].
    Frame ``s`` is frame 0 of the clip at ``s``, or, in the last F - 1 frames,
    the last frame of the clip that ends at ``s``."""
    nf = dec.F
    full = dec.decode(vid, list(range(num_frames - nf + 1)))
    full = full.view(num_frames - nf + 1, dec.views, *full.shape[1:])
    head = full[:, :, 0]
    tail = full[num_frames - 2 * nf + 2:, :, nf - 1]
    return torch.cat([head, tail])


def check_oracle(dec, vid, num_frames, starts, step, frames1, views=None, **kw):
    """``decode(starts, step=)`` row by row, frame by frame, against ``frames1``."""
    if views is None:
        got = dec.decode(vid, starts, step=step, **kw)
        rows = [(s, v) for s in starts for v in range(dec.views)]
    else:
        got = dec.decode(vid, starts, views=views, step=step, **kw)
        rows = list(zip(starts, views))
    assert got.shape[0] == len(rows)
    src = torch.tensor([clip_frames(s, dec.F, step) for s, _ in rows], device=got.device)
    view = torch.tensor([v for _, v in rows], device=got.device)
    assert torch.equal(got, frames1[src, view[:, None]]), (step, starts, views)
    return got


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return write_files(tmp_path_factory.mktemp("frame_step"))


# ------------------------------------------------------------------ index functions
@pytest.mark.parametrize("nf", [8, 16])
@pytest.mark.parametrize("step", [(1, 1), (2, 1), (3, 1), (5, 3), (2000, 1001), (1, 2)])
def test_index_functions_against_a_fraction_loop(step, nf):
    ratio = Fraction(*step)
    for start in (0, 3, 1000):
        want = []
        for f in range(nf):
            want.append(start + (f * ratio).__floor__())
        assert clip_frames(start, nf, step) == want
        assert clip_span(nf, step) == want[-1] - want[0] + 1
    assert clip_frames(7, nf) == list(range(7, 7 + nf)) and clip_span(nf) == nf


def test_step_of():
    assert step_of() == (1, 1) and step_of(frame_step=3) == (3, 1)
    assert step_of(fps=15, source_fps=(30000, 1001)) == (2000, 1001)
    assert step_of(fps=12.5, source_fps=(25, 1)) == (2, 1)
    assert step_of(fps="25:2", source_fps=(25, 1)) == (2, 1)
    assert step_of(fps=50, source_fps=(25, 1)) == (1, 2)
    assert step_of(fps="30000:1001", source_fps=(30000, 1001)) == (1, 1)
    assert step_of(fps=29.97, source_fps=(30000, 1001)) == \
        (lambda r: (r.numerator, r.denominator))(Fraction(30000, 1001) / Fraction("29.97"))
    for bad in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="frame_step"):
            step_of(frame_step=bad)
    for bad in (0, -3, "x", "1:0", "0:1", float("nan"), True):
        with pytest.raises(ValueError, match="fps"):
            step_of(fps=bad, source_fps=(25, 1))
    with pytest.raises(ValueError, match="source_fps"):
        step_of(fps=15)
    with pytest.raises(ValueError, match="frame_step.*fps"):
        step_of(frame_step=2, fps=15, source_fps=(25, 1))
    for bad in ((0, 1), (1, 0), (2, 4), (1.5, 1), 2):
        with pytest.raises(ValueError, match="step"):
            clip_frames(0, 8, bad)
        with pytest.raises(ValueError, match="step"):
            clip_span(8, bad)


# ------------------------------------------------------------------ sampler
def legacy_sample(rng, clip_length, length, population, weights):
    """The sampler's formula before clips had a span, kept literally."""
    num_clips = rng.choices(population, weights)[0]
    while num_clips > 0 and clip_length * num_clips > length:
        num_clips -= 1
    if num_clips == 0:
        return None
    stride = int(float(length) / num_clips)
    interval = stride - clip_length
    leniency = interval + (length - stride * num_clips)
    start = rng.randint(0, leniency)
    return [start + i * stride for i in range(num_clips)]


@pytest.mark.parametrize("seed", range(5))
def test_sampler_default_is_the_old_formula(seed):
    sampler, rng = R2P1DSampler(seed=seed), random.Random(seed)
    for length in range(8, 401):
        assert sampler.sample(length) == legacy_sample(rng, 8, length, [1, 15], [10, 1])
    assert sampler.rng.getstate() == rng.getstate()
    # an explicit span of clip_length is the default
    a, b = R2P1DSampler(seed=seed), R2P1DSampler(seed=seed)
    assert [a.sample(n) for n in range(8, 200)] == [b.sample(n, span=8) for n in range(8, 200)]


@pytest.mark.parametrize("placement", ["random", "uniform"])
@pytest.mark.parametrize("span", [15, 22, 29])
def test_sampler_fits_clips_by_span(span, placement):
    want_n = 15
    sampler = R2P1DSampler(num_clips_population=[want_n], num_clips_weights=[1], seed=span,
                           placement=placement)
    for length in range(span - 1, 20 * span + 1):
        starts = sampler.sample(length, span=span)
        n = min(want_n, length // span)        # the largest n <= want_n with span * n <= length
        if n == 0:
            assert starts is None and length < span
            continue
        assert len(starts) == n
        assert all(0 <= s and s + span <= length for s in starts)
        assert all(b - a == length // n for a, b in zip(starts, starts[1:]))
        if placement == "uniform":
            stride = length // n
            leniency = (stride - span) + (length - stride * n)
            assert starts[0] == leniency // 2


def test_sampler_placement():
    a = R2P1DSampler(num_clips_population=[5], num_clips_weights=[1], seed=1, placement="uniform")
    b = R2P1DSampler(num_clips_population=[5], num_clips_weights=[1], seed=2, placement="uniform")
    for length in (40, 75, 76, 300):
        for span in (None, 15):
            assert a.sample(length, span) == b.sample(length, span)
    # the count is drawn as before, the start is not drawn at all
    u, rng = R2P1DSampler(seed=7, placement="uniform"), random.Random(7)
    counts = [len(u.sample(300)) for _ in range(50)]
    assert counts == [rng.choices([1, 15], [10, 1])[0] for _ in range(50)]
    assert u.rng.getstate() == rng.getstate()
    with pytest.raises(ValueError, match="placement"):
        R2P1DSampler(placement="centre")


# ------------------------------------------------------------------ file decoders
def file_decoder(kind, device, filt="bilinear", crop="full", **kw):
    if kind == "npy":
        return NpyDecoder(device, clip_length=F, dtype=torch.float32)
    cls = Y4mDecoder if kind == "y4m" else MjpegDecoder
    crop = dict(crop) if isinstance(crop, dict) else crop
    return cls(device, clip_length=F, height=OUT_H, width=OUT_W, dtype=torch.float32,
               filter=filt, crop=crop, **kw)


def path_of(files, kind):
    return files[("y4m", "mjpeg", "npy").index(kind)]


CASES = [(k, f, c) for k in ("y4m", "mjpeg") for f in ("bilinear", "antialias")
         for c in ("full", VIEW_CROP)] + [("npy", "bilinear", "full")]


@pytest.mark.parametrize("kind,filt,crop", CASES,
                         ids=["%s-%s-%s" % (k, f, "full" if c == "full" else "views")
                              for k, f, c in CASES])
def test_stepped_decode_equals_step1_frames(files, kind, filt, crop):
    dec = file_decoder(kind, CPU, filt, crop)
    path = path_of(files, kind)
    vid, n = dec.probe(path)
    assert n == FRAMES
    frames1 = step1_frames(dec, vid, n)
    assert not any(torch.equal(frames1[i], frames1[i + 1]) for i in range(n - 1))
    for step in STEPS:
        span = clip_span(F, step)
        starts = [0, 3, FRAMES - span]
        got = check_oracle(dec, vid, n, starts, step, frames1)
        assert got.shape[0] == 3 * dec.views
        if dec.views == 3:
            check_oracle(dec, vid, n, starts, step, frames1, views=[2, 0, 1])
        # into a slot
        slot = torch.full((got.shape[0] + 1,) + tuple(got.shape[1:]), 7.0)
        assert dec.decode(vid, starts, out=slot[:-1], step=step).data_ptr() == slot.data_ptr()
        assert torch.equal(slot[:-1], got) and torch.all(slot[-1] == 7.0)
        for s in (FRAMES - span + 1, -1):
            with pytest.raises(ValueError, match=r"v\.%s.*span %d at step %d/%d"
                               % (kind, span, step[0], step[1])):
                dec.decode(vid, [0, s], step=step)
    # step (1, 1) is the default's bytes
    assert torch.equal(dec.decode(vid, [0, 5], step=(1, 1)), dec.decode(vid, [0, 5]))


def test_y4m_stepped_staging_and_frame_markers(files, tmp_path, monkeypatch):
    from rnb_amd.models.r2p1d import decoder as dmod
    dec = file_decoder("y4m", CPU, crop=VIEW_CROP)
    vid, n = dec.probe(files[0])
    hdr = dec._videos[vid][1]
    calls = []
    real = vops.yuv420_to_clip

    def clip(buf, offsets, *a, **kw):
        calls.append((int(buf.numel()), list(offsets)))
        return real(buf, offsets, *a, **kw)
    monkeypatch.setattr(dmod.vops, "yuv420_to_clip", clip)
    dec.decode(vid, [0, 9], step=(5, 3))
    # one launch over n * F * frame_stride staged bytes, clips F * frame_stride apart
    assert calls == [(2 * F * hdr.frame_stride, [0] * 3 + [F * hdr.frame_stride] * 3)]
    monkeypatch.undo()

    # frame 5 carries frame parameters: a clip that selects it raises, one that steps over it does not
    bad = str(tmp_path / "bad.y4m")
    raw = bytearray(open(files[0], "rb").read())
    a = hdr.frame_offset(5)
    raw[a:a + 9] = b"FRAME Ip\n"
    open(bad, "wb").write(bytes(raw))
    dec = file_decoder("y4m", CPU)
    vid, n = dec.probe(bad)
    assert n == FRAMES
    assert dec.decode(vid, [0], step=(2, 1)).shape[0] == 1       # 0 2 4 6 ...
    assert dec.decode(vid, [6], step=(5, 3)).shape[0] == 1
    for start, step in ((1, (2, 1)), (5, (2, 1)), (2, (5, 3)), (5, (1, 2)), (4, (1, 2))):
        assert 5 in clip_frames(start, F, step)
        with pytest.raises(ValueError, match=r"bad\.y4m: frame 5 does not start"):
            dec.decode(vid, [start], step=step)


@pytest.mark.parametrize("subseq", [0, 48])
def test_mjpeg_error_names_the_source_frame(files, tmp_path, subseq):
    """A scan the Huffman decode cannot finish: the error of a stepped request
    names the frame of the file, not its place in the clip."""
    idx = mjpeg.read_index(files[1])
    raw = bytearray(open(files[1], "rb").read())
    end = int(idx.offsets[5] + idx.lengths[5])
    raw[end - 40:end - 2] = bytes([0x55]) * 38               # frame 5's scan, before its EOI
    bad = str(tmp_path / "bad.mjpeg")
    open(bad, "wb").write(bytes(raw))
    dec = file_decoder("mjpeg", CPU, entropy="gpu", subseq_bytes=subseq)
    vid, n = dec.probe(bad)
    assert n == FRAMES
    assert dec.decode(vid, [0], step=(2, 1)).shape[0] == 1   # steps over frame 5
    for start, step in ((1, (2, 1)), (2, (5, 3)), (4, (1, 2))):
        assert 5 in clip_frames(start, F, step) and clip_frames(start, F, step)[0] != 5
        with pytest.raises(mjpeg.JpegError, match=r"bad\.mjpeg: frame 5 is not read"):
            dec.decode(vid, [0, start], step=step)


def test_source_fps_of(files, tmp_path):
    ypath, mpath, npath = files
    dec = Y4mDecoder(CPU)
    assert dec.source_fps_of(dec.probe(ypath)[0]) == (25, 1)
    ntsc, none = str(tmp_path / "ntsc.y4m"), str(tmp_path / "none.y4m")
    y4m.write_y4m(ntsc, noise_frames(4, 2), fps=(30000, 1001))
    y4m.write_y4m(none, noise_frames(4, 2), fps=(0, 0))
    assert dec.source_fps_of(dec.probe(ntsc)[0]) == (30000, 1001)
    assert dec.source_fps_of(dec.probe(none)[0]) is None
    for make, path in ((lambda **kw: MjpegDecoder(CPU, **kw), mpath),
                       (lambda **kw: NpyDecoder(CPU, **kw), npath),
                       (lambda **kw: SyntheticDecoder(CPU, **kw), "synthetic://3?frames=50")):
        d = make()
        assert d.source_fps_of(d.probe(path)[0]) is None
        for given, want in ((30, (30, 1)), ("30000:1001", (30000, 1001)), (12.5, (25, 2))):
            d = make(source_fps=given)
            assert d.source_fps_of(d.probe(path)[0]) == want
        with pytest.raises(ValueError, match="source_fps"):
            make(source_fps=0)
    for backend in ("synthetic", "synthetic-rgb", "npy", "mjpeg", "y4m"):
        d = make_decoder(backend, CPU, dtype=torch.float32, decoder_args={"source_fps": "24:1"})
        assert d.source_fps == (24, 1)
    assert "source_fps" in make_decoder.__doc__


# ------------------------------------------------------------------ synthetic mirrors
@pytest.mark.parametrize("step", [(1, 1)] + STEPS)
def test_synthetic_mirrors(step):
    starts = [0, 5, 40]
    rgb = vops.clipgen_video(9, starts, F, 16, 16, CPU, step=step)
    nv = vops.nv12gen(9, starts, F, 8, 16, CPU, step=step)
    assert rgb.shape == (3, F, 16, 16, 3) and nv.shape == (3 * F, 12, 16)
    for i, s in enumerate(starts):
        for f, src in enumerate(clip_frames(s, F, step)):
            assert torch.equal(rgb[i, f], vops.clipgen_video(9, [src], F, 16, 16, CPU)[0, 0])
            assert torch.equal(nv[i * F + f], vops.nv12gen(9, [src], F, 8, 16, CPU)[0])
    out = torch.zeros_like(nv)
    assert vops.nv12gen(9, starts, F, 8, 16, CPU, out=out, step=step) is out
    assert torch.equal(out, nv)
    for source in ("nv12", "rgb"):
        dec = SyntheticDecoder(CPU, dtype=torch.float32, source=source, src_width=16,
                               src_height=8, height=16, width=16)
        got = dec.decode(9, starts, step=step)
        for i, s in enumerate(starts):
            for f, src in enumerate(clip_frames(s, F, step)):
                assert torch.equal(got[i, f], dec.decode(9, [src])[0, 0])


# ------------------------------------------------------------------ loader
def make_loader(decoder="y4m", clips=3, seed=0, **kw):
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    return R2P1DLoader(CPU, decoder=decoder, num_clips_population=[clips], num_clips_weights=[1],
                       seed=seed, dtype="fp32", warmup=0, **kw)


def test_loader_fps_gives_the_step(files, tmp_path):
    from rnb_amd.timecard import TimeCard
    ypath, mpath, _ = files
    loader = make_loader(fps=12.5)
    (frames,), _, tc = loader((None,), ypath, TimeCard(0))
    vid, starts = tc.extra["clip_src"]
    assert tc.extra["clip_step"] == (2, 1)
    assert frames.shape[0] == 2 == tc.num_clips               # 40 frames hold two spans of 15
    assert all(s + 15 <= FRAMES for s in starts)
    assert torch.equal(frames, loader.decoder.decode(vid, starts, step=(2, 1)))
    assert not torch.equal(frames, loader.decoder.decode(vid, starts))
    # a step-1 call carries no clip_step
    plain = make_loader()
    (frames,), _, tc = plain((None,), ypath, TimeCard(0))
    assert "clip_step" not in tc.extra and len(tc.extra["clip_src"]) == 2
    assert torch.equal(frames, plain.decoder.decode(*tc.extra["clip_src"]))
    same = make_loader(fps=25)                                # the file's own rate
    (again,), _, tc = same((None,), ypath, TimeCard(0))
    assert "clip_step" not in tc.extra and torch.equal(again, frames)
    # files without a rate
    none = str(tmp_path / "none.y4m")
    y4m.write_y4m(none, noise_frames(4, 20), fps=(0, 0))
    with pytest.raises(ValueError, match=r"none\.y4m.*'F'.*source_fps"):
        make_loader(fps=12.5)((None,), none, TimeCard(0))
    with pytest.raises(ValueError, match=r"v\.mjpeg.*source_fps"):
        make_loader("mjpeg", fps=12.5)((None,), mpath, TimeCard(0))
    ok = make_loader("mjpeg", fps=12.5, decoder_args={"source_fps": 25})
    (frames,), _, tc = ok((None,), mpath, TimeCard(0))
    assert tc.extra["clip_step"] == (2, 1)
    assert torch.equal(frames, ok.decoder.decode(*tc.extra["clip_src"], step=(2, 1)))


def test_loader_segments_with_views_and_a_step(files):
    from rnb_amd.control import segment_bounds
    from rnb_amd.timecard import TimeCard
    loader = make_loader(frame_step=2, placement="uniform", crop={"short_side": 112, "views": 3},
                         clips=2, max_clips=45)
    big = os.path.join(os.path.dirname(files[0]), "big.y4m")
    y4m.write_y4m(big, noise_frames(5, FRAMES, 160, 120))
    outs = [(torch.full((6, 8, 112, 112, 4), 9.0),) for _ in range(2)]
    rows, _, tc = loader.call_into_segments((None,), big, TimeCard(0), outs)
    assert rows == [b - a for a, b in (segment_bounds(6, 2, k) for k in range(2))] == [3, 3]
    vid, starts = tc.extra["clip_src"]
    assert tc.extra["clip_step"] == (2, 1) and tc.num_clips == 6
    assert starts[0::3] == [2, 22]                # stride 20, leniency 5 + 0: centred at 2
    whole = loader.decoder.decode(vid, starts[0::3], step=(2, 1))
    assert torch.equal(torch.cat([o[0][:r] for o, r in zip(outs, rows)]), whole)
    assert all(torch.all(o[0][r:] == 9.0) for o, r in zip(outs, rows))
    # one view: the other branch
    one = make_loader(frame_step=2, placement="uniform", clips=2)
    outs = [(torch.full((2, 8, 112, 112, 4), 9.0),) for _ in range(2)]
    rows, _, tc = one.call_into_segments((None,), big, TimeCard(0), outs)
    assert rows == [1, 1]
    whole = one.decoder.decode(*tc.extra["clip_src"], step=(2, 1))
    assert torch.equal(torch.cat([o[0][:r] for o, r in zip(outs, rows)]), whole)
    # call_into writes the slot
    slot = (torch.full((3, 8, 112, 112, 4), 9.0),)
    (frames,), _, tc = one.call_into((None,), big, TimeCard(0), slot)
    assert frames.data_ptr() == slot[0].data_ptr() and torch.equal(slot[0][:2], whole)


def test_single_step_feeds_the_loaders_clips():
    from rnb_amd.models.r2p1d.model import R2P1DSingleStep
    from rnb_amd.timecard import TimeCard
    single = R2P1DSingleStep(CPU, depth=10, num_clips_population=[3], num_clips_weights=[1],
                             seed=1, warmup=0, frame_step=2)
    fed = []

    class Runner:                         # keeps what the step feeds its network
        engine = None

        def __call__(self, tensors, non_tensors, time_card):
            fed.append(tensors[0])
            return (torch.zeros(tensors[0].shape[0], 400),), None, time_card
    single.runner = Runner()
    path = "synthetic://4?frames=100"
    (logits,), _, tc = single(None, path, TimeCard(1))
    assert logits.shape == (3, 400) and tc.num_clips == 3
    loader = make_loader("synthetic", seed=1, frame_step=2)
    assert torch.equal(fed[0], loader.load(path))
    sampler = R2P1DSampler(num_clips_population=[3], num_clips_weights=[1], seed=1)
    starts = sampler.sample(100, span=15)
    assert torch.equal(fed[0], loader.decoder.decode(4, starts, step=(2, 1)))
    assert not torch.equal(fed[0], loader.decoder.decode(4, starts))


def test_bad_arguments_name_their_key():
    from rnb_amd.models.r2p1d.model import R2P1DLoader, R2P1DSingleStep
    cases = [({"frame_step": 0}, "frame_step"), ({"frame_step": 1.5}, "frame_step"),
             ({"frame_step": "2"}, "frame_step"), ({"frame_step": True}, "frame_step"),
             ({"fps": 0}, "fps"), ({"fps": -15}, "fps"), ({"fps": "fast"}, "fps"),
             ({"fps": "15:0"}, "fps"), ({"frame_step": 2, "fps": 15}, "frame_step.*fps"),
             ({"placement": "centre"}, "placement"), ({"placement": None}, "placement")]
    for kw, key in cases:
        with pytest.raises(ValueError, match=key):
            R2P1DLoader(CPU, warmup=0, **kw)
    with pytest.raises(ValueError, match="frame_step"):
        R2P1DSingleStep(CPU, depth=10, warmup=0, frame_step=0)
    ok = R2P1DLoader(CPU, warmup=0, frame_step=1, fps="30000:1001", placement="uniform")
    assert ok.fps == Fraction(30000, 1001) and ok.sampler.placement == "uniform"


def test_numerics_samples_keep_the_step(tmp_path):
    from rnb_amd.numerics import write_sample
    write_sample(str(tmp_path), 3, "runner", 7, [0, 20], np.zeros((2, 400)), "batch", "fp32",
                 step=(2, 1))
    write_sample(str(tmp_path), 4, "runner", 7, [0, 20], np.zeros((2, 400)), "batch", "fp32")
    got = {os.path.basename(f).split("_")[1]: tuple(int(v) for v in np.load(f)["step"])
           for f in glob.glob(str(tmp_path / "*.npz"))}
    assert got == {"v3": (2, 1), "v4": (1, 1)}


# ------------------------------------------------------------------ configs
def test_configs_with_the_new_keys_load_and_construct():
    from rnb_amd.config import load_pipeline
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    seen = []
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*.json"))):
        defaults = json.load(open(path)).get("defaults", {})
        if not {"frame_step", "fps", "placement"} & set(defaults):
            continue
        seen.append(os.path.basename(path))
        spec = load_pipeline(path)
        kwargs = dict(spec.steps[0].groups[0].kwargs)
        assert spec.steps[0].model.endswith("R2P1DLoader")
        assert kwargs["frame_step"] == defaults.get("frame_step", 1)
        kwargs.pop("warmup", None)
        loader = R2P1DLoader(CPU, warmup=0, **kwargs)
        assert loader.frame_step == kwargs.get("frame_step", 1)
        assert loader.sampler.placement == kwargs.get("placement", "random")
    assert "r2p1d-whole-y4m-3crop-eval.json" in seen
    assert "r2p1d-whole-mjpeg-3crop-eval.json" in seen
