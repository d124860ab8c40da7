"""Clips at a frame step on the GPU: the stepped generator kernels against
their CPU mirrors and the unchanged entry points, and every decoder's stepped
decode against step-1 decodes of the same file on the same decoder (the exact
per-frame oracle of test_frame_step_cpu.py)."""
import pytest
import torch

from rnb_amd.models.r2p1d.decoder import MjpegDecoder, SyntheticDecoder, Y4mDecoder
from rnb_amd.models.r2p1d.sampler import clip_frames
from rnb_amd.ops import video as vops
from test_frame_step_cpu import (F, FRAMES, OUT_H, OUT_W, VIEW_CROP, check_oracle, step1_frames,
                                 write_files)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
GEN_STEPS = [(1, 1), (2, 1), (5, 3), (1, 2)]
STARTS = [0, 5, 40]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(y4m, mjpeg without restart markers, mjpeg with them)."""
    plain = write_files(tmp_path_factory.mktemp("frame_step_gpu"))
    rst = write_files(tmp_path_factory.mktemp("frame_step_gpu_rst"), restart_interval=2)
    return plain[0], plain[1], rst[1]


# ------------------------------------------------------------------ generator kernels
@pytest.mark.parametrize("step", GEN_STEPS)
def test_generator_kernels_match_their_mirrors(step):
    rgb = vops.clipgen_video(9, STARTS, F, 16, 16, DEV, step=step)
    nv = vops.nv12gen(9, STARTS, F, 8, 16, DEV, step=step)
    torch.cuda.synchronize()
    assert rgb.dtype == torch.uint8 and rgb.shape == (3, F, 16, 16, 3)
    assert nv.dtype == torch.uint8 and nv.shape == (3 * F, 12, 16)
    assert torch.equal(rgb.cpu(), vops.clipgen_video(9, STARTS, F, 16, 16, CPU, step=step))
    assert torch.equal(nv.cpu(), vops.nv12gen(9, STARTS, F, 8, 16, CPU, step=step))


def test_step_entry_points_at_1_1_equal_the_old_ones():
    from rnb_amd.ops.native import kernels
    stream = torch.cuda.current_stream(DEV).cuda_stream
    old = torch.zeros((3, F, 16, 16, 3), dtype=torch.uint8, device=DEV)
    new = torch.ones_like(old)
    kernels().clipgen_video(old.data_ptr(), 9, STARTS, F, 16, 16, stream)
    kernels().clipgen_video_step(new.data_ptr(), 9, STARTS, F, 16, 16, (1, 1), stream)
    assert torch.equal(old, new)
    assert torch.equal(old, vops.clipgen_video(9, STARTS, F, 16, 16, DEV))
    old = torch.zeros((3 * F, 12, 16), dtype=torch.uint8, device=DEV)
    new = torch.ones_like(old)
    kernels().nv12gen_video(old.data_ptr(), 9, STARTS, F, 8, 16, stream)
    kernels().nv12gen_video_step(new.data_ptr(), 9, STARTS, F, 8, 16, (1, 1), stream)
    assert torch.equal(old, new)
    assert torch.equal(old, vops.nv12gen(9, STARTS, F, 8, 16, DEV))
    # the device-array forms are untouched
    vids = torch.full((3,), 9, dtype=torch.int32, device=DEV)
    st = torch.tensor(STARTS, dtype=torch.int32, device=DEV)
    assert torch.equal(old, vops.nv12gen(vids, st, F, 8, 16, DEV))


def test_launchers_refuse_a_bad_step_and_split_many_clips():
    from rnb_amd.ops.native import kernels
    stream = torch.cuda.current_stream(DEV).cuda_stream
    out = torch.zeros((1, F, 16, 16, 3), dtype=torch.uint8, device=DEV)
    for nf, step in ((F, (0, 1)), (F, (1, 0)), (F, (-2, 1)), (65536, (1, 1)),
                     (65535, (40000, 1))):
        for launch in (kernels().clipgen_video_step, kernels().nv12gen_video_step):
            with pytest.raises(RuntimeError, match="code -2"):
                launch(out.data_ptr(), 9, [0], nf, 16, 16, step, stream)
    torch.cuda.synchronize()
    assert not out.any()                                    # nothing was launched
    # more clips than one launch's arguments hold
    starts = list(range(0, 70, 2))
    assert len(starts) > 32
    rgb = vops.clipgen_video(3, starts, F, 16, 16, DEV, step=(5, 3))
    nv = vops.nv12gen(3, starts, F, 8, 16, DEV, step=(5, 3))
    assert torch.equal(rgb.cpu(), vops.clipgen_video(3, starts, F, 16, 16, CPU, step=(5, 3)))
    assert torch.equal(nv.cpu(), vops.nv12gen(3, starts, F, 8, 16, CPU, step=(5, 3)))


@pytest.mark.parametrize("source", ["nv12", "rgb"])
def test_synthetic_decoder_frames(source):
    dec = SyntheticDecoder(DEV, dtype=torch.float32, source=source)
    for step in GEN_STEPS[1:]:
        got = dec.decode(9, STARTS, step=step)
        src = [fr for s in STARTS for fr in clip_frames(s, F, step)]
        want = torch.stack([dec.decode(9, [fr])[0, 0] for fr in sorted(set(src))])
        index = torch.tensor([sorted(set(src)).index(fr) for fr in src], device=DEV)
        assert torch.equal(got.view(len(src), *got.shape[2:]), want[index]), step
    assert torch.equal(dec.decode(9, STARTS, step=(1, 1)), dec.decode(9, STARTS))


# ------------------------------------------------------------------ file decoders
MODES = [("y4m", Y4mDecoder, 0, {}), ("mjpeg_host", MjpegDecoder, 1, {"entropy": "host"}),
         ("mjpeg_gpu", MjpegDecoder, 2, {"entropy": "gpu", "subseq_bytes": 0}),
         ("mjpeg_subseq", MjpegDecoder, 1, {"entropy": "gpu", "subseq_bytes": 48})]


@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("filt", ["bilinear", "antialias"])
@pytest.mark.parametrize("mode", [m[0] for m in MODES])
def test_file_decoders_stepped_frames(files, mode, filt, views):
    _, cls, which, args = next(m for m in MODES if m[0] == mode)
    dec = cls(DEV, clip_length=F, height=OUT_H, width=OUT_W, dtype=torch.float32, filter=filt,
              crop=dict(VIEW_CROP, views=views), **args)
    vid, n = dec.probe(files[which])
    assert n == FRAMES and dec.views == views
    frames1 = step1_frames(dec, vid, n)
    for step, span in (((2, 1), 15), ((5, 3), 12)):
        starts = [0, 3, FRAMES - span]
        check_oracle(dec, vid, n, starts, step, frames1)
        if views == 3:
            check_oracle(dec, vid, n, starts, step, frames1, views=[2, 0, 1])
    if cls is MjpegDecoder:
        dec.drain()                                         # no deferred error
    torch.cuda.synchronize()


# ------------------------------------------------------------------ loader
def test_loader_call_into_a_slot(files):
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    from rnb_amd.timecard import TimeCard
    loader = R2P1DLoader(DEV, decoder="y4m", num_clips_population=[2], num_clips_weights=[1],
                         seed=0, dtype="fp32", warmup=0, frame_step=2, placement="uniform")
    slot = (torch.full((15, 8, 112, 112, 4), 9.0, device=DEV),)
    (frames,), _, tc = loader.call_into((None,), files[0], TimeCard(0), slot)
    assert frames.data_ptr() == slot[0].data_ptr() and tc.num_clips == 2
    vid, starts = tc.extra["clip_src"]
    assert starts == [2, 22] and tc.extra["clip_step"] == (2, 1)
    want = loader.decoder.decode(vid, starts, step=(2, 1))
    torch.cuda.synchronize()
    assert torch.equal(slot[0][:2], want) and torch.all(slot[0][2:] == 9.0)
    assert not torch.equal(want, loader.decoder.decode(vid, starts))
