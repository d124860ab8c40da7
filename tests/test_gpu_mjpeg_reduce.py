"""Reduced-size MJPEG decode on the GPU: jpeg_idct_reduced_kernel /
jpeg_idct_dc_kernel against box means of the fp64 ideal IDCT and against PIL's
draft luma, reduce=1 against the full-size launch, the launcher's refusals,
MjpegDecoder(reduce=) against the CPU-device decoder in every entropy mode, the
surface regrowing, the geometry pin, and the shipped reduce config end to end."""
import json
import os

import numpy as np
import pytest
import torch

from rnb_amd.models.r2p1d.decoder import MjpegDecoder
from rnb_amd.ops import video as vops
from rnb_amd.ops.native import kernels
from rnb_amd.utils import mjpeg
from test_gpu_mjpeg import MIRROR_TOL
from test_mjpeg_cpu import GOLDEN, check_band, noise_frames, ramp_frames, records_tensor
from test_mjpeg_reduce_cpu import (ALL_GOLDEN, DRAFT_CASES, IDCT_CASES, REDUCES, geometry_pin,
                                   golden_frames, ramps, reduce_inputs, reduced_ideal_planes,
                                   reduced_luma)  # noqa: F401  (ramps: a fixture)
from test_pipeline_e2e import ROOT, run_cfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def idct_cases():
    """(W, H, sampling) -> kind -> (records [6 frames], frames), computed once."""
    return {case: {kind: (records_tensor(frames), frames)
                   for kind, frames in reduce_inputs(*case).items()} for case in IDCT_CASES}


@pytest.mark.parametrize("s", REDUCES)
@pytest.mark.parametrize("W,H,sampling", IDCT_CASES)
def test_reduced_idct_kernel_against_box_means_of_fp64(idct_cases, W, H, sampling, s):
    """6 frames, a different table on each; the band rule of check_band against
    the full-size fp64 IDCT's box means. The surface is dirtied first: the bytes
    past the frames stay, every byte of the frames is written."""
    mw, mh, rb = mjpeg.geometry(W, H, sampling)
    need = 6 * vops.jpeg_frame_bytes(mw, mh, sampling, s)[1]
    for kind, (rec, frames) in idct_cases[W, H, sampling].items():
        d = rec.to(DEV)
        surf = torch.full((need + 64,), 0xAA, dtype=torch.uint8, device=DEV)
        a = vops.jpeg_idct(d, 6, mw, mh, out=surf, sampling=sampling, reduce=s)
        assert a.data_ptr() == surf.data_ptr() and a.shape == (need,)
        first = a.cpu().numpy().copy()
        assert torch.all(surf[need:] == 0xAA)                 # nothing past the frames
        surf.fill_(0x55)
        second = vops.jpeg_idct(d, 6, mw, mh, out=surf, sampling=sampling, reduce=s).cpu().numpy()
        assert np.array_equal(first, second)                  # no stale byte survives
        assert torch.all(surf[need:] == 0x55)
        fresh = vops.jpeg_idct(d, 6, mw, mh, sampling=sampling, reduce=s).cpu().numpy()
        assert np.array_equal(first, fresh)
        check_band(first, reduced_ideal_planes(frames, mw, mh, sampling, s),
                   "%dx%d %s %s reduce %d" % (W, H, sampling, kind, s),
                   tie_only=kind == "dc_only")
        if kind == "clamp" and s < 8:
            assert (first == 0).any() and (first == 255).any()


@pytest.mark.parametrize("name,s", DRAFT_CASES)
def test_reduced_idct_kernel_luma_against_pils_draft(name, s):
    W, H = ALL_GOLDEN[name]
    lumas = np.load(os.path.join(GOLDEN, "%s_draft%d_luma.npy" % (name, s)))
    frames, (mw, mh, sampling) = golden_frames(name)
    surf = vops.jpeg_idct(records_tensor(frames).to(DEV), 2, mw, mh, sampling=sampling,
                          reduce=s).cpu().numpy()
    for i in range(2):
        d = np.abs(reduced_luma(surf, i, W, H, mw, mh, sampling, s).astype(int)
                   - lumas[i].astype(int))
        print(name, s, i, "max |kernel luma - PIL draft luma| =", d.max(), "mean", d.mean())
        assert d.max() <= 2


@pytest.mark.parametrize("W,H,sampling", IDCT_CASES)
def test_reduce_1_is_the_full_size_launch(idct_cases, W, H, sampling):
    mw, mh, _ = mjpeg.geometry(W, H, sampling)
    for kind, (rec, _) in idct_cases[W, H, sampling].items():
        d = rec.to(DEV)
        assert torch.equal(vops.jpeg_idct(d, 6, mw, mh, sampling=sampling, reduce=1),
                           vops.jpeg_idct(d, 6, mw, mh, sampling=sampling)), kind


@pytest.mark.parametrize("s", REDUCES)
def test_reduced_idct_launcher_refusals(s):
    mw, mh, rb = mjpeg.geometry(46, 34)
    fb = vops.jpeg_frame_bytes(mw, mh, "420", s)[1]
    rec = torch.zeros(3 * rb, dtype=torch.uint8, device=DEV)
    surf = torch.full((3 * fb + 16,), 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="contract"):          # records too small
        vops.jpeg_idct(rec[:3 * rb - 16], 3, mw, mh, out=surf, reduce=s)
    with pytest.raises(RuntimeError, match="contract"):          # surface too small
        vops.jpeg_idct(rec, 3, mw, mh, out=surf[:3 * fb - 1], reduce=s)
    with pytest.raises(RuntimeError, match="contract"):          # a larger geometry
        vops.jpeg_idct(rec, 3, mw + 1, mh, out=surf[:3 * fb], reduce=s)
    with pytest.raises(RuntimeError, match="contract"):          # misaligned records
        vops.jpeg_idct(rec[8:8 + 2 * rb], 2, mw, mh, out=surf, reduce=s)
    if s < 8:                                                    # a surface off its store width
        with pytest.raises(RuntimeError, match="contract"):
            vops.jpeg_idct(rec, 3, mw, mh, out=surf[1:], reduce=s)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for bad in (0, 3, 5, 16, -2):                                # the launcher's own check
        with pytest.raises(RuntimeError, match="contract"):
            kernels().jpeg_idct(rec.data_ptr(), rec.numel(), rb, 3, mw, mh, surf.data_ptr(),
                                surf.numel(), stream, sampling=0, reduce=bad)
        with pytest.raises(ValueError, match="reduce"):
            vops.jpeg_idct(rec, 3, mw, mh, out=surf, reduce=bad)
    torch.cuda.synchronize()
    assert torch.all(surf == 9)                                  # nothing was launched


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """64x48 without restart markers (the subsequence path), 46x34 with them,
    and a larger 96x80 file for the regrow."""
    d = tmp_path_factory.mktemp("reduce")
    mjpeg.write_mjpeg(str(d / "a.mjpeg"), noise_frames(64, 48, 24, 12), quality=70)
    mjpeg.write_mjpeg(str(d / "b.mjpeg"), ramp_frames(46, 34, 24), quality=85, restart_interval=2)
    mjpeg.write_mjpeg(str(d / "c.mjpeg"), ramp_frames(96, 80, 12, seed=3), quality=80)
    return str(d / "a.mjpeg"), str(d / "b.mjpeg"), str(d / "c.mjpeg")


ENTROPY = [dict(entropy="host"), dict(entropy="gpu", subseq_bytes=0),
           dict(entropy="gpu", subseq_bytes=48)]


@pytest.mark.parametrize("reduce", [2, "auto"])
@pytest.mark.parametrize("mode", ENTROPY, ids=["host", "gpu", "gpu_subseq48"])
def test_decoder_with_reduce_equals_the_cpu_device(files, mode, reduce):
    """Both streams, centre crop (bilinear) and three views (antialias), output
    16 x 12: "auto" resolves to 2 for every box here but the 46x34 views' (1)."""
    crops = (("center", "bilinear"), ({"short_side": 24, "views": 3}, "antialias"))
    for crop, filter in crops:
        kw = dict(clip_length=2, height=12, width=16, dtype=torch.float32, crop=crop,
                  filter=filter, reduce=reduce)
        dec, mirror = MjpegDecoder(DEV, **dict(kw, **mode)), MjpegDecoder(CPU, **kw)
        for path in files[:2]:
            (v, n), (vm, _) = dec.probe(path), mirror.probe(path)
            assert dec.reduce_of(v) == mirror.reduce_of(vm)
            if reduce != "auto":
                assert dec.reduce_of(v) == reduce
            starts = [0, 5, n - 2]
            got = dec.decode(v, starts)
            dec.drain()
            torch.cuda.synchronize()
            want = mirror.decode(vm, starts)
            assert got.shape == want.shape == (3 * dec.views, 2, 12, 16, 4)
            err = (got.cpu() - want).abs().max().item()
            print(os.path.basename(path), mode, crop, "reduce", dec.reduce_of(v),
                  "max |decoder - cpu device| =", err)
            assert err <= MIRROR_TOL, err
            assert torch.all(got[..., 3] == 0)
    # "auto" was 2 at least once: the reduced path ran
    assert reduce != "auto" or dec.reduce_of(dec.probe(files[0])[0]) == 2


def test_decoder_surface_regrows_for_a_larger_frame_and_another_reduce(files):
    """reduce="auto", output 16 x 12: the 46x34 file (3 x 3 MCUs) decodes at 2
    into 864-byte frames, the 96x80 file (6 x 5 MCUs) at 4 into 720-byte frames
    from records three times as large. Small file first: the ring regrows for
    the larger records, the surface does not. Large file first: the surface
    regrows for the smaller reduce, the ring does not. Every result equals the
    CPU-device decoder's and does not depend on the order."""
    kw = dict(clip_length=2, height=12, width=16, dtype=torch.float32, crop="full")
    mirror = MjpegDecoder(CPU, reduce="auto", **kw)
    mb, mc = mirror.probe(files[1])[0], mirror.probe(files[2])[0]
    want_b, want_c = mirror.decode(mb, [0, 3]), mirror.decode(mc, [1, 4])
    surf_b = 15 * 2 * vops.jpeg_frame_bytes(3, 3, "420", 2)[1]
    surf_c = 15 * 2 * vops.jpeg_frame_bytes(6, 5, "420", 4)[1]
    assert surf_b == 15 * 2 * 864 and surf_c == 15 * 2 * 720
    dec = MjpegDecoder(DEV, depth=2, reduce="auto", **kw)
    vb, vc = dec.probe(files[1])[0], dec.probe(files[2])[0]
    assert (dec.reduce_of(vb), dec.reduce_of(vc)) == (2, 4)
    first = dec.decode(vb, [0, 3])
    small_ring = dec._ring_bytes
    assert dec._surface.numel() == surf_b
    second = dec.decode(vc, [1, 4])
    assert dec._ring_bytes > small_ring and len(dec._ring) == 2
    assert dec._surface.numel() == surf_b
    third = dec.decode(vb, [0, 3])                        # the small file in the large ring
    torch.cuda.synchronize()
    assert torch.equal(first, third)
    other = MjpegDecoder(DEV, depth=2, reduce="auto", **kw)
    ob, oc = other.probe(files[1])[0], other.probe(files[2])[0]
    c_first = other.decode(oc, [1, 4])
    ring = other._ring_bytes
    assert other._surface.numel() == surf_c
    b_second = other.decode(ob, [0, 3])
    assert other._surface.numel() == surf_b and other._ring_bytes == ring
    torch.cuda.synchronize()
    assert torch.equal(c_first, second) and torch.equal(b_second, first)
    for got, want in ((first, want_b), (second, want_c)):
        assert (got.cpu() - want).abs().max().item() <= MIRROR_TOL
    full = MjpegDecoder(DEV, reduce=1, **kw)
    full.decode(full.probe(files[2])[0], [1, 4])
    assert full._surface.numel() == 16 * surf_c
    # reduce=8 on the large file, and the warm-ups at the reduce in use
    dec8 = MjpegDecoder(DEV, reduce=8, **kw)
    v8 = dec8.probe(files[2])[0]
    m8 = MjpegDecoder(CPU, reduce=8, **kw)
    got = dec8.decode(v8, [1, 4])
    torch.cuda.synchronize()
    assert (got.cpu() - m8.decode(m8.probe(files[2])[0], [1, 4])).abs().max().item() <= MIRROR_TOL
    dec.warmup(1)
    dec8.warmup(1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("s", REDUCES)
def test_reduced_geometry_pin_on_linear_ramps_gpu(ramps, s, axis):
    dist, thr = geometry_pin(DEV, ramps, s, axis)
    print("reduce %d along %s: distance %.4f, quarter-pixel threshold %.4f" % (s, axis, dist, thr))
    assert dist <= thr, (dist, thr)


def test_mjpeg_reduce_config_end_to_end(tmp_path):
    """configs/r2p1d-whole-mjpeg-3crop-reduce.json on a 3-file tree (288x256, 24
    frames each: the 224-pixel window of short side 128 makes "auto" 2): 6
    videos, bulk, in child processes; every finished video brought three rows
    per clip and finite logits."""
    root = tmp_path / "videos"
    for i in range(3):
        d = root / ("label%d" % (i % 2))
        d.mkdir(parents=True, exist_ok=True)
        mjpeg.write_mjpeg(str(d / ("v%d.mjpeg" % i)), ramp_frames(288, 256, 24, seed=20 + i),
                          quality=75, restart_interval=(0, 3, 18)[i])
    probe = MjpegDecoder(CPU, crop={"short_side": 128, "views": 3}, reduce="auto")
    assert probe.reduce_of(probe.probe(str(root / "label0" / "v0.mjpeg"))[0]) == 2
    check = tmp_path / "check"
    check.mkdir()
    cfg = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-mjpeg-3crop-reduce.json")))
    assert cfg["pipeline"][0]["decoder"] == "mjpeg"
    assert cfg["pipeline"][0]["decoder_args"] == {"reduce": "auto"}
    proc, res, _ = run_cfg(tmp_path, cfg, "-v", "6", "-mi", "0", "--set", "depth=18",
                           "--set", "warmup=1", timeout=600,
                           env={"RNB_VIDEO_ROOT": str(root), "RNB_CHECK_DIR": str(check),
                                "RNB_CHECK_EVERY": "1", "RNB_CHECK_MAX": "64"})
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert res["ok"] and res["videos_done"] >= 6, res
    samples = [np.load(f) for f in sorted(check.glob("runner_v*.npz"))]
    assert len(samples) >= 6, len(samples)
    for s in samples:
        n = len(s["starts"])
        assert n % 3 == 0 and 3 <= n <= 15 and s["logits"].shape == (n, 400)
        assert 0 <= int(s["vid"]) < 3 and np.isfinite(s["logits"]).all()
