"""The mjpeg decode backend on the GPU: jpeg_idct_kernel against the fp64 ideal
IDCT and against PIL's planes, the JFIF clip stage against its CPU mirror, the
launcher's refusals, MjpegDecoder's slot / ring contract, and the shipped mjpeg
config end to end."""
import json
import os

import numpy as np
import pytest
import torch

from rnb_amd.ops import video as vops
from rnb_amd.utils import mjpeg
from test_mjpeg_cpu import (GOLDEN, GOLDEN_STREAMS, SHAPES, check_band, ideal_planes, idct_inputs,
                            native_records, noise_frames, ramp_frames, records_tensor)
from test_pipeline_e2e import ROOT, run_cfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def idct_cases():
    """(W, H) -> kind -> (records [6 frames], fp64 planes), computed once."""
    out = {}
    for W, H in SHAPES:
        mw, mh, _ = mjpeg.geometry(W, H)
        out[W, H] = {kind: (records_tensor(frames), ideal_planes(frames, mw, mh))
                     for kind, frames in idct_inputs(W, H).items()}
    return out


@pytest.mark.parametrize("W,H", SHAPES)
def test_idct_kernel_against_fp64(idct_cases, W, H):
    """6 frames, a different table on each; the band rule of check_band. The
    surface is dirtied first: padding rows and columns are written too."""
    mw, mh, rb = mjpeg.geometry(W, H)
    need = 6 * 384 * mw * mh
    for kind, (rec, ideal) in idct_cases[W, H].items():
        d = rec.to(DEV)
        surf = torch.full((need + 64,), 0xAA, dtype=torch.uint8, device=DEV)
        a = vops.jpeg_idct(d, 6, mw, mh, out=surf)
        assert a.data_ptr() == surf.data_ptr() and a.shape == (need,)
        first = a.cpu().numpy().copy()
        assert torch.all(surf[need:] == 0xAA)                 # nothing past the frames
        surf.fill_(0x55)
        second = vops.jpeg_idct(d, 6, mw, mh, out=surf).cpu().numpy()
        assert np.array_equal(first, second)                  # no stale byte survives
        fresh = vops.jpeg_idct(d, 6, mw, mh).cpu().numpy()
        assert np.array_equal(first, fresh)
        check_band(first, ideal, "%dx%d %s" % (W, H, kind), tie_only=kind == "dc_only")
        if kind == "clamp":
            assert (first == 0).any() and (first == 255).any()


@pytest.mark.parametrize("name", sorted(GOLDEN_STREAMS))
def test_idct_kernel_luma_against_pils_planes(name):
    W, H, _ = GOLDEN_STREAMS[name]
    path = os.path.join(GOLDEN, name + ".mjpeg")
    lumas = np.load(os.path.join(GOLDEN, name + "_luma.npy"))
    idx = mjpeg.read_index(path)
    frames = native_records(np.fromfile(path, dtype=np.uint8), idx)
    surf = vops.jpeg_idct(records_tensor(frames).to(DEV), 2, idx.mw, idx.mh).cpu().numpy()
    fb = 384 * idx.mw * idx.mh
    for i in range(2):
        y = surf[i * fb:i * fb + 256 * idx.mw * idx.mh].reshape(16 * idx.mh, 16 * idx.mw)
        d = np.abs(y[:H, :W].astype(int) - lumas[i].astype(int))
        print(name, i, "max |kernel luma - PIL luma| =", d.max(), "mean", d.mean())
        assert d.max() <= 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("W,H,crop", [(46, 34, None), (46, 34, (3.0, 2.0, 36.0, 28.0)),
                                      (45, 33, None)])
def test_jfif_clip_stage_matches_cpu_mirror(W, H, crop, dtype):
    """2 clips x 3 frames: the clip kernel on the IDCT kernel's own surface,
    the mirror on the same (downloaded) planes."""
    mw, mh, _ = mjpeg.geometry(W, H)
    q = mjpeg.quality_tables(80)
    frames = [(mjpeg.encode_frame(*f, q)[1], q[[0, 1, 1]]) for f in noise_frames(W, H, 6, 77)]
    surf = vops.jpeg_idct(records_tensor(frames).to(DEV), 6, mw, mh)
    fb = 384 * mw * mh
    pl = vops.jpeg_surface_planes(mw, mh)
    y = vops.yuv420_to_clip(surf, [3 * fb, 0], 3, W, H, fb, pl, 24, 16, crop=crop, dtype=dtype,
                            matrix="jfif")
    torch.cuda.synchronize()
    C = 4 if dtype == torch.float32 else 8
    assert y.shape == (2, 3, 16, 24, C) and y.dtype == dtype
    ref = vops.yuv420_to_clip(surf.cpu(), [3 * fb, 0], 3, W, H, fb, pl, 24, 16, crop=crop,
                              matrix="jfif")
    err = (y.float().cpu()[..., :3] - ref[..., :3]).abs().max().item()
    print("max |kernel - mirror| =", err)
    tol = 5e-4 if dtype == torch.float32 else 2e-2     # test_yuv420_kernel_matches_cpu_mirror's
    assert err <= tol, err
    assert torch.all(y[..., 3:] == 0)
    # not the BT.601 matrix
    other = vops.yuv420_to_clip(surf, [3 * fb, 0], 3, W & ~1, H & ~1, fb, pl, 24, 16, dtype=dtype)
    assert (other.float() - y.float()).abs().max().item() > 0.1


def test_jpeg_idct_launcher_refusals():
    mw, mh, rb = mjpeg.geometry(46, 34)
    rec = torch.zeros(3 * rb, dtype=torch.uint8, device=DEV)
    surf = torch.full((3 * 384 * mw * mh,), 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="contract"):          # records too small
        vops.jpeg_idct(rec[:3 * rb - 16], 3, mw, mh, out=surf)
    with pytest.raises(RuntimeError, match="contract"):          # surface too small
        vops.jpeg_idct(rec, 3, mw, mh, out=surf[:3 * 384 * mw * mh - 8])
    with pytest.raises(RuntimeError, match="contract"):          # a larger geometry
        vops.jpeg_idct(rec, 3, mw + 1, mh, out=surf)
    with pytest.raises(RuntimeError, match="contract"):          # records closer than a record
        vops.jpeg_idct(rec, 3, mw, mh, out=surf, record_bytes=rb - 16)
    with pytest.raises(RuntimeError, match="contract"):          # misaligned records
        vops.jpeg_idct(rec[8:8 + 2 * rb], 2, mw, mh, out=surf)
    with pytest.raises(ValueError, match="out must be"):
        vops.jpeg_idct(rec, 3, mw, mh, out=surf.view(3, -1))
    with pytest.raises(ValueError, match="out must be"):
        vops.jpeg_idct(rec, 3, mw, mh, out=surf.view(torch.int8))
    with pytest.raises(ValueError, match="out must be"):
        vops.jpeg_idct(rec, 3, mw, mh, out=surf.cpu())
    with pytest.raises(ValueError, match="records must be"):
        vops.jpeg_idct(rec.view(3, rb), 3, mw, mh, out=surf)
    torch.cuda.synchronize()
    assert torch.all(surf == 9)                                  # nothing was launched


@pytest.fixture(scope="module")
def two_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mjpeg")
    mjpeg.write_mjpeg(str(d / "a.mjpeg"), ramp_frames(46, 34, 30), quality=85, restart_interval=2)
    mjpeg.write_mjpeg(str(d / "b.mjpeg"), noise_frames(64, 48, 24, 12), quality=70)
    return str(d / "a.mjpeg"), str(d / "b.mjpeg")


# GPU decoder against the CPU-device one: the IDCT kernel and its mirror may
# round a tie differently, by one level in Y and in one chroma plane at once:
# (1 + 1.772) / (255 * 0.217) = 0.0501 after normalisation, plus the clip
# stage's own tolerance
MIRROR_TOL = 0.051


def test_mjpeg_decoder_slot_contract_and_ring_reuse(two_files):
    from rnb_amd.models.r2p1d.decoder import MjpegDecoder
    mirror = MjpegDecoder(CPU, dtype=torch.float32)
    dec = MjpegDecoder(DEV, dtype=torch.float32, depth=2)
    ids = [(dec.probe(p)[0], mirror.probe(p)[0]) for p in (two_files[0],)]
    slot = torch.full((15, 8, 112, 112, 4), 7.0, device=DEV)
    got = dec.decode(ids[0][0], [0, 9], out=slot[:2])
    torch.cuda.synchronize()
    assert got.data_ptr() == slot.data_ptr() and got.shape == (2, 8, 112, 112, 4)
    err = (slot[:2].cpu() - mirror.decode(ids[0][1], [0, 9])).abs().max().item()
    print("slot: max |decoder - mirror| =", err)
    assert err <= MIRROR_TOL, err
    assert torch.all(slot[2:] == 7.0) and torch.all(slot[:2, ..., 3] == 0)
    small = dec._ring_bytes
    # the ring regrows for the larger second file
    vb, nb = dec.probe(two_files[1])
    assert nb == 24
    dec.decode(vb, [0])
    assert dec._ring_bytes > small and len(dec._ring) == 2
    # 10 requests back to back on alternating files through a ring of 2, no host
    # synchronisation in between; every result equals a fresh decoder's
    outs = torch.zeros((10, 2, 8, 112, 112, 4), device=DEV)
    reqs = [(k % 2, [k % 7, 8 + k % 8]) for k in range(10)]
    vids = (ids[0][0], vb)
    for k, (f, starts) in enumerate(reqs):
        dec.decode(vids[f], starts, out=outs[k])
    assert len(dec._ring) == 2
    torch.cuda.synchronize()
    for k, (f, starts) in enumerate(reqs[:4]):
        fresh = MjpegDecoder(DEV, dtype=torch.float32, threads=1)
        v, _ = fresh.probe(two_files[f])
        assert torch.equal(fresh.decode(v, starts), outs[k]), k
    # bf16 slot layout, warm-up without a file
    d16 = MjpegDecoder(DEV, dtype=torch.bfloat16)
    d16.warmup(1)
    v16, _ = d16.probe(two_files[0])
    slot16 = torch.full((3, 8, 112, 112, 8), 7.0, dtype=torch.bfloat16, device=DEV)
    y = d16.decode(v16, [3], out=slot16[1:2])
    torch.cuda.synchronize()
    assert y.data_ptr() == slot16[1:2].data_ptr() and torch.all(y[..., 3:] == 0)
    assert torch.all(slot16[0] == 7.0) and torch.all(slot16[2] == 7.0)
    err = (y.float().cpu()[..., :3] - mirror.decode(ids[0][1], [3])[..., :3]).abs().max().item()
    assert err <= MIRROR_TOL + 2e-2, err


def test_mjpeg_decoder_device_offset_table_and_threads(two_files):
    """65 clips in one request: past the 64 rows that fit the clip kernel's
    arguments; 1 and 4 entropy-decode threads give identical bytes."""
    from rnb_amd.models.r2p1d.decoder import MjpegDecoder
    kw = dict(clip_length=2, height=16, width=24, dtype=torch.float32)
    d1, d4 = MjpegDecoder(DEV, threads=1, **kw), MjpegDecoder(DEV, threads=4, **kw)
    mirror = MjpegDecoder(CPU, **kw)
    v1, n = d1.probe(two_files[0])
    v4, _ = d4.probe(two_files[0])
    vm, _ = mirror.probe(two_files[0])
    starts = [(5 * k) % (n - 1) for k in range(65)]
    a, b = d1.decode(v1, starts), d4.decode(v4, starts)
    torch.cuda.synchronize()
    assert a.shape == (65, 2, 16, 24, 4) and torch.equal(a, b)
    assert torch.equal(d1._ring[0].pinned[:65 * 2 * 7296], d4._ring[0].pinned[:65 * 2 * 7296])
    err = (a.cpu() - mirror.decode(vm, starts)).abs().max().item()
    print("65 clips: max |decoder - mirror| =", err)
    assert err <= MIRROR_TOL, err


def test_mjpeg_config_end_to_end(tmp_path):
    """configs/r2p1d-whole-mjpeg.json on a 3-file tree (64x48, 40 frames each):
    6 videos, bulk, in child processes; every finished video brought clips."""
    root = tmp_path / "videos"
    for i in range(3):
        d = root / ("label%d" % (i % 2))
        d.mkdir(parents=True, exist_ok=True)
        mjpeg.write_mjpeg(str(d / ("v%d.mjpeg" % i)), ramp_frames(64, 48, 40, seed=20 + i),
                          quality=75, restart_interval=(0, 3, 12)[i])
    check = tmp_path / "check"
    check.mkdir()
    cfg = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-mjpeg.json")))
    assert cfg["pipeline"][0]["decoder"] == "mjpeg"
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
