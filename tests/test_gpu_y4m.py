"""The y4m decode backend on the GPU: yuv420_clip_kernel against its CPU
mirror and against nv12_clip_kernel, Y4mDecoder's slot / ring contract, and
the shipped y4m config end to end."""
import json
import os

import numpy as np
import pytest
import torch

from rnb_amd.ops import video as vops
from test_pipeline_e2e import ROOT, run_cfg
from test_y4m_cpu import planes, raw_y4m

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def small_buf():
    """Random bytes holding 2 clips x 3 frames of 46x34 (frame stride 2352 =
    6 + 46*34*3/2, so plane bases fall on odd offsets) at two distinct bases."""
    g = torch.Generator().manual_seed(0)
    buf = torch.randint(0, 256, (8 * 2352 + 16,), dtype=torch.uint8, generator=g)
    return buf, [5, 5 + 4 * 2352 + 3]


@pytest.fixture(scope="module")
def small_refs(small_buf):
    """CPU mirror results, computed once per (layout, crop)."""
    buf, offs = small_buf
    refs = {}
    for layout, pl in (("planar", vops.i420_planes(46, 34, 6)),
                       ("interleaved", vops.nv12_planes(46, 34, 6))):
        for crop in (None, (3.0, 2.0, 36.0, 28.0)):
            refs[layout, crop] = vops.yuv420_to_clip(buf, offs, 3, 46, 34, 2352, pl, 24, 16,
                                                     crop=crop, dtype=torch.float32)
    return refs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("crop", [None, (3.0, 2.0, 36.0, 28.0)])
def test_yuv420_kernel_matches_cpu_mirror(small_buf, small_refs, dtype, layout, crop):
    buf, offs = small_buf
    pl = vops.i420_planes(46, 34, 6) if layout == "planar" else vops.nv12_planes(46, 34, 6)
    y = vops.yuv420_to_clip(buf.to(DEV), offs, 3, 46, 34, 2352, pl, 24, 16, crop=crop,
                            dtype=dtype)
    torch.cuda.synchronize()
    C = 4 if dtype == torch.float32 else 8
    assert y.shape == (2, 3, 16, 24, C) and y.dtype == dtype
    ref = small_refs[layout, crop]
    err = (y.float().cpu()[..., :3] - ref[..., :3]).abs().max().item()
    print("max |kernel - mirror| =", err)
    # the tolerances of test_nv12_to_clip_matches_cpu_mirror (same arithmetic)
    tol = 5e-4 if dtype == torch.float32 else 2e-2
    assert err <= tol, err
    assert torch.all(y[..., 3:] == 0)


def test_yuv420_launcher_refuses_spans_outside_the_buffer(small_buf):
    """Host-side validation: nothing is launched for a span or a plane that
    would leave the uploaded bytes."""
    buf, offs = small_buf
    d = buf.to(DEV)
    pl = vops.i420_planes(46, 34, 6)
    with pytest.raises(RuntimeError, match="contract"):
        vops.yuv420_to_clip(d, [offs[0], d.numel() - 3 * 2352 + 1], 3, 46, 34, 2352, pl, 24, 16)
    with pytest.raises(RuntimeError, match="contract"):
        vops.yuv420_to_clip(d, [-1], 3, 46, 34, 2352, pl, 24, 16)
    with pytest.raises(RuntimeError, match="contract"):          # planes past the stride
        vops.yuv420_to_clip(d, offs, 3, 46, 34, 2351, pl, 24, 16)
    with pytest.raises(ValueError, match="out must be"):
        vops.yuv420_to_clip(d, offs, 3, 46, 34, 2352, pl, 24, 16,
                            out=torch.empty((2, 3, 16, 24, 8), device=DEV))
    torch.cuda.synchronize()


def test_yuv420_kernel_agrees_with_nv12_kernel():
    """340x256 -> 112x112: the new kernel on I420 frames behind FRAME markers
    and nv12_clip_kernel on the same pixels as NV12 (shared device functions;
    bound of test_nv12_decoder_writes_the_loader_slot_layout)."""
    W, H, F = 340, 256, 8
    nv = vops.nv12gen(3, [17], F, H, W, CPU)                        # [8, 384, 340]
    uv = nv[:, H:].reshape(F, H // 2, W // 2, 2)
    i420 = torch.cat([torch.full((F, 6), 70, dtype=torch.uint8), nv[:, :H].reshape(F, -1),
                      uv[..., 0].reshape(F, -1), uv[..., 1].reshape(F, -1)], dim=1)
    stride = 6 + W * H * 3 // 2
    assert i420.shape == (F, stride)
    a = vops.yuv420_to_clip(i420.reshape(-1).to(DEV), [0], F, W, H, stride,
                            vops.i420_planes(W, H, 6))
    b = vops.nv12_to_clip(nv.to(DEV), W, H)
    torch.cuda.synchronize()
    err = (a.view(F, 112, 112, 4) - b).abs().max().item()
    print("max |yuv420 kernel - nv12 kernel| =", err)
    assert err <= 2e-5, err


@pytest.fixture(scope="module")
def two_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("y4m")
    fa, fb = planes(46, 34, 30, 11), planes(64, 48, 24, 12)
    (d / "a.y4m").write_bytes(raw_y4m(46, 34, fa))
    (d / "b.y4m").write_bytes(raw_y4m(64, 48, fb, "F30:1 C420mpeg2"))
    return str(d / "a.y4m"), str(d / "b.y4m")


def test_y4m_decoder_slot_contract_and_ring_reuse(two_files):
    from rnb_amd.models.r2p1d.decoder import Y4mDecoder
    mirror = Y4mDecoder(CPU, dtype=torch.float32)
    dec = Y4mDecoder(DEV, dtype=torch.float32, depth=2)
    ids = [(dec.probe(p)[0], mirror.probe(p)[0]) for p in two_files]
    slot = torch.full((15, 8, 112, 112, 4), 7.0, device=DEV)
    got = dec.decode(ids[0][0], [0, 9], out=slot[:2])
    torch.cuda.synchronize()
    assert got.data_ptr() == slot.data_ptr() and got.shape == (2, 8, 112, 112, 4)
    ref = mirror.decode(ids[0][1], [0, 9])
    err = (slot[:2].cpu() - ref).abs().max().item()
    print("slot: max |decoder - mirror| =", err)
    assert err < 2e-5, err
    assert torch.all(slot[2:] == 7.0)
    # 12 requests back to back on alternating files through a ring of 2, no
    # host synchronisation in between: reuse is ordered by the entries' events
    outs = torch.zeros((12, 2, 8, 112, 112, 4), device=DEV)
    reqs = [(k % 2, [k % 7, 8 + k % 8]) for k in range(12)]     # b.y4m holds 24 frames
    for k, (f, starts) in enumerate(reqs):
        dec.decode(ids[f][0], starts, out=outs[k])
    assert len(dec._ring) == 2
    torch.cuda.synchronize()
    host = outs.cpu()
    for k, (f, starts) in enumerate(reqs):
        err = (host[k] - mirror.decode(ids[f][1], starts)).abs().max().item()
        assert err < 2e-5, (k, err)
    # without out= the decoder allocates; bf16 slot layout
    d16 = Y4mDecoder(DEV, dtype=torch.bfloat16)
    v16, _ = d16.probe(two_files[1])
    d16.warmup(1)
    y = d16.decode(v16, [3])
    torch.cuda.synchronize()
    assert y.shape == (1, 8, 112, 112, 8) and torch.all(y[..., 3:] == 0)
    err = (y.float().cpu()[..., :3] - mirror.decode(ids[1][1], [3])[..., :3]).abs().max().item()
    assert err <= 2e-2, err


def test_y4m_decoder_device_offset_table(tmp_path):
    """65 clips in one request: past the 64 rows that fit the kernel
    arguments, so the tables are read from device memory."""
    from rnb_amd.models.r2p1d.decoder import Y4mDecoder
    path = tmp_path / "long.y4m"
    path.write_bytes(raw_y4m(46, 34, planes(46, 34, 40, 13)))
    kw = dict(clip_length=2, height=16, width=24, dtype=torch.float32)
    dec, mirror = Y4mDecoder(DEV, **kw), Y4mDecoder(CPU, **kw)
    vid, n = dec.probe(str(path))
    mirror.probe(str(path))
    starts = [(5 * k) % 39 for k in range(65)]
    y = dec.decode(vid, starts)
    torch.cuda.synchronize()
    ref = mirror.decode(vid, starts)
    assert y.shape == (65, 2, 16, 24, 4)
    err = (y.cpu() - ref).abs().max().item()
    print("65 clips: max |decoder - mirror| =", err)
    assert err <= 5e-4, err


def test_y4m_config_end_to_end(tmp_path):
    """configs/r2p1d-whole-y4m.json on a 3-file tree (64x48, 40 frames each):
    6 videos, bulk, in child processes; every finished video brought clips."""
    root = tmp_path / "videos"
    for i in range(3):
        d = root / ("label%d" % (i % 2))
        d.mkdir(parents=True, exist_ok=True)
        (d / ("v%d.y4m" % i)).write_bytes(raw_y4m(64, 48, planes(64, 48, 40, 20 + i)))
    check = tmp_path / "check"
    check.mkdir()
    cfg = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-y4m.json")))
    assert cfg["pipeline"][0]["decoder"] == "y4m"
    proc, res, _ = run_cfg(tmp_path, cfg, "-v", "6", "-mi", "0", "--set", "depth=18",
                           "--set", "warmup=1", timeout=600,
                           env={"RNB_VIDEO_ROOT": str(root), "RNB_CHECK_DIR": str(check),
                                "RNB_CHECK_EVERY": "1", "RNB_CHECK_MAX": "64"})
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert res["ok"] and res["videos_done"] >= 6, res
    logdir = tmp_path / "logs" / res["job_id"]
    rows = sum(len(open(logdir / f).read().splitlines()) - 1
               for f in os.listdir(logdir) if f.startswith("g"))
    assert rows >= 6, rows
    # the runner's record of every served video: the clips the loader decoded
    # from the file (40 frames hold at most 5 clips of 8) and their logits
    samples = [np.load(f) for f in sorted(check.glob("runner_v*.npz"))]
    assert len(samples) >= 6, len(samples)
    for s in samples:
        assert 1 <= len(s["starts"]) <= 5 and s["logits"].shape == (len(s["starts"]), 400)
        assert 0 <= int(s["vid"]) < 3 and np.isfinite(s["logits"]).all()
