"""clip_length (8, 16 or 32 frames) through the geometry table, the engine's
size check, the plugins, the pipeline config and the file-backed decoders --
everything that runs without a GPU.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rnb_amd import config as rconfig
from rnb_amd.batcher import Batcher
from rnb_amd.models.r2p1d import engine as eng
from rnb_amd.models.r2p1d.decoder import MjpegDecoder, Y4mDecoder
from rnb_amd.models.r2p1d.model import (R2P1DAggregator, R2P1DLoader, R2P1DRunner,
                                        build_engine, build_network)
from rnb_amd.models.r2p1d.network import (LAYER_INPUT_CTHW, LAYER_OUTPUT_CTHW, layer_geometry)
from rnb_amd.utils import mjpeg, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
M = "rnb_amd.models.r2p1d.model."


def test_geometry_at_8_is_the_module_constants():
    assert layer_geometry(8) == (LAYER_INPUT_CTHW, LAYER_OUTPUT_CTHW)
    assert layer_geometry() == (LAYER_INPUT_CTHW, LAYER_OUTPUT_CTHW)


@pytest.mark.parametrize("bad", [12, 0, -8, 64, "16", None, True])
def test_other_clip_lengths_raise(bad):
    with pytest.raises(ValueError, match="clip_length"):
        layer_geometry(bad)


@pytest.mark.parametrize("clip_length", [8, 16, 32])
def test_geometry_equals_what_the_module_produces(clip_length):
    """For every start layer 1-5: the table's input shape fed to the nn.Module
    of layers [start, start] (depth 10, one clip) gives the table's output
    shape, i.e. the next layer's input."""
    inp, out = layer_geometry(clip_length)
    for start in range(1, 6):
        net = build_network(start, start, depth=10)
        e = eng.R2P1DEngine(net, CPU, backend="module", dtype=torch.float32,
                            clip_length=clip_length)
        c, t, h, w = inp[start]
        assert e.input_shape(1) == (1, t, h, w, eng.boundary_channels_p(start, torch.float32))
        with torch.no_grad():
            y = e.module(torch.zeros(1, c, t, h, w))
        if start == 5:
            assert out[5] is None and tuple(y.shape) == (1, 400)
            assert e.output_shape(1) == (1, 400)
        else:
            assert tuple(y.shape) == (1,) + out[start], (start, tuple(y.shape))
            assert out[start] == inp[start + 1]
            co, to, ho, wo = out[start]
            assert e.output_shape(1) == (1, to, ho, wo, co)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("clip_length", [8, 16, 32])
def test_max_clips_bound_from_arithmetic(clip_length, dtype):
    """The construction-time check accepts the largest fitting max_clips and
    refuses the next one; nothing is allocated. The bound is the kernels'
    per-launch limit over the largest activation of the range: per clip the
    conv2 stage's (2+1)D intermediate, 144 channels x T x 56 x 56."""
    fit = eng.max_clips_limit(1, 5, dtype, clip_length)
    per = 144 * clip_length * 56 * 56
    assert eng.activation_elems_per_clip(1, 5, dtype, clip_length) == per
    if dtype == torch.float32:
        # fp32 conv launches are split by clips; the BatchNorm kernels index
        # float4s of the whole call with 32 bits
        assert fit == (4 * 0x7FFFFFFF) // per
    else:
        assert fit == 0x7FFFFF00 // (2 * per)
    assert eng.check_max_clips(fit, 1, 5, dtype, clip_length) == fit
    with pytest.raises(ValueError) as err:
        eng.check_max_clips(fit + 1, 1, 5, dtype, clip_length)
    msg = str(err.value)
    assert "max_clips" in msg and "clip_length %d" % clip_length in msg and str(fit) in msg
    # rows per clip grow with T: the bound shrinks in proportion
    assert fit <= eng.max_clips_limit(1, 5, dtype, 8) * 8 // clip_length + 1


def test_max_clips_bound_at_8_covers_every_shipped_value():
    """bench.py serves up to --clips-per-batch 256 clips per call (fp32 and
    bf16); the shipped configs set max_clips 5, 15 (default) and 16."""
    used = {256, 15}
    for name in os.listdir(os.path.join(ROOT, "configs")):
        cfg = json.load(open(os.path.join(ROOT, "configs", name)))
        for step in cfg.get("pipeline", []):
            for d in [cfg.get("defaults", {}), step] + list(step.get("queue_groups", [])):
                if "max_clips" in d:
                    used.add(int(d["max_clips"]))
    for dtype in (torch.float32, torch.bfloat16):
        assert max(used) <= eng.max_clips_limit(1, 5, dtype, 8), (used, dtype)
    # a later range alone is bounded by its own (smaller) activations
    assert eng.max_clips_limit(4, 5, torch.float32, 32) > eng.max_clips_limit(1, 5,
                                                                              torch.float32, 32)


def test_engine_construction_refuses_a_max_clips_past_the_bound():
    fit = eng.max_clips_limit(1, 5, torch.bfloat16, 32)
    with pytest.raises(ValueError, match="max_clips"):
        eng.check_max_clips(fit + 1, 1, 5, torch.bfloat16, 32)
    # the torch / module backends launch no such kernel: not checked
    e = build_engine(CPU, depth=10, backend="torch", max_clips=10 ** 6, clip_length=32,
                     dtype="fp32")
    assert e.clip_length == 32 and e.input_shape(2) == (2, 32, 112, 112, 4)


def test_loader_serves_16_frame_clips():
    ld = R2P1DLoader(CPU, clip_length=16, warmup=0, num_clips_population=(3,),
                     num_clips_weights=(1,), seed=1)
    frames = ld.load("synthetic://7?frames=300")
    assert tuple(frames.shape) == (3, 16, 112, 112, 4)
    assert R2P1DLoader.output_shape_for(clip_length=16) == ((15, 16, 112, 112, 4),)
    assert R2P1DLoader.output_shape_for(max_clips=4, dtype="bf16", clip_length=32) == \
        ((4, 32, 112, 112, 8),)
    assert R2P1DLoader.output_shape_for() == ((15, 8, 112, 112, 4),)
    assert ld.sampler.clip_length == 16


def test_plugins_take_clip_length_and_refuse_other_values():
    assert R2P1DRunner.output_shape_for(start_index=1, end_index=2, clip_length=16) == \
        ((15, 16, 56, 56, 64),)
    assert R2P1DRunner.output_shape_for(start_index=1, end_index=3, clip_length=32,
                                        max_clips=2) == ((2, 16, 28, 28, 128),)
    assert R2P1DRunner.output_shape_for(end_index=4) == ((15, 2, 14, 14, 256),)
    assert Batcher.output_shape_for(max_rows=6, clip_length=16) == ((6, 16, 112, 112, 4),)
    assert Batcher(CPU, batch=2, clip_length=32).input_shape() == ((15, 32, 112, 112, 4),)
    r = R2P1DRunner(CPU, start_index=3, end_index=5, depth=10, warmup=0, clip_length=16,
                    backend="torch")
    assert r.input_shape() == ((15, 16, 56, 56, 64),)
    for make in (lambda: R2P1DLoader(CPU, clip_length=12, warmup=0),
                 lambda: R2P1DRunner(CPU, depth=10, warmup=0, clip_length=24),
                 lambda: R2P1DAggregator(CPU, clip_length=0),
                 lambda: Batcher(CPU, clip_length=7),
                 lambda: R2P1DRunner.output_shape_for(clip_length=9),
                 lambda: R2P1DLoader.output_shape_for(clip_length=4)):
        with pytest.raises(ValueError, match="clip_length"):
            make()


def _pipeline(loader_kw, runner_kw, defaults=None):
    return {"video_path_iterator": M + "R2P1DVideoPathIterator",
            "defaults": defaults or {},
            "pipeline": [
                dict({"model": M + "R2P1DLoader",
                      "queue_groups": [{"gpus": [-1], "out_queues": [0]}]}, **loader_kw),
                dict({"model": M + "R2P1DRunner",
                      "queue_groups": [{"gpus": [-1], "in_queue": 0}]}, **runner_kw)]}


def test_pipeline_whose_steps_disagree_is_refused(tmp_path):
    path = tmp_path / "p.json"
    path.write_text(json.dumps(_pipeline({"clip_length": 16}, {"clip_length": 8})))
    with pytest.raises(rconfig.ConfigError) as err:
        rconfig.load_pipeline(str(path))
    msg = str(err.value)
    assert "clip_length" in msg and "step 0" in msg and "step 1" in msg
    assert "R2P1DLoader" in msg and "R2P1DRunner" in msg and "16" in msg and "8" in msg
    # the runner's default is 8: a loader alone at 16 disagrees too
    path.write_text(json.dumps(_pipeline({"clip_length": 16}, {})))
    with pytest.raises(rconfig.ConfigError, match="clip_length"):
        rconfig.load_pipeline(str(path))
    # set once in defaults, or in both steps: accepted, and every step sees it
    for cfg in (_pipeline({}, {}, {"clip_length": 16}),
                _pipeline({"clip_length": 32}, {"clip_length": 32})):
        path.write_text(json.dumps(cfg))
        spec = rconfig.load_pipeline(str(path))
        assert len({g.kwargs["clip_length"] for s in spec.steps for g in s.groups}) == 1
    spec = rconfig.load_pipeline(os.path.join(ROOT, "configs", "r2p1d-whole-16f.json"))
    assert all(g.kwargs["clip_length"] == 16 for s in spec.steps for g in s.groups)
    base = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole.json")))
    long = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-16f.json")))
    assert long["defaults"].pop("clip_length") == 16 and long == base


def test_whole_16f_config_served_on_cpu_and_rechecked(tmp_path):
    """One --cpu-only launcher run of the shipped 16-frame config at depth 10:
    the sampled videos' logits, recomputed offline from the clip length the
    samples record, within the bound of tests/test_pipeline_e2e.py's check."""
    from rnb_amd.numerics import recheck
    check = tmp_path / "check"
    check.mkdir()
    out = tmp_path / "res.json"
    env = dict(os.environ, RNB_NO_TQDM="1", RNB_CPU_THREADS="1", PYTHONPATH=ROOT,
               RNB_CHECK_DIR=str(check), RNB_CHECK_EVERY="2")
    cmd = [sys.executable, os.path.join(ROOT, "benchmark.py"),
           "-c", os.path.join(ROOT, "configs", "r2p1d-whole-16f.json"),
           "--log-root", str(tmp_path / "logs"), "--json-out", str(out),
           "--barrier-timeout", "200", "-v", "5", "-mi", "0", "--cpu-only",
           "--set", "depth=10", "--set", "num_clips_population=[1,3]",
           "--set", "num_clips_weights=[2,1]", "--set", "warmup=0", "--set", "max_clips=3",
           "--set", "bn_mode=batch"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=env)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    res = json.loads(out.read_text())
    assert res["ok"] and res["videos_done"] == 5
    files = sorted(check.glob("*.npz"))
    assert files and all(int(np.load(f)["clip_length"]) == 16 for f in files)
    num = recheck(str(check), 10, CPU, bn_mode="batch")
    print("numerics:", num)
    assert num["videos_checked"] >= 1, num
    assert num["top1_agree"] >= 0.99 and num["max_rel_err"] <= 1e-4, num


def test_old_samples_without_a_clip_length_read_as_8(tmp_path):
    """A sample file written before clips had a length: recheck decodes 8
    frames per clip for it."""
    from rnb_amd.numerics import recheck
    net = build_network(1, 5, depth=10, seed=0)
    mod = eng.R2P1DEngine(net, CPU, backend="module", bn_mode="batch", dtype=torch.float32)
    ld = R2P1DLoader(CPU, warmup=0)
    x = ld.decoder.decode(4, [0, 9])
    assert x.shape[1] == 8
    with torch.no_grad():
        logits = mod.forward(x).numpy()
    np.savez(tmp_path / "runner_v0_p1.npz", kind="runner", vid=4,
             starts=np.asarray([0, 9], dtype=np.int64), logits=logits, bn_mode="batch",
             dtype="torch.float32", segments=1, call_rows=2, stratum="small")
    num = recheck(str(tmp_path), 10, CPU)
    assert num["videos_checked"] == 1 and num["max_rel_err"] <= 1e-6, num


def _frames(W, H, n, seed):
    rng = np.random.default_rng(seed)
    # smooth planes plus noise: a JPEG-friendly picture that still differs per frame
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        y = (96 + 60 * np.sin((xx + 3 * i) / 7.0) + 40 * np.cos((yy - 2 * i) / 5.0)
             + rng.integers(-6, 7, (H, W)))
        u = 128 + 50 * np.sin((xx[::2, ::2] + i) / 9.0) + rng.integers(-4, 5, (H // 2, W // 2))
        v = 128 + 50 * np.cos((yy[::2, ::2] + 2 * i) / 6.0) + rng.integers(-4, 5, (H // 2, W // 2))
        out.append(tuple(np.clip(p, 0, 255).astype(np.uint8) for p in (y, u, v)))
    return out


@pytest.mark.parametrize("kind", ["y4m", "mjpeg"])
def test_file_decoders_at_16_frames_match_the_8_frame_decoder(tmp_path, kind):
    """CPU mirrors on a generated 20-frame 46 x 34 file: frame j of the
    16-frame clip starting at s equals the 8-frame decoder's output for the
    same source frame s + j (span tables, clip offsets and upload sizing all
    follow the clip length)."""
    W, H, N = 46, 34, 20
    fr = _frames(W, H, N, 7)
    path = str(tmp_path / ("v." + kind))
    if kind == "y4m":
        y4m.write_y4m(path, fr, fps=(25, 1))
        make = lambda F: Y4mDecoder(CPU, clip_length=F, dtype=torch.float32)
    else:
        mjpeg.write_mjpeg(path, fr, quality=85)
        make = lambda F: MjpegDecoder(CPU, clip_length=F, dtype=torch.float32)
    d8, d16 = make(8), make(16)
    v8, n8 = d8.probe(path)
    v16, n16 = d16.probe(path)
    assert n8 == n16 == N
    starts = [0, 3, 4]                                   # the last clip ends on frame 19
    got = d16.decode(v16, starts)
    assert tuple(got.shape) == (3, 16, 112, 112, 4)
    ref = d8.decode(v8, list(range(0, N - 7)))           # every 8-frame clip of the file
    for k, s in enumerate(starts):
        for j in range(16):
            src = s + j
            a, f = (src, 0) if src <= N - 8 else (N - 8, src - (N - 8))
            assert torch.equal(got[k, j], ref[a, f]), (kind, k, j)
    assert tuple(d16.decode(v16, []).shape) == (0, 16, 112, 112, 4)
    with pytest.raises(ValueError):
        d16.decode(v16, [5])                             # frames 5..20: past the file
    d32 = make(32)
    v32, _ = d32.probe(path)
    with pytest.raises(ValueError):
        d32.decode(v32, [0])                             # a 32-frame clip of a 20-frame file
