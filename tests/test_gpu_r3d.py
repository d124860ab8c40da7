"""``tv_block="3d"`` (torchvision's r3d_18) on the GPU: whole engines, with the
weights of the independent oracle tests/r3d_oracle.py loaded through
``ckpt_path``, against the oracle in fp64, graph replays, the per-video module
and one launcher run of the shipped config."""
import json
import os

import pytest
import torch

import r3d_oracle
from test_gpu_f32 import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    ora = r3d_oracle.make(seed=9)
    path = str(tmp_path_factory.mktemp("r3d") / "r3d18.pt")
    torch.save(ora.state_dict(), path)
    return ora, path


def _engine(path, **kw):
    from rnb_amd.models.r2p1d.model import build_engine
    return build_engine(DEV, depth=18, arch="torchvision", ckpt_path=path, autotune=False, **kw)


def _use_h3v(eng, n):
    """Point every conv that is offered h3v at its first h3v id for calls of n
    clips (untuned engines pick generic configs); how many convs that is."""
    from rnb_amd.ops.conv_f32 import is_h3v
    shapes, served = {"x": eng.input_shape(n)}, 0
    for op in eng.ops:
        shp = shapes[op.src]
        shapes[op.dst] = op.layer.out_shape(shp)
        ids = [c for c in op.layer.candidates(shp) if is_h3v(c)]
        if ids:
            op.layer._config[tuple(shp[:4])] = ids[0]
            served += 1
    return served


def _clips32(videos, clip_length=8):
    from rnb_amd.models.r2p1d.decoder import SyntheticDecoder
    dec = SyntheticDecoder(DEV, dtype=torch.float32, clip_length=clip_length)
    return [dec.decode(vid, starts) for vid, starts in videos]


@pytest.mark.parametrize("clip_length,starts", [(8, [0, 80, 160]), (16, [0, 90])])
def test_fp32_eval_engine_vs_fp64_oracle(ckpt, clip_length, starts):
    """e_hip <= 3 e_mod + 1e-6 against the oracle in fp64, with layers 2-4's
    stride-1 3x3x3 convs over >= 2 frames on the volume-band kernel."""
    from rnb_amd.ops.video import ndhwc_to_ncdhw
    ora, path = ckpt
    hip = _engine(path, bn_mode="eval", dtype="fp32", use_graphs=False, clip_length=clip_length)
    mod = _engine(path, bn_mode="eval", dtype="fp32", backend="module", clip_length=clip_length)
    assert hip.backend == "hip" and hip.tv_block == "3d" and len(hip.ops) == 20
    (x,) = _clips32([(31, starts)], clip_length)
    served = _use_h3v(hip, x.shape[0])
    assert served == (6 if clip_length == 8 else 9), served
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        y = hip.forward(x).double().cpu()
        ym = mod.forward(x).double().cpu()
        y64 = ora.double()(ndhwc_to_ncdhw(x, 3).double().cpu())
    ora.float()
    scale = y64.abs().max().item()
    e_hip = (y - y64).abs().max().item() / scale
    e_mod = (ym - y64).abs().max().item() / scale
    print("r3d_18 %d frames vs fp64: HIP %.2e, module %.2e" % (clip_length, e_hip, e_mod))
    assert e_hip <= 3 * e_mod + 1e-6, (e_hip, e_mod)


def test_graph_replay_matches_eager_and_repeats_bit_equal(ckpt):
    from rnb_amd.models.r2p1d.engine import GraphedEngine
    hip = _engine(ckpt[1], bn_mode="eval", dtype="fp32", use_graphs=False)
    for b in (1, 2, 4):
        assert _use_h3v(hip, b) == 6
    ge = GraphedEngine(hip, max_clips=6, buckets=(1, 2, 4), autotune=False)
    for n in (1, 3, 6):
        x = torch.randn(hip.input_shape(n), device=DEV)
        x[..., 3:] = 0
        a = ge(x).clone()
        a2 = ge(x).clone()
        b = hip.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(a, a2), n
        assert torch.allclose(a, b, atol=1e-3, rtol=1e-3), (n, (a - b).abs().max().item())


def test_graphed_batch_bn_per_video_vs_module(ckpt):
    """'batch', graphed: videos of 1 + 3 clips against the per-video module."""
    from rnb_amd.models.r2p1d.engine import GraphedEngine
    g = _engine(ckpt[1], bn_mode="batch", dtype="fp32", max_clips=4, buckets=[4])
    assert isinstance(g, GraphedEngine) and g.batch_bn
    mod = _engine(ckpt[1], bn_mode="batch", dtype="fp32", backend="module")
    xs = _clips32([(21, [30]), (23, [0, 90, 180])])
    with torch.no_grad():
        y = g.forward(torch.cat(xs), clip_offsets=[0, 1, 4]).clone()
        ref = torch.cat([mod.forward(x) for x in xs])
    torch.cuda.synchronize()
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 5e-4, err


def test_launcher_serves_the_r3d18_config(tmp_path):
    from test_pipeline_e2e import run_cfg
    cfg = json.loads(open(os.path.join(ROOT, "configs", "r2p1d-whole-tv-r3d18.json")).read())
    proc, res, _ = run_cfg(tmp_path, cfg, "-v", "8", "-mi", "0", "--set", "autotune=false",
                           "--set", "num_clips_population=[1,3]",
                           "--set", "num_clips_weights=[2,1]", "--set", "max_clips=3",
                           "--set", "warmup=1", timeout=300)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert res["termination_flag"] == "TARGET_NUM_VIDEOS_REACHED" and res["videos_done"] >= 8
