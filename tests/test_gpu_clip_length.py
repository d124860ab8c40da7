"""16- and 32-frame clips on the GPU: the fp32 engine against an fp64 module,
graphed replay and BatchNorm running statistics, the head over the longer
pooling windows, loader into runner, and the default clip length's configs.

No autotuning (``autotune=False``, explicit buckets): the convs run the seed
table's / heuristic's configs, whichever family they are. The bounds are the
ones the 8-frame tests hold the same code to (named per test).
"""
import copy
import os

import pytest
import torch

from test_gpu_bn_state import Ref64, running_vs_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _videos(clip_length, videos):
    """Synthetic clips of ``videos`` = [(video id, [start frames])] at
    ``clip_length`` frames, fp32 NDHWC4."""
    from rnb_amd.models.r2p1d.decoder import SyntheticDecoder
    dec = SyntheticDecoder(DEV, clip_length=clip_length, dtype=torch.float32)
    return [dec.decode(v, s) for v, s in videos]


@pytest.mark.parametrize("clip_length,depth,videos", [
    (16, 18, [(21, [30]), (23, [0, 90])]),          # 3 clips in two videos
    (32, 10, [(22, [100]), (24, [7])])])            # 2 clips
def test_eager_fp32_batch_bn_error_vs_fp64(clip_length, depth, videos):
    """The rule of test_batch_bn_fp32_error_vs_fp64: against the same network
    in fp64 (one video per forward), the HIP fp32 engine is at least as close
    as PyTorch's own fp32 module, within a factor 3."""
    from rnb_amd.models.r2p1d.engine import R2P1DEngine
    from rnb_amd.models.r2p1d.model import build_network
    from rnb_amd.ops.video import ndhwc_to_ncdhw
    net = build_network(1, 5, depth=depth, seed=11)
    hip = R2P1DEngine(copy.deepcopy(net), DEV, backend="hip", bn_mode="batch",
                      dtype=torch.float32, clip_length=clip_length)
    mod = R2P1DEngine(copy.deepcopy(net), DEV, backend="module", bn_mode="batch",
                      dtype=torch.float32, clip_length=clip_length)
    net64 = copy.deepcopy(net).double().train()
    xs = _videos(clip_length, videos)
    assert tuple(xs[0].shape[1:]) == hip.input_shape(1)[1:]
    offs = [0]
    for x in xs:
        offs.append(offs[-1] + x.shape[0])
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        y = hip.forward_checked(torch.cat(xs), clip_offsets=offs).double().cpu()
        ym = torch.cat([mod.forward(x) for x in xs]).double().cpu()
        y64 = torch.cat([net64(ndhwc_to_ncdhw(x, 3).double().cpu()) for x in xs])
    assert hip.range_guard is None or hip.range_guard.fallbacks == 0
    scale = y64.abs().max().item()
    e_hip = (y - y64).abs().max().item() / scale
    e_mod = (ym - y64).abs().max().item() / scale
    print("%d frames, depth %d, batch-BN fp32 vs fp64: HIP %.2e, PyTorch fp32 module %.2e"
          % (clip_length, depth, e_hip, e_mod))
    assert e_hip <= 3 * e_mod + 1e-6, (e_hip, e_mod)


def test_graphed_16_frames_matches_eager_and_running_stats():
    """GraphedEngine at 16 frames, buckets (1, 2, 4): every replay equals the
    eager engine within atol = rtol = 1e-3 (the rule of
    test_graphed_engine_matches_eager), and after three replays (padding rows,
    a one-clip video) every BatchNorm's running statistics match the fp64
    module's within tests/test_gpu_bn_state.py's 1e-3 / 2e-3 bounds."""
    from rnb_amd.models.r2p1d.engine import GraphedEngine, R2P1DEngine
    from rnb_amd.models.r2p1d.model import build_network
    from test_gpu_bn_state import sync_running
    net = build_network(1, 5, depth=10, seed=7)
    kw = dict(backend="hip", bn_mode="batch", dtype=torch.float32, clip_length=16)
    eng = R2P1DEngine(net, DEV, **kw)
    eager = R2P1DEngine(net, DEV, **kw)
    ref = Ref64(net, eng)
    g = GraphedEngine(eng, 4, buckets=(1, 2, 4), autotune=False)
    g.prepare()
    torch.cuda.synchronize()
    assert g.graphs[4][1].shape == (4, 16, 112, 112, 4)
    ref.load_running()
    sync_running(eager, eng)
    calls = [([(3, [0]), (5, [40, 80])], [0, 1, 3]),      # 3 clips in bucket 4
             ([(8, [16])], [0, 1]),                       # bucket 1
             ([(9, [0, 32])], [0, 2])]                    # bucket 2
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        for videos, offs in calls:
            x = torch.cat(_videos(16, videos))
            y = g.forward(x, clip_offsets=offs).clone()
            e = eager.forward(x, clip_offsets=offs)
            torch.cuda.synchronize()
            assert torch.allclose(y, e, atol=1e-3, rtol=1e-3)
            r = ref.forward(x, offs)
            scale = r.abs().max().item()
            assert (y.double().cpu() - r).abs().max().item() <= 1e-3 * scale
    assert eng.range_guard is None or not eng.range_guard.tripped()
    wm, wv = running_vs_ref(ref.pairs, "graph, 16 frames")
    print("16 frames graphed: running mean %.2e, var %.2e of the bound's scale" % (wm, wv))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("frames", [2, 4])
def test_head_over_longer_pooling_windows(frames, dtype):
    """The head pools S = T H W positions: 98 at 16-frame clips, 196 at 32
    (49 at 8). Three clips, C = 512, against torch's mean + linear at the
    bound of test_head_matches_torch."""
    from rnb_amd.ops import video as vops
    g = torch.Generator().manual_seed(frames)
    lin = torch.nn.Linear(512, 400)
    head = vops.Head(lin, DEV)
    x = torch.randn((3, frames, 7, 7, 512), generator=g).to(dtype).to(DEV)
    assert frames * 49 in (98, 196)
    y = head.forward(x)
    torch.cuda.synchronize()
    w, b = lin.weight.detach().to(DEV), lin.bias.detach().to(DEV)
    ref = x.float().mean(dim=(1, 2, 3)) @ w.t() + b
    assert torch.allclose(y, ref, atol=1e-4, rtol=1e-4)


def test_loader_into_runner_at_16_frames():
    """Loader and runner plugins in one process at 16 frames (synthetic
    decoder, depth 10): the runner's logits on the loader's own output equal
    an eager engine's of the same weights (graph replay vs eager: 1e-3), and
    no call fell back on the full-range kernels."""
    from rnb_amd.models.r2p1d.model import R2P1DLoader, R2P1DRunner, build_engine
    from rnb_amd.timecard import TimeCard
    kw = dict(depth=10, bn_mode="batch", dtype="fp32", clip_length=16)
    loader = R2P1DLoader(DEV, clip_length=16, dtype="fp32", warmup=1, seed=3,
                         num_clips_population=(1, 3), num_clips_weights=(1, 1), max_clips=4)
    runner = R2P1DRunner(DEV, warmup=1, max_clips=4, bucket_step=1, autotune=False, **kw)
    eager = build_engine(DEV, use_graphs=False, autotune=False, max_clips=4, **kw)
    assert runner.input_shape() == ((4, 16, 112, 112, 4),)
    assert R2P1DLoader.output_shape_for(max_clips=4, clip_length=16) == runner.input_shape()
    for i in range(3):
        tc = TimeCard(i)
        (frames,), _, tc = loader(None, "synthetic://%d?frames=300" % (40 + i), tc)
        assert frames.shape[0] == tc.num_clips and tuple(frames.shape[1:]) == (16, 112, 112, 4)
        (y,), _, _ = runner((frames,), None, tc)
        torch.cuda.synchronize()
        runner.on_complete(None)
        e = eager.forward(frames)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (frames.shape[0], 400)
        assert torch.allclose(y, e, atol=1e-3, rtol=1e-3)
    st = runner.runtime_stats()
    assert st.get("h3_range_fallbacks", 0) == 0, st


@pytest.mark.parametrize("clip_length,n", [(16, 3), (32, 2)])
def test_bf16_engine_matches_torch_plan_at_longer_clips(clip_length, n):
    """bf16 at 16 and 32 frames: the shape-specialised temporal kernel
    (csrc/conv_temporal.hip: compiled for T 8 / 4 / 2) declines and the
    generic kernels serve every conv. The rule of
    test_engine_hip_matches_torch_plan: the hip plan against the same folded
    plan through torch, and that against the unfolded fp32 module."""
    from rnb_amd.models.r2p1d.engine import R2P1DEngine
    from rnb_amd.models.r2p1d.model import build_network
    net = build_network(1, 5, depth=10, seed=3)
    hip, ref, mod = (R2P1DEngine(net, DEV, backend=b, clip_length=clip_length)
                     for b in ("hip", "torch", "module"))
    assert hip.dtype == torch.bfloat16
    g = torch.Generator().manual_seed(clip_length)
    x = torch.randn(hip.input_shape(n), generator=g).to(torch.bfloat16).to(DEV)
    x[..., 3:] = 0
    from rnb_amd.ops.native import kernels
    # stem and conv2 temporal at this T: no specialised variant
    assert kernels().temporal_lds_bytes(clip_length, 88, 64) < 0
    assert kernels().temporal_lds_bytes(clip_length, 144, 64) < 0
    assert kernels().temporal_lds_bytes(8, 144, 64) > 0
    y = hip.forward(x).float()
    r = ref.forward(x).float()
    m = mod.forward(x).float()
    torch.cuda.synchronize()
    scale = r.abs().max().item()
    assert (y - r).abs().max().item() <= 3e-2 * scale + 3e-2
    assert (r - m).abs().max().item() <= 5e-2 * scale + 5e-2


def test_default_clip_length_picks_the_same_configs():
    """clip_length=8 passed explicitly changes nothing: a depth-18 engine's
    chosen config id per layer and input shape (autotune off) and each layer's
    autotune candidate set equal those of an engine built without it."""
    from rnb_amd.models.r2p1d.engine import R2P1DEngine
    from rnb_amd.models.r2p1d.model import build_network
    net = build_network(1, 5, depth=18, seed=0)
    kw = dict(backend="hip", bn_mode="batch", dtype=torch.float32)
    a = R2P1DEngine(copy.deepcopy(net), DEV, **kw)
    b = R2P1DEngine(copy.deepcopy(net), DEV, clip_length=8, **kw)
    assert a.input_shape(3) == b.input_shape(3) == (3, 8, 112, 112, 4)

    def picks(eng):
        out, shapes = [], {"x": eng.input_shape(2)}
        for op in eng.ops:
            shape = shapes[op.src]
            out.append((op.layer.name, tuple(shape), op.layer.config_for(shape),
                        tuple(op.layer.candidates(shape))))
            shapes[op.dst] = op.layer.out_shape(shape)
        return out
    pa, pb = picks(a), picks(b)
    assert len(pa) == len(a.ops) and pa == pb
    assert a.flops_per_clip() == b.flops_per_clip()
