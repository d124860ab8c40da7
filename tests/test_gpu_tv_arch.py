"""``arch="torchvision"`` on the GPU: every conv geometry the new tree adds,
on every kernel config offered for it, against an fp64 conv; then whole
engines (weights of the independent oracle tests/tv_oracle.py, saved and
loaded through ``ckpt_path``) against the oracle in fp64, the module, the
torch plan and eager runs, and one launcher run of the shipped config."""
import json
import os

import pytest
import torch

import tv_oracle
from test_gpu_f32 import DEV, _input, _ref64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K111, K133, K311, K177 = (1, 1, 1), (1, 3, 3), (3, 1, 1), (1, 7, 7)
# name: (cin, cout, kernel, stride, padding, (T, H, W), clips, cin_pad, cout_pad) as the
# engine builds them (mid activations padded to 16 channels; a 3x1x1 conv over
# one frame runs as its centre tap)
GEOMS = {
    "shortcut64_odd": (64, 128, K111, (2, 2, 2), (0, 0, 0), (3, 7, 5), 2, 0, 0),
    "shortcut64_56": (64, 128, K111, (2, 2, 2), (0, 0, 0), (8, 56, 56), 1, 0, 0),
    "shortcut256": (256, 512, K111, (2, 2, 2), (0, 0, 0), (2, 14, 14), 2, 0, 0),
    "stem_spatial_112": (3, 45, K177, (1, 2, 2), (0, 3, 3), (2, 112, 112), 2, 0, 48),
    "stem_spatial_19x17": (3, 45, K177, (1, 2, 2), (0, 3, 3), (1, 19, 17), 2, 0, 48),
    "stem_spatial_30x112": (3, 45, K177, (1, 2, 2), (0, 3, 3), (2, 30, 112), 2, 0, 48),
    "stem_temporal_t8": (45, 64, K311, (1, 1, 1), (1, 0, 0), (8, 12, 8), 2, 48, 0),
    "stem_temporal_t16": (45, 64, K311, (1, 1, 1), (1, 0, 0), (16, 12, 8), 2, 48, 0),
    "spatial230_28": (128, 230, K133, (1, 1, 1), (0, 1, 1), (2, 28, 28), 2, 0, 240),
    "spatial230_15x13": (128, 230, K133, (1, 1, 1), (0, 1, 1), (1, 15, 13), 2, 0, 240),
    "temporal230": (230, 128, K311, (1, 1, 1), (1, 0, 0), (4, 28, 28), 2, 240, 0),
    "temporal921_t1": (921, 512, K111, (1, 1, 1), (0, 0, 0), (1, 7, 7), 2, 928, 0),
}


# Integer weights are multiples of 24. "Bit-exact on small integers" asks that
# every intermediate of a kernel be exactly representable, so that any
# difference is an indexing or accumulation fault and not rounding. The
# Winograd candidates transform the weights on the host: F(2x2, 3x3) divides
# them by up to 4, the temporal F(4, 3) (points 0, +-1, +-2, inf) by 4, 6, 12 and
# 24 -- with weights in {-2..2} the transformed weights are not binary
# fractions and the fp64 conv is matched only to rounding (measured on this
# test's first version: 9e-5 .. 6e-4 absolute on outputs of a few hundred, on
# the four temporal Winograd ids alone). With multiples of lcm(4, 6, 12, 24) =
# 24 every transformed weight is an integer, the input and output transforms
# have integer coefficients, and every partial sum stays below 2^24 (largest
# here: K = 928 x 48 x 3 < 2^18 direct; x 10 x 20 through the F(4, 3)
# transforms at K = 240 < 2^22). 24 = 3 x 2^3 and 48 = 3 x 2^4 are exact in the
# fp16 and bf16 parts of the split kernels.
INT_W_STEP = 24


def _tv_layer(case, relu=True, integer=False, seed=0):
    from rnb_amd.ops.conv import ConvGeom
    from rnb_amd.ops.conv_f32 import F32_ALIGN, ConvLayerF32
    cin, cout, k, s, p, _, _, cin_pad, cout_pad = case
    g = torch.Generator().manual_seed(seed)
    if integer:
        w = INT_W_STEP * torch.randint(-2, 3, (cout, cin) + k, generator=g).float()
        b = torch.randint(-4, 5, (cout,), generator=g).float()
    else:
        w = torch.randn((cout, cin) + k, generator=g) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
    geom = ConvGeom(cin=cin, cout=cout, kernel=k, stride=s, padding=p, align=F32_ALIGN,
                    cin_pad=cin_pad, cout_pad=cout_pad)
    return ConvLayerF32(w, b, geom, relu, DEV, "tvtest")


def _stats_capable(cid):
    from rnb_amd.ops.conv_f32 import WINO_ALL, is_x6d
    return cid in WINO_ALL or is_x6d(cid)


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_every_candidate_of_every_new_geometry(name):
    """Every id of ``candidates(x_shape)``: bit-exact on small integers (with a
    residual and ReLU), within 1e-5 of the fp64 conv on normal data, pad
    channels zero; where the config takes them, the producer's BN + ReLU on
    load (within 1e-5 of the fp64 conv of the applied input) and the per-video
    epilogue sums (against fp64 sums of the stored output, the bounds of
    tests/test_gpu_h3.py). The stem's 45 (48) channels go to the 48-channel
    h3stem variants only."""
    from rnb_amd.ops.conv_f32 import H3STEM_BASE, is_h3stem
    from rnb_amd.ops.native import kernels
    case = GEOMS[name]
    cin, cout, k, s, p, thw, n, _, _ = case
    li, lf = _tv_layer(case, integer=True), _tv_layer(case, relu=False)
    cin_p, cout_p = li.geom.cin_p, li.geom.cout_p
    xi = _input(n, thw, cin_p, cin, integer=True)
    oshape = li.out_shape(xi.shape)
    res = _input(n, tuple(oshape[1:4]), cout_p, cout, integer=True, seed=3)
    ref_i = _ref64(li, xi, res).float().to(DEV)
    xf = _input(n, thw, cin_p, cin)
    ref_f = _ref64(lf, xf).to(DEV)
    scale = ref_f.abs().max().item()
    ids = li.candidates(xi.shape)
    assert ids == lf.candidates(xf.shape) and len(ids) == len(set(ids))
    if k == K177:
        tiles = [kernels().conv_h3stem_ctile(c - H3STEM_BASE) for c in ids if is_h3stem(c)]
        assert tiles and all(t == 48 for t in tiles), tiles
    # BN + ReLU on load: two videos, per-video scale / shift
    g = torch.Generator().manual_seed(5)
    seg = torch.tensor([0] * (n // 2) + [1] * (n - n // 2), dtype=torch.int32, device=DEV)
    ss = torch.empty((2, 2, cin_p), dtype=torch.float32)
    ss[:, 0] = torch.rand((2, cin_p), generator=g) + 0.5
    ss[:, 1] = torch.randn((2, cin_p), generator=g) * 0.5
    ss[:, :, cin:] = 0                      # pad channels: gamma = beta = 0
    ss = ss.to(DEV)
    xa = torch.relu(xf * ss[seg.long(), 0][:, None, None, None, :]
                    + ss[seg.long(), 1][:, None, None, None, :])
    ref_a = _ref64(lf, xa).to(DEV)
    scale_a = ref_a.abs().max().item()
    bounds = [(a, b) for a, b in ((0, n // 2), (n // 2, n))]
    worst = {}
    failures = []
    for cid in ids:
        y = li.forward_hip(xi, res, config=cid)
        if not torch.equal(y[..., :cout], ref_i):
            d = (y[..., :cout] - ref_i).abs().max().item()
            failures.append("cid %d: integers differ by up to %.3e" % (cid, d))
        if not torch.all(y[..., cout:] == 0):
            failures.append("cid %d: pad channels not zero (integers)" % cid)
        stats = _stats_capable(cid)
        sums = torch.zeros((2, 2, cout_p), dtype=torch.float64, device=DEV)
        y = lf.forward_hip(xf, config=cid, out_stats=(sums, seg) if stats else None)
        err = (y[..., :cout].double() - ref_f).abs().max().item() / scale
        worst[cid] = err
        if err > 1e-5:
            failures.append("cid %d: rel err %.3e > 1e-5" % (cid, err))
        if not torch.all(y[..., cout:] == 0):
            failures.append("cid %d: pad channels not zero" % cid)
        if stats:
            yd = y[..., :cout].double()
            for v, (a, b) in enumerate(bounds):
                part = yd[a:b].reshape(-1, cout)
                got = sums[v, :, :cout]
                tol1 = 1e-6 * part.abs().sum(0) + 1e-9
                if not ((got[0] - part.sum(0)).abs() <= tol1).all():
                    failures.append("cid %d: epilogue sums of video %d" % (cid, v))
                if not torch.allclose(got[1], (part * part).sum(0), rtol=1e-6, atol=1e-9):
                    failures.append("cid %d: epilogue square sums of video %d" % (cid, v))
        if lf.affine_ok(cid, xf.shape):
            for ost in ((None,) if not stats else (None, (sums.zero_(), seg))):
                y = lf.forward_hip(xf, config=cid, in_affine=(ss, seg), out_stats=ost)
                err = (y[..., :cout].double() - ref_a).abs().max().item() / scale_a
                worst[("aff", cid)] = max(worst.get(("aff", cid), 0.0), err)
                if err > 1e-5:
                    failures.append("cid %d: BN on load rel err %.3e > 1e-5" % (cid, err))
    torch.cuda.synchronize()
    print("%s: %d ids, worst rel err %.3e (cid %s), BN on load on %d ids worst %.3e"
          % (name, len(ids), max(v for c, v in worst.items() if not isinstance(c, tuple)),
             max((c for c in worst if not isinstance(c, tuple)), key=lambda c: worst[c]),
             sum(1 for c in worst if isinstance(c, tuple)),
             max([v for c, v in worst.items() if isinstance(c, tuple)] or [0.0])))
    for f in failures:
        print("  FAIL", name, f)
    assert not failures, failures[:8]


# ---------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------
def _ckpt(tmp_path, depth, rule, eps, seed=9):
    ora = tv_oracle.make(depth, mid_rule=rule, bn_eps=eps, seed=seed)
    path = str(tmp_path / ("tv%d_%s.pt" % (depth, rule)))
    torch.save(ora.state_dict(), path)
    return ora, path


def _engine(path, depth, eps, **kw):
    from rnb_amd.models.r2p1d.model import build_engine
    return build_engine(DEV, depth=depth, arch="torchvision", ckpt_path=path, bn_eps=eps,
                        autotune=False, **kw)


def _clips32(videos):
    from rnb_amd.models.r2p1d.decoder import SyntheticDecoder
    dec = SyntheticDecoder(DEV, dtype=torch.float32)
    return [dec.decode(vid, starts) for vid, starts in videos]


@pytest.mark.parametrize("depth,rule,eps", [(18, "block", 1e-5), (18, "conv", 1e-5),
                                            (34, "conv", 1e-3)])
def test_fp32_eval_engine_vs_fp64_oracle(tmp_path, depth, rule, eps):
    """Published-weights numerics (running statistics folded): the HIP plan on
    3 clips is as close to the oracle in fp64 as PyTorch's own fp32 module is,
    within a factor 3 (the rule of test_batch_bn_fp32_error_vs_fp64)."""
    from rnb_amd.ops.video import ndhwc_to_ncdhw
    ora, path = _ckpt(tmp_path, depth, rule, eps)
    hip = _engine(path, depth, eps, bn_mode="eval", dtype="fp32", use_graphs=False)
    mod = _engine(path, depth, eps, bn_mode="eval", dtype="fp32", backend="module")
    assert hip.backend == "hip" and hip.arch == "torchvision"
    if rule == "conv":
        assert hip.net.layer2[0].conv2[0][0].out_channels == 288
    (x,) = _clips32([(31, [0, 80, 160])])
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        y = hip.forward(x).double().cpu()
        ym = mod.forward(x).double().cpu()
        y64 = ora.double()(ndhwc_to_ncdhw(x, 3).double().cpu())
    scale = y64.abs().max().item()
    e_hip = (y - y64).abs().max().item() / scale
    e_mod = (ym - y64).abs().max().item() / scale
    print("tv%d %s eval fp32 vs fp64: HIP %.2e, PyTorch fp32 module %.2e" % (depth, rule, e_hip,
                                                                              e_mod))
    assert e_hip <= 3 * e_mod + 1e-6, (e_hip, e_mod)


def test_graphed_batch_bn_per_video_vs_module(tmp_path):
    """'batch' stays available and graphed at fp32: videos of 1 + 1 + 3 clips
    in buckets [5, 8] against the module run once per video, within 5e-4 of
    the logit scale (the project's bound for this comparison)."""
    from rnb_amd.models.r2p1d.engine import GraphedEngine
    _, path = _ckpt(tmp_path, 18, "block", 1e-5)
    g = _engine(path, 18, 1e-5, bn_mode="batch", dtype="fp32", max_clips=8, buckets=[5, 8])
    assert isinstance(g, GraphedEngine) and g.batch_bn
    mod = _engine(path, 18, 1e-5, bn_mode="batch", dtype="fp32", backend="module")
    xs = _clips32([(21, [30]), (22, [100]), (23, [0, 90, 180])])
    with torch.no_grad():
        y = g.forward(torch.cat(xs), clip_offsets=[0, 1, 2, 5]).clone()
        ref = torch.cat([mod.forward(x) for x in xs])
    torch.cuda.synchronize()
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    print("tv18 graphed batch BN vs per-video module: %.2e" % err)
    assert err <= 5e-4, err


def test_bf16_eval_engine_vs_torch_plan(tmp_path):
    _, path = _ckpt(tmp_path, 18, "block", 1e-5)
    hip = _engine(path, 18, 1e-5, bn_mode="eval", dtype="bf16", use_graphs=False)
    ref = _engine(path, 18, 1e-5, bn_mode="eval", dtype="bf16", backend="torch")
    x = torch.randn(hip.input_shape(3), device=DEV).to(torch.bfloat16)
    x[..., 3:] = 0
    y, r = hip.forward(x).float(), ref.forward(x).float()
    torch.cuda.synchronize()
    scale = r.abs().max().item()
    err = (y - r).abs().max().item()
    print("tv18 bf16 hip vs torch plan: %.3e of scale %.3e" % (err, scale))
    assert err <= 3e-2 * scale + 3e-2


def test_graph_replay_matches_eager_and_repeats_bit_equal(tmp_path):
    from rnb_amd.models.r2p1d.engine import GraphedEngine
    _, path = _ckpt(tmp_path, 18, "block", 1e-5)
    hip = _engine(path, 18, 1e-5, bn_mode="eval", dtype="fp32", use_graphs=False)
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


def test_launcher_serves_the_tv18_config(tmp_path):
    """configs/r2p1d-whole-tv18.json through the launcher on GPU 0 (untuned
    kernels: the new shapes have no seed-table entries)."""
    from test_pipeline_e2e import run_cfg
    cfg = json.loads(open(os.path.join(ROOT, "configs", "r2p1d-whole-tv18.json")).read())
    proc, res, _ = run_cfg(tmp_path, cfg, "-v", "8", "-mi", "0", "--set", "autotune=false",
                           "--set", "num_clips_population=[1,3]",
                           "--set", "num_clips_weights=[2,1]", "--set", "max_clips=3",
                           "--set", "warmup=1", timeout=300)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert res["termination_flag"] == "TARGET_NUM_VIDEOS_REACHED" and res["videos_done"] >= 8
