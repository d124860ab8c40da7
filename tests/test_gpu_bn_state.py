"""BatchNorm state of the graphed fp32 batch-BN engine against an fp64 module.

The convolutions of the headline path are held to 1e-5 of an fp64 conv
elsewhere; this file checks the state around them: the running statistics
after a sequence of bucket-graph replays (every running-update route, with
bucket padding and empty videos), the per-video epilogue sums and running
accumulators re-armed after every use, the consumer-side scale / shift rows
(csrc/x6d_common.h BnAffSums) under graphs, and the from-sums finalize kernels
on badly centred data. The reference is a deep copy of the network in fp64,
training mode, on the CPU, run once per video in video order -- what the
reference project's one-video forwards do.
"""
import copy

import pytest
import torch

from test_gpu_f32 import DEV, _layer

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
_SUFFIX = {
    ("conv1", "spatial"): lambda blk: blk.conv1.bn,
    ("conv1", "temporal"): lambda blk: blk.bn1,
    ("conv2", "spatial"): lambda blk: blk.conv2.bn,
    ("conv2", "temporal"): lambda blk: blk.bn2,
    ("downsample", "spatial"): lambda blk: blk.downsampleconv.bn,
    ("downsample", "temporal"): lambda blk: blk.downsamplebn,
}


def bn_pairs(eng, net):
    """[(engine BatchNormBatch, module BatchNorm3d)] by the plan ops' layer
    names; every BatchNorm3d of ``net`` is matched exactly once."""
    body = net.res2plus1d
    pairs = []
    for op in eng.ops:
        if op.bn is None:
            continue
        parts = op.layer.name.split(".")
        if len(parts) == 2:                       # the stem: conv1.spatial
            assert parts == ["conv1", "spatial"], op.layer.name
            mod = body.conv1.bn
        else:
            blk = body.get_submodule(".".join(parts[:-2]))
            mod = _SUFFIX[(parts[-2], parts[-1])](blk)
        assert mod.num_features == op.bn.channels, op.layer.name
        pairs.append((op.bn, mod))
    mods = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    assert len(pairs) == len(mods)
    assert {id(m) for _, m in pairs} == {id(m) for m in mods}
    assert len({id(b) for b, _ in pairs}) == len(pairs)
    return pairs


class Ref64:
    """fp64 training-mode copy of ``net`` on the CPU, one forward per video."""

    def __init__(self, net, eng):
        self.net = copy.deepcopy(net).double().train()
        self.pairs = bn_pairs(eng, self.net)
        self.cin = eng.ops[0].layer.geom.cin

    def load_running(self):
        """The engine BNs' running statistics into the module's buffers."""
        with torch.no_grad():
            for b, m in self.pairs:
                m.running_mean.copy_(b.running_mean.double().cpu())
                m.running_var.copy_(b.running_var.double().cpu())

    def forward(self, x, offs):
        from rnb_amd.ops.video import ndhwc_to_ncdhw
        xin = ndhwc_to_ncdhw(x, self.cin).double().cpu()
        outs = []
        with torch.no_grad():
            for a, b in zip(offs[:-1], offs[1:]):
                if b > a:
                    outs.append(self.net(xin[a:b]))
        return torch.cat(outs)


def sync_running(dst_eng, src_eng):
    """In place: dst's BN running statistics := src's."""
    dst = [op.bn for op in dst_eng.ops if op.bn is not None]
    src = [op.bn for op in src_eng.ops if op.bn is not None]
    assert len(dst) == len(src)
    for d, s in zip(dst, src):
        d.running_mean.copy_(s.running_mean)
        d.running_var.copy_(s.running_var)


def running_vs_ref(pairs, what):
    """Asserts every BN's running statistics against the fp64 module's at the
    engine bound (1e-3 of the activation scale for the mean, twice that of the
    largest variance for the variance); returns the largest relative errors."""
    worst_m = worst_v = 0.0
    for i, (b, m) in enumerate(pairs):
        rm, rv = b.running_mean.double().cpu(), b.running_var.double().cpu()
        assert torch.isfinite(rm).all() and torch.isfinite(rv).all(), (what, i)
        s = m.running_mean.abs().max().item() + m.running_var.max().item() ** 0.5
        dm = (rm - m.running_mean).abs().max().item()
        dv = (rv - m.running_var).abs().max().item()
        worst_m = max(worst_m, dm / s)
        worst_v = max(worst_v, dv / m.running_var.max().item())
        assert dm <= 1e-3 * s, (what, i, dm, s)
        assert dv <= 2e-3 * m.running_var.max().item(), (what, i, dv, m.running_var.max().item())
    return worst_m, worst_v


def running_vs_engine(eng_a, eng_b, what):
    a = [op.bn for op in eng_a.ops if op.bn is not None]
    b = [op.bn for op in eng_b.ops if op.bn is not None]
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.allclose(p.running_mean, q.running_mean, rtol=1e-5, atol=1e-6), (what, i)
        assert torch.allclose(p.running_var, q.running_var, rtol=1e-5, atol=1e-6), (what, i)


class AffArmWatch:
    """Counts kernels().bn_aff_arm / bn_aff_disarm (host-global state read by
    the launches of the armed conv) and tracks whether it is left armed."""

    def __init__(self, monkeypatch):
        from rnb_amd.ops.native import kernels
        k = kernels()
        self.arms, self.armed = 0, False
        arm, disarm = k.bn_aff_arm, k.bn_aff_disarm

        def w_arm(*a):
            self.arms += 1
            self.armed = True
            return arm(*a)

        def w_disarm():
            self.armed = False
            return disarm()
        monkeypatch.setattr(k, "bn_aff_arm", w_arm)
        monkeypatch.setattr(k, "bn_aff_disarm", w_disarm)


def assert_state_rearmed(eng, nseg, watch=None):
    """After a forward: every BN's epilogue sums and running accumulators are
    zero again, and no consumer-side rows are armed or marked used."""
    from rnb_amd.ops.native import kernels
    torch.cuda.synchronize()
    for i, op in enumerate(eng.ops):
        if op.bn is None:
            continue
        if getattr(op.bn, "_esums", None) is not None:
            assert float(op.bn.epilogue_sums(nseg, DEV).abs().sum()) == 0.0, ("sums", i)
            assert float(op.bn._esums.abs().sum()) == 0.0, ("sums buffer", i)
        acc = getattr(op.bn, "_run_acc", None)
        if acc is not None:
            assert float(acc.abs().sum()) == 0.0, ("run_acc", i)
    assert not kernels().bn_aff_used()
    if watch is not None:
        assert not watch.armed


def _clips(n, seed, cin_p=128, cin=128):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 4, 28, 28, cin_p), generator=g)
    x[..., cin:] = 0
    return x.to(DEV)


# ------------------------------------- A. replay sequences, one per route
# (clips, clip offsets) per replay of the one bucket graph; >= 3 replays and
# >= 8 one-clip videos per sequence (49 rows per clip at conv5: a missing
# n / (n - 1) moves running_var by 2 % per step)
SEQUENCES = {
    1: [(1, [0, 1])] * 8,
    4: [(3, [0, 1, 3]), (4, [0, 3, 4, 4]), (2, [0, 2]), (4, [0, 1, 2, 3, 4]),
        (3, [0, 1, 2, 3])],
    24: [(19, [0, 1, 2, 3, 4, 19]), (24, [0, 1, 2, 3, 4, 12, 24]), (17, [0, 17])],
    40: [(35, [0, 1, 2, 10, 35]), (40, list(range(41))), (2, [0, 2])],
}


def _run_entries(eng):
    """(entries with epilogue sums, bare entries) of the batched running
    update tables this engine's forwards built."""
    with_sums = bare = 0
    for key in getattr(eng, "_run_tables", {}):
        with_sums = max(with_sums, sum(1 for _, p, _ in key if p))
        bare = max(bare, sum(1 for _, p, _ in key if not p))
    return with_sums, bare


# environment read at capture time: "finalize" leaves each BN's statistics
# and running update to the finalize kernels chosen by the segment count
# (rnb_bn_seg_stats_from_sums_f32) instead of the default ss-only finalize /
# apply-from-sums + batched running update
ROUTE_ENV = {
    "batched": {},
    "finalize": {"RNB_BN_SS_ONLY": "0", "RNB_BN_APPLY_SUMS": "0"},
}


@pytest.mark.parametrize("bucket", sorted(SEQUENCES))
@pytest.mark.parametrize("route", sorted(ROUTE_ENV))
def test_graphed_replay_sequence_running_stats_match_fp64(route, bucket, monkeypatch):
    """R(2+1)D-18 layers 4-5 (20 BatchNorms), one bucket graph replayed over a
    sequence of calls with padding rows, empty and one-clip videos: logits
    after every replay against the fp64 module (1e-3) and the eager engine
    (1e-5; nseg = videos there and default switches: another BN route);
    running statistics of every BN at the end against the fp64 module's and
    the eager engine's; epilogue sums, running accumulators and the
    consumer-side arming left clear.

    The graph's segment count is the bucket size b. Route "batched" (the
    default switches): every BN is fed from epilogue sums, its rows come from
    the ss-only finalize, the apply-from-sums kernel or (b = 1) the consuming
    conv, and bn_seg_running_batched_kernel walks the sums. Route "finalize":
    b = 1 consumer-side rows plus walk + apply in one dispatch, b <= 16 the
    in-order walk, 17-32 bn_seg_finalize_running_f32_kernel, > 32 the split
    finalize plus the batched kernel on its accumulators.

    Measured on MI355X, largest over the BNs and buckets, relative to the
    bounds' scales (profiles/NOTES.md): running mean 1.6e-7 (bound 1e-3),
    running var 8.6e-7 (bound 2e-3), logits 1.3e-6 vs fp64, 1.2e-6 vs eager."""
    from rnb_amd.models.r2p1d.engine import GraphedEngine, R2P1DEngine
    from rnb_amd.models.r2p1d.model import build_network
    from rnb_amd.ops.native import kernels
    seq = SEQUENCES[bucket]
    assert len(seq) >= 3 and sum(
        sum(1 for a, b in zip(o[:-1], o[1:]) if b - a == 1) for _, o in seq) >= 8
    net = build_network(4, 5, depth=18, seed=7)
    eng = R2P1DEngine(net, DEV, backend="hip", bn_mode="batch", dtype=torch.float32)
    eager = R2P1DEngine(net, DEV, backend="hip", bn_mode="batch", dtype=torch.float32)
    ref = Ref64(net, eng)
    assert len(ref.pairs) == 20
    watch = AffArmWatch(monkeypatch)
    g = GraphedEngine(eng, bucket, buckets=(bucket,), autotune=False)
    env = dict(ROUTE_ENV[route])
    if route == "finalize" and bucket == 1:
        env["RNB_BN_WALK_APPLY"] = "1"
    k = kernels()
    with monkeypatch.context() as mp:
        for name, val in env.items():
            mp.setenv(name, val)
        g.prepare()
        torch.cuda.synchronize()
    assert g.offsets[bucket].numel() == bucket + 1      # nseg of the graph = bucket size
    # the route taken
    k.bn_seg_set_defer_running(True)
    try:
        defers = [bool(k.bn_seg_defers_running(bucket, s)) for s in (1, 0)]
    finally:
        k.bn_seg_set_defer_running(False)
    with_sums, bare = _run_entries(eng)
    aff = getattr(eng, "bn_aff_sums", 0)
    tickets = sum(1 for op in eng.ops if op.bn is not None and hasattr(op.bn, "_ticket"))
    print("%s bucket %d: bn_aff_sums %d, arms %d, running table: %d from sums + %d bare, "
          "walk + apply BNs %d, defers %s" % (route, bucket, aff, watch.arms, with_sums, bare,
                                              tickets, defers))
    # 17-32: the fused finalize + running kernel must run; > 32: the split
    # finalize leaves the update to the batched kernel
    assert defers == [bucket > 32, bucket > 32]
    if bucket == 1:
        assert aff > 0 and watch.arms == aff and aff % 2 == 0     # warm-up + capture
    else:
        assert aff == 0 and watch.arms == 0
    if route == "batched":
        assert (with_sums, bare) == (20, 0)
        assert tickets == 0
    elif bucket == 1:
        assert (with_sums, bare) == (aff // 2, 0)     # the consumer-side BNs only
        assert 0 < tickets <= 20 - aff // 2           # applied BNs: walk + apply
    elif bucket <= 32:
        assert (with_sums, bare) == (0, 0)            # walk / fused finalize + running
    else:
        assert (with_sums, bare) == (0, 20)           # finalize accumulators, batched kernel
    assert_state_rearmed(eng, bucket, watch)
    armed_at_capture = getattr(eng, "bn_aff_sums", 0)

    ref.load_running()
    sync_running(eager, eng)
    worst_ref = worst_eager = 0.0
    with torch.no_grad():
        for i, (n, offs) in enumerate(seq):
            x = _clips(n, 100 * bucket + i)
            y = g.forward(x, clip_offsets=offs).clone()
            e = eager.forward(x, clip_offsets=offs)
            torch.cuda.synchronize()
            r = ref.forward(x, offs)
            scale = r.abs().max().item()
            d_ref = (y.double().cpu() - r).abs().max().item()
            d_eager = (y - e).abs().max().item()
            worst_ref, worst_eager = max(worst_ref, d_ref / scale), max(worst_eager,
                                                                        d_eager / scale)
            assert y.shape[0] == n and torch.isfinite(y).all()
            assert d_ref <= 1e-3 * scale, (i, d_ref, scale)
            assert d_eager <= 1e-5 * scale, (i, d_eager, scale)
    assert not eng.range_guard.tripped()
    wm, wv = running_vs_ref(ref.pairs, "graph")
    print("%s bucket %d: logits vs fp64 %.2e, vs eager %.2e; running mean %.2e, var %.2e "
          "of the bound's scale" % (route, bucket, worst_ref, worst_eager, wm, wv))
    running_vs_engine(eng, eager, "graph vs eager")
    assert_state_rearmed(eng, bucket, watch)
    assert_state_rearmed(eager, 1)
    # replays arm nothing; every arming is counted by the engine that did it
    assert getattr(eng, "bn_aff_sums", 0) == armed_at_capture
    assert armed_at_capture + getattr(eager, "bn_aff_sums", 0) == watch.arms


# ---------------------------- B. consumer-side BN rows under bucket graphs
def test_graphed_consumer_side_bn_rows_match_finalize_and_fp64(monkeypatch):
    """R(2+1)D-34 layers 4-5, bucket-1 graph: the deferred BNs whose rows the
    consuming h3 direct conv computes from the producer's sums (on by default,
    armed through host-global state at capture time) against the same engine
    built with RNB_BN_AFF_SUMS_MAX=0 (finalize dispatch) -- logits and running
    statistics over three replays -- and against the fp64 module; a bucket-2
    graph of the same engine (two one-clip videos) must not engage the path."""
    from rnb_amd.models.r2p1d.engine import GraphedEngine, R2P1DEngine
    from rnb_amd.models.r2p1d.model import build_network
    net = build_network(4, 5, depth=34, seed=11)

    def build(aff):
        if not aff:
            monkeypatch.setenv("RNB_BN_AFF_SUMS_MAX", "0")
        try:
            eng = R2P1DEngine(net, DEV, backend="hip", bn_mode="batch", dtype=torch.float32)
            g = GraphedEngine(eng, 2, buckets=(1, 2), autotune=False)
            g.prepare(sizes=[1])
            torch.cuda.synchronize()
        finally:
            monkeypatch.delenv("RNB_BN_AFF_SUMS_MAX", raising=False)
        return eng, g

    eng0, g0 = build(False)
    assert getattr(eng0, "bn_aff_sums", 0) == 0
    watch = AffArmWatch(monkeypatch)
    eng1, g1 = build(True)
    c1 = getattr(eng1, "bn_aff_sums", 0)
    print("bucket 1: %d consumer-side BN rows per forward x (warm-up + capture)" % c1)
    assert c1 > 0 and watch.arms == c1 and not watch.armed
    ref = Ref64(net, eng1)
    ref.load_running()
    sync_running(eng0, eng1)
    with torch.no_grad():
        for i in range(3):
            x = _clips(1, 40 + i)
            a = g1.forward(x).clone()
            b = g0.forward(x).clone()
            torch.cuda.synchronize()
            r = ref.forward(x, [0, 1])
            scale = r.abs().max().item()
            assert (a - b).abs().max().item() <= 1e-5 * scale + 1e-6, i
            assert (a.double().cpu() - r).abs().max().item() <= 1e-3 * scale, i
    running_vs_engine(eng1, eng0, "aff sums on vs off")
    running_vs_ref(ref.pairs, "bucket 1")
    assert getattr(eng1, "bn_aff_sums", 0) == c1          # replays arm nothing
    assert_state_rearmed(eng1, 1, watch)
    # two videos: RNB_BN_AFF_SUMS_VIDEOS=1 keeps the path off
    g1.prepare(sizes=[2])
    torch.cuda.synchronize()
    assert getattr(eng1, "bn_aff_sums", 0) == c1 and watch.arms == c1
    ref.load_running()
    with torch.no_grad():
        x = _clips(2, 50)
        a = g1.forward(x, clip_offsets=[0, 1, 2]).clone()
        torch.cuda.synchronize()
        r = ref.forward(x, [0, 1, 2])
    assert (a.double().cpu() - r).abs().max().item() <= 1e-3 * r.abs().max().item()
    running_vs_ref(ref.pairs, "bucket 2")
    assert_state_rearmed(eng1, 2, watch)


# --------------------- D. BN statistics on badly centred data, kernel level
D_OFFS = [0, 1, 3, 5, 5]                      # clips per video 1, 2, 2, 0
D_SEG = [0, 1, 1, 2, 2]                       # video of each clip


def _centred_layer(kind, r, x):
    """A 64 -> 144 1x3x3 or 144 -> 64 3x1x1 conv whose bias is r times the
    per-channel standard deviation of its bias-free output on ``x`` (fp64),
    so the output has |mean| / std ~ r per channel."""
    import torch.nn.functional as F
    from rnb_amd.ops.conv_f32 import ConvLayerF32, f32_geom
    cin, cout, k, p = ((64, 144, (1, 3, 3), (0, 1, 1)) if kind == "spatial"
                       else (144, 64, (3, 1, 1), (1, 0, 0)))
    w = _layer(cin, cout, k, (1, 1, 1), p, relu=False, seed=3).w_ref.cpu()
    y0 = F.conv3d(x[..., :cin].double().cpu().permute(0, 4, 1, 2, 3), w.double(), None,
                  padding=p)
    std = y0.permute(0, 2, 3, 4, 1).reshape(-1, cout).std(0)
    bias = (r * std).float()
    return ConvLayerF32(w, bias, f32_geom(cin, cout, k, (1, 1, 1), p), False, DEV, "bnstate")


def _producers(kind, layer, shape):
    """{family: config id}: one config of each producer family of this conv
    kind that accumulates BN sums in its epilogue."""
    from rnb_amd.ops import conv_f32 as c
    from rnb_amd.ops.native import kernels
    k = kernels()
    if kind == "spatial":
        fam = {"x6 direct": c.X6D_BASE, "h3 direct": c.H3D_BASE + 2,
               "h3w": c.H3W_BASE, "wino spatial": c.WINO_DEFAULT}
        assert layer.h3r_ok(shape)
        fam["h3 row band"] = next(c.H3R_BASE + i for i in range(k.h3r_variants)
                                  if layer.h3r_fits(i, shape))
        fam["split-K"] = next(c.X6K_BASE + j for j in range(len(c.X6K_CONFIGS))
                              if layer.ksplit_for(c.X6K_BASE + j, shape) > 1)
    elif kind == "temporal":
        assert layer.h3t_ok(shape)
        fam = {"wino temporal": c.WINOT_DEFAULT,
               "h3t": next(c.H3T_BASE + v for v in range(k.h3t_variants)
                           if layer.h3t_fits(v, shape))}
    else:                                       # the h3p kernel's shape: T 8, H W % 16 == 0
        assert layer.h3p_ok(shape)
        fam = {"h3p": c.H3P_BASE}
    return fam


def _bn_ref64(y, bn, res, relu, offs, rm0, rv0):
    """fp64 per-video training-mode BN of the stored output + residual + ReLU,
    and the running statistics after the videos' EMA steps in order."""
    C = bn.num_features
    yd = y[..., :C].double().cpu()
    out = torch.zeros_like(yd)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    g, b = bn.weight.detach().double(), bn.bias.detach().double()
    for a, e in zip(offs[:-1], offs[1:]):
        if e == a:
            continue
        part = yd[a:e].reshape(-1, C)
        mu, va = part.mean(0), part.var(0, unbiased=False)
        out[a:e] = (yd[a:e] - mu) / torch.sqrt(va + bn.eps) * g + b
        n = part.shape[0]
        rm = (1 - bn.momentum) * rm + bn.momentum * mu
        rv = (1 - bn.momentum) * rv + bn.momentum * va * n / (n - 1)
    if res is not None:
        out = out + res[..., :C].double().cpu()
    if relu:
        out = out.clamp(min=0)
    return out, rm, rv


def _make_bn(C, seed):
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm3d(C)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
    return bn


def _check_bn(tag, op, z, bn, ref, rm, rv, tol):
    """z and op's running statistics against the fp64 reference at ``tol``
    (relative to the largest |ref|; the running variance at twice that)."""
    C = bn.num_features
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    err = (z[..., :C].double().cpu() - ref).abs().max().item()
    s = rm.abs().max().item() + rv.max().item() ** 0.5
    dm = (op.running_mean.double().cpu() - rm).abs().max().item()
    dv = (op.running_var.double().cpu() - rv).abs().max().item()
    print("%-46s out %.2e  run mean %.2e  run var %.2e  (bound %.1e)"
          % (tag, err / scale, dm / s, dv / rv.max().item(), tol))
    assert err <= tol * scale, (tag, err, scale)
    assert dm <= tol * s, (tag, dm, s)
    assert dv <= 2 * tol * rv.max().item(), (tag, dv, rv.max().item())
    return err / scale


def _d_input(kind):
    shape = {"spatial": (5, 4, 14, 14, 64), "temporal": (5, 4, 14, 14, 144),
             "h3p": (5, 8, 4, 4, 144)}[kind]
    g = torch.Generator().manual_seed(21)
    return torch.randn(shape, generator=g).to(DEV)


@pytest.mark.parametrize("r", [0, 16, 256])
def test_bn_stats_pass_badly_centred(r):
    """The statistics pass (shifted sums; forward_hip(sums=None)) on a conv
    output with |mean| / std = r per channel: output and running statistics
    within 1e-4 of the fp64 BN of the stored output, independent of r."""
    from rnb_amd.ops.bn import BatchNormBatch
    x = _d_input("spatial")
    layer = _centred_layer("spatial", r, x)
    y = layer.forward_hip(x)
    thw = y.shape[1] * y.shape[2] * y.shape[3]
    res = torch.randn(y.shape, generator=torch.Generator().manual_seed(22)).to(DEV)
    bn = _make_bn(layer.geom.cout, 5)
    seg = torch.tensor(D_OFFS, dtype=torch.int32, device=DEV)
    op = BatchNormBatch(bn, layer.geom.cout_p, DEV)
    ref, rm, rv = _bn_ref64(y, bn, res, True, D_OFFS, bn.running_mean, bn.running_var)
    z = op.forward_hip(y, res, True, segments=seg, rpc=thw)
    _check_bn("stats pass r=%d" % r, op, z, bn, ref, rm, rv, 1e-4)
    assert float(op._run_acc.abs().sum()) == 0.0


def _from_sums_routes():
    return ["walk+apply pair", "walk+apply one dispatch", "ss-only+apply+batched",
            "apply-from-sums+batched", "fused finalize-running (20 seg)",
            "split finalize+running (40 seg)"]


def _run_route(route, op, y, res, sums, seg, thw, monkeypatch):
    """One from-sums route of ops/bn.py on the producer's sums; returns z."""
    from rnb_amd.ops import bn as bn_mod
    from rnb_amd.ops.native import kernels
    k = kernels()
    if route in ("ss-only+apply+batched", "apply-from-sums+batched"):
        nseg = seg.numel() - 1
        k.bn_seg_set_defer_running(True)
        bn_mod._RUN_SINK[0] = []
        try:
            if route.startswith("ss-only"):
                z = op.forward_hip(y, res, True, segments=seg, sums=sums, rpc=thw)
            else:
                z = op.apply_from_sums(y, res, True, out=torch.empty_like(y), segments=seg,
                                       sums=sums, rpc=thw)
            ent = bn_mod._RUN_SINK[0]
            assert len(ent) == 1 and isinstance(ent[0], tuple)
            tab = bn_mod.running_update_table(ent, DEV)
            k.bn_seg_running_batched(tab.data_ptr(), 1, bn_mod.running_table_channels(ent),
                                     seg.data_ptr(), nseg,
                                     torch.cuda.current_stream(DEV).cuda_stream)
            torch.cuda.synchronize()
        finally:
            k.bn_seg_set_defer_running(False)
            bn_mod._RUN_SINK[0] = None
        return z
    with monkeypatch.context() as mp:
        if route == "walk+apply one dispatch":
            mp.setenv("RNB_BN_WALK_APPLY", "1")
        z = op.forward_hip(y, res, True, segments=seg, sums=sums, rpc=thw)
        torch.cuda.synchronize()
    if route == "walk+apply one dispatch":
        assert int(op._ticket.item()) == 0
    return z


@pytest.mark.parametrize("kind", ["spatial", "temporal", "h3p"])
def test_bn_from_sums_routes_badly_centred(kind, monkeypatch):
    """Every from-sums route (walk + apply as a pair and in one dispatch, the
    ss-only finalize and the apply-from-sums kernel with the batched running
    update, the fused finalize + running kernel at 20 segments and the split
    finalize + running kernels at 40, both by padding the offsets with empty
    videos) fed the epilogue sums of one config of every producer family (x6
    direct, h3 direct, h3 row band, h3w, fp32 Winograd spatial, split-K;
    fp32 Winograd temporal, h3t; h3p at its own 8-frame shape), on conv
    outputs with |mean| / std = r in {0, 4, 16}: output and running statistics
    within (1e-4 + 2e-6 r^2) of the fp64 BN of the stored output (running
    variance at twice that). The r^2 term: the sums are held to rtol 1e-6 of
    fp64 sums, and S2 / n - (S1 / n)^2 loses a factor 1 + r^2.

    Measured on MI355X (table in profiles/NOTES.md): the six routes agree per
    producer; worst output error 3.5e-7 at r = 0, 8.6e-7 at r = 4, 1.4e-5 at
    r = 16 (h3p; the block-reduced producers 2.5e-7), bound 6.1e-4 there."""
    from rnb_amd.ops.bn import BatchNormBatch
    x = _d_input(kind)
    clip_seg = torch.tensor(D_SEG, dtype=torch.int32, device=DEV)
    worst = {}
    for r in (0, 4, 16):
        layer = _centred_layer("spatial" if kind == "spatial" else "temporal", r, x)
        tol = 1e-4 + 2e-6 * r * r
        bn = _make_bn(layer.geom.cout, 5)
        for fam, cid in _producers(kind, layer, x.shape).items():
            for route in _from_sums_routes():
                nseg = 20 if "20 seg" in route else 40 if "40 seg" in route else 4
                offs = D_OFFS + [D_OFFS[-1]] * (nseg - 4)
                seg = torch.tensor(offs, dtype=torch.int32, device=DEV)
                sums = torch.zeros((nseg, 2, layer.geom.cout_p), dtype=torch.float64,
                                   device=DEV)
                y = layer.forward_hip(x, config=cid, out_stats=(sums, clip_seg))
                torch.cuda.synchronize()
                assert float(sums[:3].abs().sum()) > 0 and float(sums[3:].abs().sum()) == 0
                thw = y.shape[1] * y.shape[2] * y.shape[3]
                res = torch.randn(y.shape, generator=torch.Generator().manual_seed(22)).to(DEV)
                ref, rm, rv = _bn_ref64(y, bn, res, True, offs, bn.running_mean,
                                        bn.running_var)
                op = BatchNormBatch(bn, layer.geom.cout_p, DEV)
                z = _run_route(route, op, y.clone(), res, sums, seg, thw, monkeypatch)
                e = _check_bn("%s r=%d %s" % (fam, r, route), op, z, bn, ref, rm, rv, tol)
                worst[(fam, r)] = max(worst.get((fam, r), 0.0), e)
                assert float(sums.abs().sum()) == 0.0, ("sums not re-armed", fam, route)
                acc = getattr(op, "_run_acc", None)
                assert acc is None or float(acc.abs().sum()) == 0.0
    for (fam, r), e in sorted(worst.items()):
        print("family %-14s r=%-3d worst output error %.2e" % (fam, r, e))
