"""``arch="torchvision"`` on the CPU: the module tree against an independent
statement of torchvision's R(2+1)D layout (tests/tv_oracle.py), the
checkpoint loader, the layer ranges, the engine's plan on the torch backend,
the config keys and one launcher run."""
import json
import os
import subprocess
import sys

import pytest
import torch

import tv_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _net(**kw):
    from rnb_amd.models.r2p1d.model import build_network
    kw.setdefault("arch", "torchvision")
    return build_network(kw.pop("start", 1), kw.pop("end", 5), **kw)


def _clips(n, seed=1, t=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, t, 112, 112, generator=g)


@pytest.mark.parametrize("depth", [18, 34])
def test_oracle_counts_are_torchvisions(depth):
    """The oracle itself: depth 18 has torchvision's published num_params for
    r2plus1d_18, and the state dicts have the entry counts of the layout."""
    m = tv_oracle.TVOracle(depth)
    params, entries = tv_oracle.COUNTS[depth]
    assert sum(p.numel() for p in m.parameters()) == params
    assert len(m.state_dict()) == entries


@pytest.mark.parametrize("depth", [18, 34])
@pytest.mark.parametrize("rule", ["block", "conv"])
def test_tree_keys_and_shapes_equal_the_oracles(depth, rule):
    want = {k: tuple(v.shape) for k, v in tv_oracle.TVOracle(depth, mid_rule=rule)
            .state_dict().items()}
    got = {k: tuple(v.shape) for k, v in _net(depth=depth, midplanes=rule).state_dict().items()}
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    assert got == want


def test_mid_channels_of_depth_18():
    """torchvision's rule: 144, 144 | 230, 288 | 460, 576 | 921, 1152 for the two
    blocks of each layer, the same in both convs of a block; the per-conv rule
    differs only in the downsampling blocks' second conv."""
    from rnb_amd.models.r2p1d.network import tv_block_mids
    sizes = {2: 2, 3: 2, 4: 2, 5: 2}
    block, conv = tv_block_mids(sizes, "block"), tv_block_mids(sizes, "conv")
    assert [block["layer%d.%d.conv1" % (l, b)] for l in (1, 2, 3, 4) for b in (0, 1)] == \
        [144, 144, 230, 288, 460, 576, 921, 1152]
    assert all(block[k.replace("conv1", "conv2")] == v for k, v in block.items()
               if k.endswith("conv1"))
    assert block["layer2.0.conv2"] == 230 and conv["layer2.0.conv2"] == 288
    assert {k for k in block if block[k] != conv[k]} == {"layer2.0.conv2", "layer3.0.conv2",
                                                         "layer4.0.conv2"}
    assert (conv["layer3.0.conv2"], conv["layer4.0.conv2"]) == (576, 1152)


@pytest.mark.parametrize("rule,eps", [("block", 1e-5), ("conv", 1e-3)])
def test_loaded_tree_matches_oracle_fp64(rule, eps):
    """The oracle's state dict loaded into the product tree: both in fp64,
    eval, on one 3 x 8 x 112 x 112 clip, agree to 1e-12 of the logit scale."""
    from rnb_amd.models.r2p1d.network import load_torchvision_state_dict
    ora = tv_oracle.make(18, mid_rule=rule, bn_eps=eps, seed=3)
    net = _net(depth=18, midplanes=rule, bn_eps=eps, seed=11)
    load_torchvision_state_dict(net, ora.state_dict())
    x = _clips(1).double()
    with torch.no_grad():
        want = ora.double()(x)
        got = net.double()(x)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print("fp64 tree vs oracle: err %.3e scale %.3e" % (err, scale))
    assert scale > 0.1 and err <= 1e-12 * scale


def test_mids_are_inferred_from_the_checkpoint(tmp_path):
    """A "conv"-rule file loads with no ``midplanes`` given (and under a
    contradicting one): every mid comes from the tensor shapes."""
    ora = tv_oracle.make(18, mid_rule="conv", seed=5)
    path = str(tmp_path / "conv_rule.pt")
    torch.save({"state_dict": ora.state_dict()}, path)
    for given in (None, "block"):
        net = _net(depth=18, ckpt_path=path, midplanes=given)
        assert net.layer2[0].conv2[0][0].out_channels == 288
        assert net.layer4[0].conv2[0][3].in_channels == 1152
        assert net.layer2[0].conv1[0][0].out_channels == 230
        for k, v in ora.state_dict().items():
            assert torch.equal(net.state_dict()[k], v), k
    raw = str(tmp_path / "raw.pt")
    torch.save(tv_oracle.make(18, mid_rule="block", seed=6).state_dict(), raw)
    assert _net(depth=18, ckpt_path=raw).layer2[0].conv2[0][0].out_channels == 230


def test_ranges_compose_to_the_whole_model(tmp_path):
    """Ranges (1, 2) + (3, 5) hold the whole model's weights (seeded, and
    loaded from a checkpoint) and compute the whole model's function."""
    x = _clips(1, seed=2)
    whole = _net(depth=18, seed=4)
    a, b = _net(start=1, end=2, depth=18, seed=4), _net(start=3, end=5, depth=18, seed=4)
    assert set(a.state_dict()) | set(b.state_dict()) == set(whole.state_dict())
    assert not set(a.state_dict()) & set(b.state_dict())
    assert all(k.startswith(("stem.", "layer1.")) for k in a.state_dict())
    for part in (a, b):
        for k, v in part.state_dict().items():
            assert torch.equal(v, whole.state_dict()[k]), k
    with torch.no_grad():
        mid = a(x)
        assert tuple(mid.shape) == (1, 64, 8, 56, 56)
        assert torch.equal(b(mid), whole(x))
    path = str(tmp_path / "tv18.pt")
    ora = tv_oracle.make(18, seed=8)
    torch.save(ora.state_dict(), path)
    a, b = (_net(start=1, end=2, depth=18, ckpt_path=path),
            _net(start=3, end=5, depth=18, ckpt_path=path))
    with torch.no_grad():
        assert torch.allclose(b(a(x)), ora(x), rtol=0, atol=1e-5 * ora(x).abs().max().item())


def test_loader_errors_name_what_is_wrong():
    from rnb_amd.models.r2p1d.network import load_torchvision_state_dict
    good = tv_oracle.make(18, seed=1).state_dict()
    net = _net(depth=18)
    # accepted: wrapped dicts, num_batches_tracked present or absent
    load_torchvision_state_dict(net, {"state_dict": dict(good)})
    load_torchvision_state_dict(net, {k: v for k, v in good.items()
                                      if not k.endswith("num_batches_tracked")})
    missing = {k: v for k, v in good.items() if k != "layer3.1.conv2.0.3.weight"}
    with pytest.raises(ValueError, match=r"missing key 'layer3\.1\.conv2\.0\.3\.weight'"):
        load_torchvision_state_dict(net, missing)
    extra = dict(good)
    extra["layer1.2.conv1.1.weight"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"unexpected key 'layer1\.2\.conv1\.1\.weight'"):
        load_torchvision_state_dict(net, extra)
    load_torchvision_state_dict(net, extra, strict=False)
    # keys outside the built range are not this range's business
    part = _net(start=1, end=2, depth=18)
    load_torchvision_state_dict(part, good)
    with pytest.raises(ValueError, match=r"missing key 'stem\.0\.weight'"):
        load_torchvision_state_dict(part, {k: v for k, v in good.items()
                                           if k != "stem.0.weight"})
    conv_rule = tv_oracle.make(18, mid_rule="conv").state_dict()
    with pytest.raises(ValueError) as e:
        load_torchvision_state_dict(net, conv_rule)
    msg = str(e.value)
    assert "layer2.0.conv2.0.0.weight" in msg
    assert "(288, 128, 1, 3, 3)" in msg and "(230, 128, 1, 3, 3)" in msg
    other = tv_oracle.make(18, num_classes=101).state_dict()
    with pytest.raises(ValueError, match="num_classes") as e:
        load_torchvision_state_dict(net, other)
    assert "101" in str(e.value) and "400" in str(e.value)
    from rnb_amd.models.r2p1d.model import build_network
    ref = build_network(1, 5, depth=18).state_dict()
    with pytest.raises(ValueError, match="arch") as e:
        load_torchvision_state_dict(net, ref)
    assert "res2plus1d." in str(e.value)


def test_build_network_arguments(tmp_path):
    from rnb_amd.models.r2p1d.model import build_network, default_bn_mode
    with pytest.raises(ValueError, match="arch"):
        build_network(1, 5, depth=18, arch="resnet")
    with pytest.raises(ValueError, match="midplanes"):
        build_network(1, 5, depth=18, arch="torchvision", midplanes="layer")
    with pytest.raises(ValueError, match="bn_eps"):
        build_network(1, 5, depth=18, arch="torchvision", bn_eps=-1.0)
    with pytest.raises(ValueError, match="midplanes"):
        build_network(1, 5, depth=18, midplanes="conv")
    net = build_network(4, 5, depth=34, arch="torchvision", bn_eps=1e-3)
    assert all(m.eps == 1e-3 for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d))
    assert not net.training and not hasattr(net, "stem") and hasattr(net, "fc")
    # the default tree is today's
    assert type(build_network(1, 5, depth=18)).__name__ == "R2Plus1DLayerWrapper"
    assert default_bn_mode(None, "fp32", "torchvision") == "eval"
    assert default_bn_mode(None, "bf16", "torchvision") == "eval"
    assert default_bn_mode("batch", "fp32", "torchvision") == "batch"
    assert default_bn_mode(None, "fp32") == "batch" and default_bn_mode(None, "fp32", None) == "batch"


def _plan_distance(arch, bn_mode, x, seed):
    """max |torch-backend plan - its own module| over the logit scale."""
    from rnb_amd.models.r2p1d.model import build_engine
    from rnb_amd.ops.video import ncdhw_to_ndhwc
    kw = dict(depth=18, arch=arch, bn_mode=bn_mode, dtype="fp32", seed=seed)
    plan = build_engine(CPU, backend="torch", **kw)
    mod = build_engine(CPU, backend="module", **kw)
    with torch.no_grad():
        got = plan(ncdhw_to_ndhwc(x, 4, dtype=torch.float32))
        want = mod(x)
    return (got - want).abs().max().item() / want.abs().max().item(), plan


@pytest.mark.parametrize("bn_mode", ["eval", "batch"])
def test_torch_plan_is_as_close_to_its_module_as_the_reference_archs(bn_mode):
    """The folded (eval) and the unfolded batch-BN plan of the new tree on the
    torch backend: fp32 distance to the tree's own module within 4 x the
    distance the reference arch's plan has from its module (same seed, same
    clips)."""
    x = _clips(2, seed=7)
    d_ref, _ = _plan_distance("reference", bn_mode, x, 3)
    d_tv, plan = _plan_distance("torchvision", bn_mode, x, 3)
    print("%s: reference %.3e torchvision %.3e" % (bn_mode, d_ref, d_tv))
    assert d_ref > 0 and d_tv <= 4 * d_ref
    assert plan.arch == "torchvision"


def test_plan_of_the_new_tree():
    """The plan: 45 -> 48 and 230 -> 240 mid padding for the 16-channel
    temporal kernels, one conv per shortcut whose output is the residual of
    conv2's temporal conv, every temporary freed once, deferred BNs only where
    the consumer is the only reader, and the per-clip activation bound of
    check_max_clips equal to the plan's largest tensor."""
    from rnb_amd.models.r2p1d.engine import activation_elems_per_clip, max_clips_limit
    from rnb_amd.models.r2p1d.model import build_engine
    eng = build_engine(CPU, depth=18, arch="torchvision", bn_mode="batch", dtype="fp32",
                       backend="torch")
    ops = {op.layer.name: op for op in eng.ops}
    assert len(eng.ops) == 2 + 8 * 4 + 3
    g = ops["stem.spatial"].layer.geom
    assert (g.cin_p, g.cout, g.cout_p) == (4, 45, 48)
    assert ops["stem.temporal"].layer.geom.cin_p == 48 and ops["stem.temporal"].bn_relu
    assert ops["layer2.0.conv2.spatial"].layer.geom.cout_p == 240
    assert ops["layer2.0.conv2.temporal"].layer.geom.cin_p == 240
    assert ops["layer3.0.conv2.spatial"].layer.geom.cout_p == 464
    assert ops["layer2.0.conv1.spatial"].layer.geom.cout_p == 232       # stride-2 temporal
    for n in (2, 3, 4):
        ds = ops["layer%d.0.downsample" % n]
        dg = ds.layer.geom
        assert dg.kernel == (1, 1, 1) and dg.stride == (2, 2, 2) and dg.padding == (0, 0, 0)
        assert ds.res is None and not ds.bn_relu and ds.bn is not None
        assert ops["layer%d.0.conv2.temporal" % n].res == ds.dst
        assert ds.src == ops["layer%d.0.conv1.spatial" % n].src
        assert not eng._defer_ok[eng.ops.index(ds)]
    assert ops["layer1.0.conv2.temporal"].res == ops["stem.temporal"].dst
    assert not eng._defer_ok[eng.ops.index(ops["stem.temporal"])]       # two readers
    assert eng._defer_ok[eng.ops.index(ops["stem.spatial"])]
    freed = [n for names in eng._free_after for n in names]
    assert len(freed) == len(set(freed)) == len(eng.ops) - 1
    for i, op in enumerate(eng.ops):
        for later in eng.ops[i + 1:]:
            for name in eng._free_after[i]:
                assert name not in (later.src, later.res)
    worst = max(t * h * w * op.layer.geom.cout_p for op in eng.ops
                for (t, h, w) in [eng._thw[op.dst]])
    for dt in (torch.float32,):
        assert activation_elems_per_clip(1, 5, dt, 8, "torchvision") == worst
    # the stem alone: the 48-channel intermediate is below the 64-channel output
    assert activation_elems_per_clip(1, 1, torch.float32, 8, "torchvision") == 8 * 56 * 56 * 64
    assert activation_elems_per_clip(1, 1, torch.float32, 8) == 8 * 56 * 56 * 96
    assert max_clips_limit(1, 1, torch.float32, 8, "torchvision") > \
        max_clips_limit(1, 1, torch.float32, 8)
    # a bias-free conv folds: the folded bias is the BN's shift
    ev = build_engine(CPU, depth=18, arch="torchvision", bn_mode="eval", dtype="fp32",
                      backend="torch")
    bn = ev.net.stem[1]
    want = bn.bias - bn.running_mean * bn.weight / torch.sqrt(bn.running_var + bn.eps)
    assert torch.allclose(ev.ops[0].layer.b_ref[:45].cpu(), want.float(), atol=1e-6)
    assert ev.head is not None and ev.head.num_classes == 400


def test_config_keys_are_validated():
    from rnb_amd.config import ConfigError, load_pipeline, parse_pipeline
    spec = load_pipeline(os.path.join(ROOT, "configs", "r2p1d-whole-tv18.json"))
    assert all(g.kwargs["arch"] == "torchvision" and g.kwargs["depth"] == 18
               for s in spec.steps for g in s.groups)
    spec = load_pipeline(os.path.join(ROOT, "configs", "r2p1d-whole-y4m-3crop-eval-tv18.json"))
    kw = spec.steps[1].groups[0].kwargs
    assert kw["arch"] == "torchvision" and kw["bn_mode"] == "eval" and "ckpt_path" not in kw
    assert spec.override_kwargs({"ckpt_path": "/w.pt"}).steps[1].groups[0].kwargs["ckpt_path"] \
        == "/w.pt"
    base = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-tv18.json")))

    def with_(where, **kw):
        cfg = json.loads(json.dumps(base))
        (cfg["defaults"] if where == "defaults" else cfg["pipeline"][1]).update(kw)
        return cfg

    for where in ("defaults", "step"):
        with pytest.raises(ConfigError, match="arch"):
            parse_pipeline(with_(where, arch="tv"))
        with pytest.raises(ConfigError, match="midplanes"):
            parse_pipeline(with_(where, midplanes="per-conv"))
        with pytest.raises(ConfigError, match="bn_eps"):
            parse_pipeline(with_(where, bn_eps="1e-3"))
        ok = parse_pipeline(with_(where, midplanes="conv", bn_eps=1e-3))
        assert ok.steps[1].groups[0].kwargs["midplanes"] == "conv"
    assert issubclass(ConfigError, ValueError)
    cfg = with_("defaults", midplanes="conv")
    cfg["defaults"]["arch"] = "reference"
    with pytest.raises(ConfigError, match="midplanes"):
        parse_pipeline(cfg)


def test_runner_and_single_step_pass_the_layout_through():
    from rnb_amd.models.r2p1d.model import R2P1DRunner, R2P1DSingleStep
    kw = dict(depth=10, arch="torchvision", midplanes="conv", bn_eps=1e-3, warmup=0, max_clips=3)
    r = R2P1DRunner(CPU, **kw)
    assert r.arch == "torchvision" and r.bn_mode == "eval"
    assert r.engine.arch == "torchvision"
    assert r.engine.net.layer2[0].conv2[0][0].out_channels == 288
    assert r.engine.net.stem[1].eps == 1e-3
    with pytest.raises(ValueError, match="arch"):
        R2P1DRunner(CPU, depth=10, arch="caffe2", warmup=0)
    s = R2P1DSingleStep(CPU, num_clips_population=(1,), num_clips_weights=(1,), **kw)
    assert s.runner.engine.arch == "torchvision"
    assert s.runner.engine.net.layer3[0].conv2[0][0].out_channels == 576


def test_launcher_serves_the_tv18_config_on_cpu(tmp_path):
    """configs/r2p1d-whole-tv18.json through the real launcher, replicas on the
    CPU (a shallower tree and few clips per video, as the other shipped-config
    runs of tests/test_pipeline_e2e.py)."""
    out = tmp_path / "res.json"
    cmd = [sys.executable, os.path.join(ROOT, "benchmark.py"),
           "-c", os.path.join(ROOT, "configs", "r2p1d-whole-tv18.json"),
           "--log-root", str(tmp_path / "logs"), "--json-out", str(out),
           "--barrier-timeout", "200", "-v", "6", "-mi", "0", "--cpu-only",
           "--set", "depth=10", "--set", "num_clips_population=[1,2]",
           "--set", "num_clips_weights=[2,1]", "--set", "warmup=0"]
    env = dict(os.environ, RNB_NO_TQDM="1", RNB_CPU_THREADS="1", PYTHONPATH=ROOT)
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    res = json.loads(out.read_text())
    assert res["termination_flag"] == "TARGET_NUM_VIDEOS_REACHED" and res["videos_done"] >= 6
