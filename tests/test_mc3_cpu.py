"""``tv_block="mc3"`` (torchvision's mc3_18) on the CPU: the module tree against
the independent oracle tests/mc3_oracle.py, the tree chosen from a checkpoint,
the error messages and the engine's plan, whose layers keep the frame count."""
import pytest
import torch

import mc3_oracle
import r3d_oracle

CPU = torch.device("cpu")
KW = dict(arch="torchvision", depth=18)


def _net(start=1, end=5, **kw):
    from rnb_amd.models.r2p1d.model import build_network
    return build_network(start, end, **dict(KW, **kw))


def test_keys_shapes_and_parameter_count():
    ora = mc3_oracle.MC3Oracle()
    want = {k: tuple(v.shape) for k, v in ora.state_dict().items()}
    assert sum(p.numel() for p in ora.parameters()) == mc3_oracle.PARAMS == 11695440
    assert want["stem.0.weight"] == (64, 3, 3, 7, 7)
    assert want["layer1.0.conv1.0.weight"] == (64, 64, 3, 3, 3)
    assert want["layer2.0.conv1.0.weight"] == (128, 64, 1, 3, 3)
    assert want["layer4.0.downsample.0.weight"] == (512, 256, 1, 1, 1)
    net = _net(tv_block="mc3")
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want
    assert sum(p.numel() for p in net.parameters()) == 11695440


def test_checkpoint_detects_the_tree_and_matches_fp64(tmp_path):
    """The oracle's state dict with no ``tv_block``: layer2.0.conv1.0.weight's
    temporal extent chooses the tree (an r3d_18 file still chooses "3d"), and
    both trees in fp64 agree to 1e-12 on a 2-clip input."""
    ora = mc3_oracle.make(seed=3)
    path, p3 = str(tmp_path / "mc3.pt"), str(tmp_path / "r3d.pt")
    torch.save(ora.state_dict(), path)
    torch.save(r3d_oracle.make(seed=2).state_dict(), p3)
    net = _net(ckpt_path=path, seed=11)
    assert net.tv_block == "mc3" and _net(ckpt_path=path, tv_block="mc3").tv_block == "mc3"
    assert _net(ckpt_path=p3).tv_block == "3d"
    x = torch.randn(2, 3, 3, 32, 32, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        want, got = ora.double()(x), net.double()(x)
    scale = want.abs().max().item()
    assert scale > 1e-3 and (got - want).abs().max().item() <= 1e-12 * scale
    for given, file in (("3d", path), ("2plus1d", path), ("mc3", p3)):
        key = "stem.0.weight" if given == "2plus1d" else "layer2.0.conv1.0.weight"
        with pytest.raises(ValueError, match="tv_block %r contradicts the checkpoint, whose %s"
                           % (given, key)):
            _net(ckpt_path=file, tv_block=given)


def test_midplanes_and_partial_ranges_raise():
    from rnb_amd.config import ConfigError, _check_arch_keys
    from rnb_amd.models.r2p1d.model import R2P1DRunner, build_engine
    with pytest.raises(ValueError, match="midplanes belongs to tv_block='2plus1d'"):
        _net(tv_block="mc3", midplanes="block")
    with pytest.raises(ConfigError, match="midplanes belongs to"):
        _check_arch_keys(dict(KW, tv_block="mc3", midplanes="conv"), "step 0")
    with pytest.raises(ValueError, match="tv_block 'mc3' serves layers 1..5"):
        _net(1, 3, tv_block="mc3")
    with pytest.raises(ValueError, match="tv_block 'mc3' serves layers 1..5"):
        build_engine(CPU, 2, 5, backend="torch", tv_block="mc3", **KW)
    with pytest.raises(ValueError, match="tv_block 'mc3' serves layers 1..5"):
        R2P1DRunner(CPU, 1, 4, backend="torch", tv_block="mc3", **KW)
    with pytest.raises(ConfigError, match="tv_block \"mc3\" serves layers 1..5"):
        _check_arch_keys(dict(KW, tv_block="mc3", start_index=3, end_index=5), "step 1")
    _check_arch_keys(dict(KW, tv_block="mc3", start_index=1, end_index=5), "step 1")


@pytest.mark.parametrize("clip_length", [8, 16])
def test_torch_plan_keeps_the_frame_count(clip_length):
    """1 + 16 + 3 ops; every layer leaves clip_length frames; the plan agrees
    with the module at fp32; the geometry helpers know the tree."""
    from rnb_amd.models.r2p1d.engine import activation_elems_per_clip
    from rnb_amd.models.r2p1d.model import build_engine
    from rnb_amd.models.r2p1d.network import layer_geometry
    kw = dict(KW, tv_block="mc3", dtype="fp32", seed=5, clip_length=clip_length)
    plan = build_engine(CPU, backend="torch", **kw)
    mod = build_engine(CPU, backend="module", **kw)
    assert plan.tv_block == "mc3" and len(plan.ops) == 1 + 16 + 3
    t = clip_length
    assert layer_geometry(t, "mc3")[1] == {1: (64, t, 56, 56), 2: (64, t, 56, 56),
                                           3: (128, t, 28, 28), 4: (256, t, 14, 14), 5: None}
    assert layer_geometry(t, "3d") == layer_geometry(t)
    assert plan._thw[plan.out_name] == (t, 7, 7)
    x = torch.randn(plan.input_shape(1), generator=torch.Generator().manual_seed(2))
    x[..., 3:] = 0
    with torch.no_grad():
        y, r = plan.forward(x), mod.forward(x)
    assert (y - r).abs().max().item() <= 1e-4 * r.abs().max().item()
    assert (activation_elems_per_clip(1, 5, torch.float32, t, "torchvision", "mc3")
            == t * 56 * 56 * 64)
