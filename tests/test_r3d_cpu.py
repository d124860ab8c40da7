"""``tv_block="3d"`` (torchvision's r3d_18) on the CPU: the module tree against
the independent oracle tests/r3d_oracle.py, the checkpoint loader with the
tree chosen from the file, the error messages and the engine's torch plan."""
import pytest
import torch

import r3d_oracle
import tv_oracle

CPU = torch.device("cpu")


def _net(**kw):
    from rnb_amd.models.r2p1d.model import build_network
    kw.setdefault("arch", "torchvision")
    kw.setdefault("depth", 18)
    return build_network(1, 5, **kw)


def test_keys_shapes_and_parameter_count():
    ora = r3d_oracle.R3DOracle()
    want = {k: tuple(v.shape) for k, v in ora.state_dict().items()}
    assert sum(p.numel() for p in ora.parameters()) == r3d_oracle.PARAMS
    assert len(want) == r3d_oracle.ENTRIES
    assert want["stem.0.weight"] == (64, 3, 3, 7, 7)
    assert want["layer3.0.conv1.0.weight"] == (256, 128, 3, 3, 3)
    assert want["layer3.0.downsample.0.weight"] == (256, 128, 1, 1, 1)
    net = _net(tv_block="3d")
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    assert got == want
    assert sum(p.numel() for p in net.parameters()) == 33371472


@pytest.mark.parametrize("wrapped", [False, True])
def test_checkpoint_round_trip_detects_the_tree_and_matches_fp64(tmp_path, wrapped):
    """The oracle's state dict through ``ckpt_path`` with no ``tv_block``: the
    tree comes from the file's stem, the weights are the file's, and both
    trees in fp64 agree to 1e-12 on a 2-frame-deep tiny input."""
    ora = r3d_oracle.make(seed=3)
    path = str(tmp_path / "r3d.pt")
    torch.save({"state_dict": ora.state_dict()} if wrapped else ora.state_dict(), path)
    for given in (None, "3d"):
        net = _net(ckpt_path=path, tv_block=given, seed=11)
        assert net.tv_block == "3d"
        for k, v in ora.state_dict().items():
            assert torch.equal(net.state_dict()[k], v), k
    x = torch.randn(2, 3, 2, 32, 32, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        want, got = ora.double()(x), net.double()(x)
    scale = want.abs().max().item()
    assert scale > 1e-3 and (got - want).abs().max().item() <= 1e-12 * scale
    # an R(2+1)D file still chooses the (2+1)D tree
    p2 = str(tmp_path / "r2p1d.pt")
    torch.save(tv_oracle.make(18, seed=2).state_dict(), p2)
    assert _net(ckpt_path=p2).tv_block == "2plus1d"


def test_errors_name_the_key(tmp_path):
    from rnb_amd.config import ConfigError, _check_arch_keys
    from rnb_amd.models.r2p1d.network import load_torchvision_state_dict
    path = str(tmp_path / "r3d.pt")
    good = r3d_oracle.make(seed=4).state_dict()
    torch.save(good, path)
    with pytest.raises(ValueError, match="tv_block '2plus1d' contradicts the checkpoint"):
        _net(ckpt_path=path, tv_block="2plus1d")
    with pytest.raises(ValueError, match="midplanes belongs to tv_block='2plus1d'"):
        _net(tv_block="3d", midplanes="block")
    net = _net(tv_block="3d")
    ref = {"res2plus1d.conv1.spatial_conv.weight": torch.zeros(1), "linear.bias": torch.zeros(1)}
    with pytest.raises(ValueError, match="reference-format keys"):
        load_torchvision_state_dict(net, ref)
    with pytest.raises(ConfigError, match="tv_block must be one of"):
        _check_arch_keys({"arch": "torchvision", "tv_block": "r3d"}, "step 0")
    with pytest.raises(ConfigError, match="tv_block belongs to"):
        _check_arch_keys({"tv_block": "3d"}, "step 0")


@pytest.mark.parametrize("bn_mode", ["eval", "batch"])
def test_torch_plan_matches_the_module(tmp_path, bn_mode):
    """The engine's plan of the "3d" tree (backend="torch") against the module
    itself, at fp32; FLOPs and the activation bound follow the tree."""
    from rnb_amd.models.r2p1d.engine import activation_elems_per_clip
    from rnb_amd.models.r2p1d.model import build_engine
    kw = dict(depth=18, arch="torchvision", tv_block="3d", bn_mode=bn_mode, dtype="fp32", seed=5)
    plan = build_engine(CPU, backend="torch", **kw)
    mod = build_engine(CPU, backend="module", **kw)
    assert plan.tv_block == "3d" and len(plan.ops) == 1 + 8 * 2 + 3
    x = torch.randn(plan.input_shape(2), generator=torch.Generator().manual_seed(2))
    x[..., 3:] = 0
    with torch.no_grad():
        y, r = plan.forward(x), mod.forward(x)
    assert (y - r).abs().max().item() <= 1e-4 * r.abs().max().item()
    # 2 FLOPs per MAC: the stem and layer1's four convs alone
    assert plan.flops_per_clip() > 2 * 8 * 56 * 56 * 64 * (3 * 147 + 4 * 64 * 27)
    assert (activation_elems_per_clip(1, 5, torch.float32, 8, "torchvision", "3d")
            == 8 * 56 * 56 * 64)
