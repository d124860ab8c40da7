"""``tv_block="mc3"`` (torchvision's mc3_18) on the GPU: whole engines, with the
weights of the independent oracle tests/mc3_oracle.py loaded through
``ckpt_path`` and the tree chosen from the file, against the oracle in fp64."""
import os

import pytest
import torch

import mc3_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    ora = mc3_oracle.make(seed=9)
    path = str(tmp_path_factory.mktemp("mc3") / "mc3_18.pt")
    torch.save(ora.state_dict(), path)
    return ora, path


def _engine(path, **kw):
    from rnb_amd.models.r2p1d.model import build_engine
    return build_engine(DEV, depth=18, arch="torchvision", ckpt_path=path, autotune=False,
                        bn_mode="eval", use_graphs=False, **kw)


def _clips_and_fp64(ora, dtype, clip_length, starts):
    from rnb_amd.models.r2p1d.decoder import SyntheticDecoder
    from rnb_amd.ops.video import ndhwc_to_ncdhw
    x = SyntheticDecoder(DEV, dtype=dtype, clip_length=clip_length).decode(31, starts)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        y64 = ora.double()(ndhwc_to_ncdhw(x.float(), 3).double().cpu())
    ora.float()
    return x, y64


@pytest.mark.parametrize("clip_length,starts", [(8, [0, 60, 120, 180]), (16, [0, 90])])
def test_fp32_eval_engine_vs_fp64_oracle(ckpt, clip_length, starts):
    """e_hip <= 3 e_mod + 1e-6 against the oracle in fp64 (the r3d_18 rule);
    at 16 frames the head still pools 16 x 7 x 7."""
    ora, path = ckpt
    hip = _engine(path, dtype="fp32", clip_length=clip_length)
    mod = _engine(path, dtype="fp32", backend="module", clip_length=clip_length)
    assert hip.backend == "hip" and hip.tv_block == "mc3" and len(hip.ops) == 20
    assert hip._thw[hip.out_name] == (clip_length, 7, 7)
    x, y64 = _clips_and_fp64(ora, torch.float32, clip_length, starts)
    with torch.no_grad():
        y = hip.forward(x).double().cpu()
        ym = mod.forward(x).double().cpu()
    scale = y64.abs().max().item()
    e_hip = (y - y64).abs().max().item() / scale
    e_mod = (ym - y64).abs().max().item() / scale
    print("mc3_18 %d frames vs fp64: HIP %.2e, module %.2e" % (clip_length, e_hip, e_mod))
    assert e_hip <= 3 * e_mod + 1e-6, (e_hip, e_mod)


def test_bf16_stride2_convs_on_sp2(ckpt, monkeypatch):
    """layer2.0, layer3.0 and layer4.0's first convs forced on the id: the
    logits may lie twice as far from the fp64 oracle as those of the engine
    built under RNB_SP2=0, with the same top-1."""
    from rnb_amd.ops.conv import SP2, SP2_VARIANT
    ora, path = ckpt
    x, y64 = _clips_and_fp64(ora, torch.bfloat16, 8, [0, 60, 120, 180])
    thw = {64: (8, 56, 56), 128: (8, 28, 28), 256: (8, 14, 14)}    # input of the conv over cin
    err, ran = {}, {}
    for on in ("1", "0"):
        monkeypatch.setenv("RNB_SP2", on)
        eng = _engine(path, dtype="bf16")
        assert eng.tv_block == "mc3" and len(eng.ops) == 20
        s2 = [layer for layer in eng.conv_layers()
              if (layer.geom.kernel, layer.geom.stride) == ((1, 3, 3), (1, 2, 2))]
        if on == "1":
            for layer in s2:
                layer._config[(4,) + thw[layer.geom.cin_p]] = SP2
        y = eng.forward(x).double().cpu()
        err[on] = (y - y64).abs().max().item() / y64.abs().max().item()
        # the configs these convs ran: one per conv, so the forced keys were the shapes seen
        ran[on] = [c for layer in s2 for k, c in layer._config.items() if isinstance(k[0], int)]
        if on == "1":
            assert y.argmax(1).tolist() == y64.argmax(1).tolist()
    print("mc3_18 bf16 vs fp64: conv_sp2 %.3e, RNB_SP2=0 %.3e" % (err["1"], err["0"]))
    assert ran["1"] == [SP2] * 3
    assert len(ran["0"]) == 3 and not set(ran["0"]) & set(SP2_VARIANT)
    assert err["1"] <= 2 * err["0"], err
