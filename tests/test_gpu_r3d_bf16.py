"""r3d_18 (``tv_block="3d"``) served in bf16: the stride-1 3x3x3 convs on the
volume-halo kernel (csrc/conv_vol.hip) against the fp64 oracle."""
import pytest
import torch

import r3d_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def test_bf16_r3d18_vs_fp64_oracle(tmp_path, monkeypatch):
    """The logits may lie twice as far from the fp64 module as those of the
    same engine built without the family (RNB_VOL=0), with the same top-1."""
    from rnb_amd.models.r2p1d.decoder import SyntheticDecoder
    from rnb_amd.models.r2p1d.model import build_engine
    from rnb_amd.ops.conv import VOL_VARIANT
    from rnb_amd.ops.video import ndhwc_to_ncdhw
    ora = r3d_oracle.make(seed=9)
    path = str(tmp_path / "r3d18.pt")
    torch.save(ora.state_dict(), path)
    x = SyntheticDecoder(DEV).decode(31, [0, 60, 120, 180])
    assert x.dtype == torch.bfloat16 and x.shape[:2] == (4, 8)
    with torch.no_grad():
        y64 = ora.double()(ndhwc_to_ncdhw(x.float(), 3).double().cpu())
    err, picked = {}, {}
    for vol in ("1", "0"):
        monkeypatch.setenv("RNB_VOL", vol)
        eng = build_engine(DEV, depth=18, arch="torchvision", ckpt_path=path, autotune=False,
                           bn_mode="eval", dtype="bf16", use_graphs=False)
        assert eng.tv_block == "3d" and len(eng.ops) == 20
        y = eng.forward(x).double().cpu()
        err[vol] = (y - y64).abs().max().item() / y64.abs().max().item()
        picked[vol] = [c for layer in eng.conv_layers() for k, c in layer._config.items()
                       if isinstance(k[0], int) and c in VOL_VARIANT]
        if vol == "1":
            assert y.argmax(1).tolist() == y64.argmax(1).tolist()
    print("r3d_18 bf16 vs fp64: conv_vol %.3e, RNB_VOL=0 %.3e, %d convs on conv_vol"
          % (err["1"], err["0"], len(picked["1"])))
    assert picked["1"] and not picked["0"]
    assert err["1"] <= 2 * err["0"], err
