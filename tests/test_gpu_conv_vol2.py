"""The bf16 parity-staged 3x3x3 stride-2 kernel (csrc/conv_vol2.hip) against the fp64 conv."""
import pytest
import torch
import torch.nn.functional as F

import r3d_oracle
from rnb_amd.ops.conv import VOL2, VOL2_VARIANT, ConvGeom, ConvLayer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# (cin, cout, (T, H, W), clips)
CASES = [
    (64, 64, (4, 6, 8), 3),         # even sizes; clip borders on both sides of the middle clip
    (64, 48, (3, 5, 7), 2),         # odd T, H, W: the far padding is read; cout no tile multiple
    (32, 64, (1, 4, 4), 2),         # one input frame (only dt = 1 inside); a single chunk
    (128, 128, (5, 9, 6), 2),       # four chunks; three frame boxes (one output frame per box)
    (64, 128, (8, 56, 56), 1),      # r3d_18 layer2.0: 7 row bands x 4 frame boxes
    (128, 256, (4, 28, 28), 1),     # r3d_18 layer3.0: 2 row bands x 2 frame boxes
    (256, 512, (2, 14, 14), 2),     # r3d_18 layer4.0
]
K3, ONE, TWO = (3, 3, 3), (1, 1, 1), (2, 2, 2)


def _setup(case, integer):
    """Layer, bf16 input, bf16 residual and the fp64 conv (+ bias) of the
    bf16-rounded operands as NDHWC."""
    cin, cout, thw, n = case
    geom = ConvGeom(cin, cout, K3, TWO, ONE)
    out = (n,) + geom.out_thw(*thw) + (cout,)
    g = torch.Generator().manual_seed(cin + cout + thw[1])
    if integer:
        w = torch.randint(-2, 3, (cout, cin) + K3, generator=g).float()
        b = torch.randint(-4, 5, (cout,), generator=g).float()
        x = torch.randint(-3, 4, (n,) + thw + (cin,), generator=g).float()
        r = torch.randint(-40, 41, out, generator=g).float()
    else:
        w = torch.randn((cout, cin) + K3, generator=g) * (2.0 / (27 * cin)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        x = torch.randn((n,) + thw + (cin,), generator=g)
        r = torch.randn(out, generator=g)
    layer = ConvLayer(w, b, geom, integer, DEV, "vol2")
    x, r = x.to(torch.bfloat16), r.to(torch.bfloat16)
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.to(torch.bfloat16).double(), b.double(),
                   stride=2, padding=1).permute(0, 2, 3, 4, 1)
    return layer, x.to(DEV), r.to(DEV), ref


def _ids(c):
    return "%dx%d_%s_n%d" % (c[0], c[1], "x".join(map(str, c[2])), c[3])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_vol2_integers_bit_exact(case):
    """|w| <= 2, |x| <= 3: every partial sum is an exact fp32 integer (at most
    27 * 512 * 6 = 82 944 < 2^24), so with bias, residual and ReLU the output is
    the fp64 result rounded once to bf16, for every eligible variant; with two
    or more clips no clip may have read a neighbour's frames."""
    layer, x, res, ref = _setup(case, integer=True)
    want = torch.relu(ref + res.double().cpu()).to(torch.bfloat16)
    ids = layer.vol2_candidates(x.shape)
    assert VOL2 in ids
    for cid in ids:
        y = layer.forward_hip(x, residual=res, config=cid).cpu()
        assert torch.equal(y[..., :case[1]], want), \
            (cid, (y[..., :case[1]].double() - want.double()).abs().max().item())
        assert torch.count_nonzero(y[..., case[1]:]) == 0


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_vol2_normal_data_within_twice_generic_error(case):
    """Against the fp64 conv of the bf16-rounded operands the new kernel may
    err twice what the worst generic conv_igemm config does on the same
    inputs: both add the same bf16 products in fp32, in another order, and
    round once to bf16."""
    cin, cout, thw, _ = case
    layer, x, _, ref = _setup(case, integer=False)
    e_gen = max((layer.forward_hip(x, config=c).cpu()[..., :cout].double() - ref).abs().max().item()
                for c in layer.generic_candidates())
    ids = layer.vol2_candidates(x.shape)
    assert VOL2 in ids
    for cid in ids:
        y = layer.forward_hip(x, config=cid).cpu()[..., :cout].double()
        e_vol = (y - ref).abs().max().item()
        print("conv_vol2 %s id %d: max error %.3e, generic worst %.3e" % (_ids(case), cid, e_vol,
                                                                         e_gen))
        assert e_vol <= 2 * e_gen, (cid, e_vol, e_gen)


@pytest.mark.parametrize("cin,kernel,stride,padding", [
    (64, K3, ONE, ONE),                       # stride-1 3x3x3 (conv_vol's)
    (64, (1, 3, 3), (1, 2, 2), (0, 1, 1)),    # spatial stride-2 conv of R(2+1)D
    (64, K3, (1, 2, 2), ONE),                 # mc3_18's
    (3, K3, TWO, ONE),                        # cin_p = 8
], ids=["stride1", "1x3x3", "s122", "cin8"])
def test_vol2_not_offered_elsewhere(cin, kernel, stride, padding, monkeypatch):
    """The ids go to no other geometry, forcing one there raises, and
    RNB_VOL2=0 takes them from the geometry they serve."""
    geom = ConvGeom(cin, 64, kernel, stride, padding)
    layer = ConvLayer(torch.zeros((64, cin) + kernel), torch.zeros(64), geom, True, DEV)
    x = torch.zeros((2, 4, 8, 8, geom.cin_p), dtype=torch.bfloat16, device=DEV)
    assert not layer.vol2_candidates(x.shape)
    assert not set(layer.special_candidates(x.shape)) & set(VOL2_VARIANT)
    for cid in VOL2_VARIANT:
        with pytest.raises(ValueError):
            layer.forward_hip(x, config=cid)
    monkeypatch.setenv("RNB_VOL2", "0")
    served = ConvLayer(torch.zeros((64, 64) + K3), torch.zeros(64), ConvGeom(64, 64, K3, TWO, ONE),
                       True, DEV)
    assert not served.vol2_candidates((2, 4, 8, 8, 64))


def test_bf16_r3d18_stride2_convs_on_vol2(tmp_path, monkeypatch):
    """r3d_18 with layer2.0, layer3.0 and layer4.0's first convs forced on the
    id: the logits may lie twice as far from the fp64 module as those of the
    engine built under RNB_VOL2=0, with the same top-1."""
    from rnb_amd.models.r2p1d.decoder import SyntheticDecoder
    from rnb_amd.models.r2p1d.model import build_engine
    from rnb_amd.ops.video import ndhwc_to_ncdhw
    ora = r3d_oracle.make(seed=9)
    path = str(tmp_path / "r3d18.pt")
    torch.save(ora.state_dict(), path)
    x = SyntheticDecoder(DEV).decode(31, [0, 60, 120, 180])
    with torch.no_grad():
        y64 = ora.double()(ndhwc_to_ncdhw(x.float(), 3).double().cpu())
    thw = {64: (8, 56, 56), 128: (4, 28, 28), 256: (2, 14, 14)}    # input of the conv over cin
    err, ran = {}, {}
    for on in ("1", "0"):
        monkeypatch.setenv("RNB_VOL2", on)
        eng = build_engine(DEV, depth=18, arch="torchvision", ckpt_path=path, autotune=False,
                           bn_mode="eval", dtype="bf16", use_graphs=False)
        assert eng.tv_block == "3d" and len(eng.ops) == 20
        s2 = [layer for layer in eng.conv_layers()
              if (layer.geom.kernel, layer.geom.stride) == (K3, TWO)]
        if on == "1":
            for layer in s2:
                layer._config[(4,) + thw[layer.geom.cin_p]] = VOL2
        y = eng.forward(x).double().cpu()
        err[on] = (y - y64).abs().max().item() / y64.abs().max().item()
        # the configs these convs ran: one per conv, so the forced keys were the shapes seen
        ran[on] = [c for layer in s2 for k, c in layer._config.items() if isinstance(k[0], int)]
        if on == "1":
            assert y.argmax(1).tolist() == y64.argmax(1).tolist()
    print("r3d_18 bf16 vs fp64: conv_vol2 %.3e, RNB_VOL2=0 %.3e" % (err["1"], err["0"]))
    assert ran["1"] == [VOL2] * 3
    assert len(ran["0"]) == 3 and not set(ran["0"]) & set(VOL2_VARIANT)
    assert err["1"] <= 2 * err["0"], err
