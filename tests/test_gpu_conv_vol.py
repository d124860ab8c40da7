"""The bf16 volume-halo 3x3x3 kernel (csrc/conv_vol.hip) against the fp64 conv."""
import pytest
import torch
import torch.nn.functional as F

from rnb_amd.ops.conv import VOL_VARIANT, ConvGeom, ConvLayer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# (cin, cout, (T, H, W), clips)
CASES = [
    (64, 64, (2, 9, 16), 3),        # clip borders on both sides of the middle clip
    (64, 48, (3, 7, 5), 2),         # cout no multiple of the channel tile; odd W
    (128, 128, (5, 6, 6), 2),       # odd T: the last box has a frame past T; two chunks
    (128, 128, (4, 28, 28), 1),     # r3d_18 layer2
    (256, 256, (2, 14, 14), 2),     # r3d_18 layer3
    (512, 512, (2, 7, 7), 2),       # r3d_18 layer4
    (64, 64, (4, 56, 56), 1),       # r3d_18 layer1
]
K3, ONE = (3, 3, 3), (1, 1, 1)


def _setup(case, integer):
    """Layer, bf16 input, bf16 residual and the fp64 conv (+ bias) of the
    bf16-rounded operands as NDHWC."""
    cin, cout, thw, n = case
    g = torch.Generator().manual_seed(cin + cout + thw[1])
    if integer:
        w = torch.randint(-2, 3, (cout, cin) + K3, generator=g).float()
        b = torch.randint(-4, 5, (cout,), generator=g).float()
        x = torch.randint(-3, 4, (n,) + thw + (cin,), generator=g).float()
        r = torch.randint(-40, 41, (n,) + thw + (cout,), generator=g).float()
    else:
        w = torch.randn((cout, cin) + K3, generator=g) * (2.0 / (27 * cin)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        x = torch.randn((n,) + thw + (cin,), generator=g)
        r = torch.randn((n,) + thw + (cout,), generator=g)
    layer = ConvLayer(w, b, ConvGeom(cin, cout, K3, ONE, ONE), integer, DEV, "vol")
    x, r = x.to(torch.bfloat16), r.to(torch.bfloat16)
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.to(torch.bfloat16).double(), b.double(),
                   padding=1).permute(0, 2, 3, 4, 1)
    return layer, x.to(DEV), r.to(DEV), ref


def _ids(c):
    return "%dx%d_%s_n%d" % (c[0], c[1], "x".join(map(str, c[2])), c[3])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_vol_integers_bit_exact(case):
    """|w| <= 2, |x| <= 3: every partial sum is an exact fp32 integer below
    2^24, so with bias, residual and ReLU the output is the fp64 result
    rounded once to bf16 (nearest even), for every eligible variant; with two
    or more clips no clip may have read a neighbour's frames."""
    layer, x, res, ref = _setup(case, integer=True)
    want = torch.relu(ref + res.double().cpu()).to(torch.bfloat16)
    ids = layer.vol_candidates(x.shape)
    assert ids
    for cid in ids:
        y = layer.forward_hip(x, residual=res, config=cid).cpu()
        assert torch.equal(y[..., :case[1]], want), \
            (cid, (y[..., :case[1]].double() - want.double()).abs().max().item())
        assert torch.count_nonzero(y[..., case[1]:]) == 0


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_vol_normal_data_within_twice_generic_error(case):
    """Against the fp64 conv of the bf16-rounded operands the new kernel may
    err twice what the worst generic conv_igemm config does on the same
    inputs: both add the same bf16 products in fp32, in another order, and
    round once to bf16. Also: which geometries are offered the family."""
    cin, cout, thw, _ = case
    layer, x, _, ref = _setup(case, integer=False)
    e_gen = max((layer.forward_hip(x, config=c).cpu()[..., :cout].double() - ref).abs().max().item()
                for c in layer.generic_candidates())
    ids = layer.vol_candidates(x.shape)
    assert ids
    for cid in ids:
        y = layer.forward_hip(x, config=cid).cpu()[..., :cout].double()
        e_vol = (y - ref).abs().max().item()
        print("conv_vol %s id %d: max error %.3e, generic worst %.3e" % (_ids(case), cid, e_vol,
                                                                        e_gen))
        assert e_vol <= 2 * e_gen, (cid, e_vol, e_gen)
    if thw[2] in (28, 14, 7):
        assert set(layer.special_candidates(x.shape)) & set(VOL_VARIANT)
    w2 = torch.zeros((cout, cin) + K3)
    s2 = ConvLayer(w2, torch.zeros(cout), ConvGeom(cin, cout, K3, (2, 2, 2), ONE), True, DEV)
    sp = ConvLayer(w2[:, :, :1], torch.zeros(cout), ConvGeom(cin, cout, (1, 3, 3), ONE, (0, 1, 1)),
                   True, DEV)
    for other in (s2, sp):
        assert not other.vol_candidates(x.shape)
        assert not set(other.special_candidates(x.shape)) & set(VOL_VARIANT)
