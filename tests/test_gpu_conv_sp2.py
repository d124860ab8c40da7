"""The bf16 frame-stacked 1x3x3 stride-(1,2,2) kernel (csrc/conv_sp2.hip) against the fp64 conv."""
import pytest
import torch
import torch.nn.functional as F

from rnb_amd.ops.conv import SP2, SP2_VARIANT, ConvGeom, ConvLayer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# (cin, cout, (T, H, W), clips)
CASES = [
    (32, 64, (1, 4, 4), 2),         # one chunk; a box spanning both clips
    (64, 48, (3, 5, 7), 3),         # odd H, W: the far padding is read; cout no tile multiple
    (128, 128, (2, 9, 6), 2),       # four chunks: the patch prefetch runs; a partial last box
    (64, 128, (2, 56, 56), 1),      # mc3_18 layer2.0: 7 row bands per frame pair
    (128, 256, (2, 28, 28), 1),     # mc3_18 layer3.0
    (256, 512, (3, 14, 14), 1),     # mc3_18 layer4.0: frames stacked in a box, the last group short
    (64, 144, (1, 12, 12), 2),      # two output tiles, the second partial (R(2+1)D's mid count)
]
K133, S122, P011 = (1, 3, 3), (1, 2, 2), (0, 1, 1)
K3, ONE, TWO = (3, 3, 3), (1, 1, 1), (2, 2, 2)


def _setup(case, integer):
    """Layer, bf16 input, bf16 residual and the fp64 conv (+ bias) of the
    bf16-rounded operands as NDHWC."""
    cin, cout, thw, n = case
    geom = ConvGeom(cin, cout, K133, S122, P011)
    out = (n,) + geom.out_thw(*thw) + (cout,)
    g = torch.Generator().manual_seed(cin + cout + thw[1])
    if integer:
        w = torch.randint(-2, 3, (cout, cin) + K133, generator=g).float()
        b = torch.randint(-4, 5, (cout,), generator=g).float()
        x = torch.randint(-3, 4, (n,) + thw + (cin,), generator=g).float()
        r = torch.randint(-40, 41, out, generator=g).float()
    else:
        w = torch.randn((cout, cin) + K133, generator=g) * (2.0 / (9 * cin)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        x = torch.randn((n,) + thw + (cin,), generator=g)
        r = torch.randn(out, generator=g)
    layer = ConvLayer(w, b, geom, integer, DEV, "sp2")
    x, r = x.to(torch.bfloat16), r.to(torch.bfloat16)
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.to(torch.bfloat16).double(), b.double(),
                   stride=S122, padding=P011).permute(0, 2, 3, 4, 1)
    return layer, x.to(DEV), r.to(DEV), ref


def _ids(c):
    return "%dx%d_%s_n%d" % (c[0], c[1], "x".join(map(str, c[2])), c[3])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_sp2_integers_bit_exact(case):
    """|w| <= 2, |x| <= 3: every partial sum is an exact fp32 integer (at most
    9 * 256 * 6 = 13 824 < 2^24), so with bias, residual and ReLU the output is
    the fp64 result rounded once to bf16; no frame may have read a neighbour."""
    layer, x, res, ref = _setup(case, integer=True)
    want = torch.relu(ref + res.double().cpu()).to(torch.bfloat16)
    assert layer.sp2_candidates(x.shape) == [SP2]
    y = layer.forward_hip(x, residual=res, config=SP2).cpu()
    assert torch.equal(y[..., :case[1]], want), \
        (y[..., :case[1]].double() - want.double()).abs().max().item()
    assert torch.count_nonzero(y[..., case[1]:]) == 0


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_sp2_normal_data_within_twice_generic_error(case):
    """Against the fp64 conv of the bf16-rounded operands the new kernel may
    err twice what the worst generic conv_igemm config does on the same
    inputs: both add the same bf16 products in fp32, in another order, and
    round once to bf16."""
    cin, cout, thw, _ = case
    layer, x, _, ref = _setup(case, integer=False)
    e_gen = max((layer.forward_hip(x, config=c).cpu()[..., :cout].double() - ref).abs().max().item()
                for c in layer.generic_candidates())
    y = layer.forward_hip(x, config=SP2).cpu()[..., :cout].double()
    e_sp2 = (y - ref).abs().max().item()
    print("conv_sp2 %s: max error %.3e, generic worst %.3e" % (_ids(case), e_sp2, e_gen))
    assert e_sp2 <= 2 * e_gen, (e_sp2, e_gen)


@pytest.mark.parametrize("cin,kernel,stride,padding", [
    (64, K133, ONE, P011),                    # stride-1 1x3x3 (the halo kernels')
    (64, K3, S122, ONE),                      # 3x3x3 stride (1,2,2)
    (64, K3, TWO, ONE),                       # 3x3x3 stride 2 (conv_vol2's)
    (3, K133, S122, P011),                    # cin_p = 8
], ids=["stride1", "3x3x3_s122", "3x3x3_s2", "cin8"])
def test_sp2_not_offered_elsewhere(cin, kernel, stride, padding, monkeypatch):
    """The id goes to no other geometry, forcing it there raises, and
    RNB_SP2=0 takes it from the geometry it serves."""
    geom = ConvGeom(cin, 64, kernel, stride, padding)
    layer = ConvLayer(torch.zeros((64, cin) + kernel), torch.zeros(64), geom, True, DEV)
    x = torch.zeros((2, 4, 8, 8, geom.cin_p), dtype=torch.bfloat16, device=DEV)
    assert not layer.sp2_candidates(x.shape)
    assert not set(layer.special_candidates(x.shape)) & set(SP2_VARIANT)
    with pytest.raises(ValueError):
        layer.forward_hip(x, config=SP2)
    monkeypatch.setenv("RNB_SP2", "0")
    served = ConvLayer(torch.zeros((64, 64) + K133), torch.zeros(64),
                       ConvGeom(64, 64, K133, S122, P011), True, DEV)
    assert not served.sp2_candidates((2, 4, 8, 8, 64))
