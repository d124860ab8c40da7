"""The bf16 patch-staged 3x7x7 stem kernel (csrc/conv_stem3d.hip) against the fp64 conv."""
import pytest
import torch
import torch.nn.functional as F

import r3d_oracle
from rnb_amd.ops.conv import STEM3D, ConvGeom, ConvLayer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# (cin, cout, (T, H, W), clips)
CASES = [
    (3, 64, (2, 8, 12), 3),         # all border; the middle clip has neighbours on both sides
    (3, 64, (3, 10, 15), 2),        # odd T: the last box has a frame past T; odd W
    (4, 48, (4, 14, 18), 1),        # the fourth channel carries data; Cout_p < 64
    (3, 64, (5, 23, 30), 2),        # odd H, a partial last row band, three frame boxes
    (3, 64, (4, 112, 112), 1),      # the workload's frame, Wo = 56
]
K, S, P = (3, 7, 7), (1, 2, 2), (1, 3, 3)


def _setup(case, integer):
    """Layer, bf16 NDHWC8 input, bf16 residual and the fp64 conv (+ bias) of
    the bf16-rounded operands as NDHWC. Channels cin..7 of the input hold
    data the conv must not see."""
    cin, cout, thw, n = case
    g = torch.Generator().manual_seed(cin + cout + thw[1])
    To, Ho, Wo = thw[0], (thw[1] - 1) // 2 + 1, (thw[2] - 1) // 2 + 1
    if integer:
        w = torch.randint(-2, 3, (cout, cin) + K, generator=g).float()
        b = torch.randint(-4, 5, (cout,), generator=g).float()
        x = torch.randint(-3, 4, (n,) + thw + (8,), generator=g).float()
        r = torch.randint(-40, 41, (n, To, Ho, Wo, cout), generator=g).float()
    else:
        w = torch.randn((cout, cin) + K, generator=g) * (2.0 / (147 * cin)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        x = torch.randn((n,) + thw + (8,), generator=g)
        r = torch.randn((n, To, Ho, Wo, cout), generator=g)
    layer = ConvLayer(w, b, ConvGeom(cin, cout, K, S, P), integer, DEV, "stem3d")
    x, r = x.to(torch.bfloat16), r.to(torch.bfloat16)
    ref = F.conv3d(x[..., :cin].double().permute(0, 4, 1, 2, 3), w.to(torch.bfloat16).double(),
                   b.double(), stride=S, padding=P).permute(0, 2, 3, 4, 1)
    return layer, x.to(DEV), r.to(DEV), ref


def _ids(c):
    return "%dx%d_%s_n%d" % (c[0], c[1], "x".join(map(str, c[2])), c[3])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_stem3d_integers_bit_exact(case):
    """|w| <= 2, |x| <= 3: every partial sum is an exact fp32 integer below
    2^24, so with bias, residual and ReLU the output is the fp64 result
    rounded once to bf16, with one block per box and with 5 blocks that walk
    the boxes (a block's later rounds reuse its patch buffer)."""
    layer, x, res, ref = _setup(case, integer=True)
    want = torch.relu(ref + res.double().cpu()).to(torch.bfloat16)
    assert layer.stem3d_candidates(x.shape) == [STEM3D]
    for grid in (0, 5):
        layer.stem3d_grid = grid
        y = layer.forward_hip(x, residual=res, config=STEM3D).cpu()
        assert y.shape[-1] == layer.geom.cout_p
        assert torch.equal(y[..., :case[1]], want), \
            (grid, (y[..., :case[1]].double() - want.double()).abs().max().item())
        assert torch.count_nonzero(y[..., case[1]:]) == 0


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_stem3d_normal_data_within_twice_generic_error(case):
    """Against the fp64 conv of the bf16-rounded operands the new kernel may
    err twice what the worst generic conv_igemm config does on the same
    inputs: both add the same bf16 products in fp32, in another order, and
    round once to bf16."""
    cin, cout, thw, _ = case
    layer, x, _, ref = _setup(case, integer=False)
    e_gen = max((layer.forward_hip(x, config=c).cpu()[..., :cout].double() - ref).abs().max().item()
                for c in layer.generic_candidates())
    y = layer.forward_hip(x, config=STEM3D).cpu()[..., :cout].double()
    e_new = (y - ref).abs().max().item()
    print("conv_stem3d %s: max error %.3e, generic worst %.3e" % (_ids(case), e_new, e_gen))
    assert e_new <= 2 * e_gen, (e_new, e_gen)


def test_stem3d_eligibility(monkeypatch):
    """Which geometries are offered the id, and RNB_STEM3D=0."""
    def layer(cin, kernel, stride, padding):
        return ConvLayer(torch.zeros((64, cin) + kernel), torch.zeros(64),
                         ConvGeom(cin, 64, kernel, stride, padding), True, DEV)
    shape = (2, 4, 14, 18, 8)
    assert layer(3, K, S, P).stem3d_candidates(shape) == [STEM3D]
    for other in (layer(3, (1, 7, 7), S, (0, 3, 3)), layer(3, K, (1, 1, 1), P), layer(8, K, S, P)):
        assert other.stem3d_candidates(shape) == []
        assert STEM3D not in other.special_candidates(shape)
        with pytest.raises((ValueError, RuntimeError)):
            other.forward_hip(torch.zeros(shape, dtype=torch.bfloat16, device=DEV), config=STEM3D)
    monkeypatch.setenv("RNB_STEM3D", "0")
    for case in CASES:
        off = layer(case[0], K, S, P)
        assert off.stem3d_candidates((case[3],) + case[2] + (8,)) == []


def test_stem3d_r3d18_vs_fp64_oracle(tmp_path, monkeypatch):
    """bf16 r3d_18 with its stem pinned to the id has the fp64 oracle's top-1,
    and its logits lie at most twice as far from the oracle's as those of the
    engine built under RNB_STEM3D=0."""
    from rnb_amd.models.r2p1d.decoder import SyntheticDecoder
    from rnb_amd.models.r2p1d.model import build_engine
    from rnb_amd.ops.video import ndhwc_to_ncdhw
    ora = r3d_oracle.make(seed=9)
    path = str(tmp_path / "r3d18.pt")
    torch.save(ora.state_dict(), path)
    x = SyntheticDecoder(DEV).decode(31, [0, 60, 120, 180])
    with torch.no_grad():
        y64 = ora.double()(ndhwc_to_ncdhw(x.float(), 3).double().cpu())
    err = {}
    for on in ("1", "0"):
        monkeypatch.setenv("RNB_STEM3D", on)
        eng = build_engine(DEV, depth=18, arch="torchvision", ckpt_path=path, autotune=False,
                           bn_mode="eval", dtype="bf16", use_graphs=False)
        stem = eng.conv_layers()[0]
        assert stem.geom.kernel == K
        if on == "1":
            assert stem.stem3d_candidates(x.shape) == [STEM3D]
            stem._config[tuple(x.shape[:4])] = STEM3D
        y = eng.forward(x).double().cpu()
        assert (stem._config[tuple(x.shape[:4])] == STEM3D) == (on == "1")
        err[on] = (y - y64).abs().max().item() / y64.abs().max().item()
        if on == "1":
            assert y.argmax(1).tolist() == y64.argmax(1).tolist()
    print("r3d_18 bf16 vs fp64: stem on conv_stem3d %.3e, RNB_STEM3D=0 %.3e" % (err["1"], err["0"]))
    assert err["1"] <= 2 * err["0"], err
