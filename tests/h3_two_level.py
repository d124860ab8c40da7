"""Two-level data for the h3 kernels: non-zero lo parts, exact answers.

The h3 kernels split every fp32 operand, after a power-of-two scale, into an
fp16 hi and lo part and sum the hi / lo products in fp32. Small integers (the
data of the bit-exact tests in tests/test_gpu_h3.py) have lo = 0, so those
tests never see a lo fragment. A *two-level* value v = A + B u (A, B small
integers, u = 2^-11) splits into hi ~ A and lo ~ B u, both exact, so hi + lo
== v with lo != 0 for about half of the elements. With one operand two-level
and the other fp16-exact (small integers, lo = 0) the al bl term vanishes,
every product is an integer multiple of u, and while the *span* of an output
(sum |x| |w| + |bias| + |residual|, in units of u) stays below 2^22 every
partial sum in any order is exact in fp32: the fp64 conv is then the only
correct fp32 answer and the kernels are held to it bit for bit.

No GPU here: generators, the host emulation of the split, the span and the
lo coverage, and the table of cases shared by tests/test_h3_two_level_cpu.py
and tests/test_gpu_h3_lo_path.py.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

U_LOG2 = -11                 # u = 2^-11
SPAN_LIMIT_BITS = 22         # two bits below fp32's 24
MIN_LO_COVERAGE = 0.4
B_VALUES = (-3, -2, -1, 0, 1, 2, 3)
B_ODD = (-3, -1, 1, 3)

# value sets by reduction length K = taps * Cin: the integer weights (and the A
# of two-level weights), their density, the B of two-level weights, the integer
# inputs. Two-level inputs always take A in {-2, -1, 1, 2}. Weights whose A is
# +-1 scale to 2^13 +- 4 B: above 2^13 the fp16 ulp is 8 and only an odd B
# leaves a lo part, below it the ulp is 4 and none does, so those sets draw B
# from the odd values to keep the lo coverage at one half. Spans: the table in
# profiles/h3_lo_path.txt.
VALUE_SETS = {
    "k576": SimpleNamespace(w=(-2, -1, 0, 1, 2), w_density=1.0, w_b=B_VALUES,
                            x=(-3, -2, -1, 0, 1, 2, 3)),
    "k1728": SimpleNamespace(w=(-1, 0, 0, 1), w_density=1.0, w_b=B_ODD, x=(-1, 0, 1)),
    "k4608": SimpleNamespace(w=(-1, 1), w_density=0.25, w_b=B_ODD, x=(-1, 0, 1)),
    "k4608a": SimpleNamespace(w=(-1, 1), w_density=0.125, w_b=B_ODD, x=(-1, 0, 1)),
}
# the input BN on load turns a two-level x into relu(x s + t), up to 2 |x| + 2
# at u / 2: those cases take the next sparser weights
AFFINE_VSET = {"k576": "k1728", "k1728": "k4608", "k4608": "k4608a", "h3w": "h3wa"}
X_TWO_LEVEL_A = (-2, -1, 1, 2)


def value_set_for(k_total: int) -> str:
    """The densest value set whose span fits 22 bits at reduction length K."""
    return "k576" if k_total <= 640 else "k1728" if k_total <= 1728 else "k4608"


def _choice(values, shape, g):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def exact_ints(shape, values, density=1.0, seed=0):
    """fp16-exact partner tensor: small integers from ``values`` (lo = 0),
    kept with probability ``density`` and zero elsewhere. fp32."""
    g = torch.Generator().manual_seed(seed)
    a = _choice(values, shape, g)
    if density < 1.0:
        a = a * (torch.rand(shape, generator=g, dtype=torch.float64) < density)
    return a.float()


def two_level(shape, a_values, b_values=B_VALUES, density=1.0, seed=0, u_log2=U_LOG2):
    """(v, A): v = A + B u as fp32 (exact: 13 bits at most), A from
    ``a_values`` kept with probability ``density``, B from ``b_values`` where
    A != 0 and 0 elsewhere (a zero stays a zero: padding and sparsity)."""
    g = torch.Generator().manual_seed(seed)
    a = _choice(a_values, shape, g)
    if density < 1.0:
        a = a * (torch.rand(shape, generator=g, dtype=torch.float64) < density)
    b = _choice(b_values, shape, g) * (a != 0)
    v = a + b * 2.0 ** u_log2
    assert torch.equal(v.float().double(), v)
    return v.float(), a


def split_fp16(a: torch.Tensor, scale_log2: int):
    """The packers' and kernels' split of a * 2^scale_log2 (RNE): h =
    fp16(a), l = fp16(a - h) with a - h formed in a's own precision. Returns
    (h, l, scaled a), h and l as fp16."""
    s = a * (2.0 ** scale_log2)
    h = s.half()
    lo = (s - h.to(s.dtype)).half()
    return h, lo, s


def lo_coverage(a_level: torch.Tensor, lo: torch.Tensor) -> float:
    """Among elements whose A != 0, the share with a non-zero lo part."""
    m = a_level != 0
    return float((lo[m] != 0).double().mean()) if m.any() else 0.0


def host_layer(w, b, k, s, p, relu=True):
    """What span_bits and ref64 need of a ConvLayerF32, without a device."""
    geom = SimpleNamespace(cin=w.shape[1], cout=w.shape[0], kernel=tuple(k), stride=tuple(s),
                           padding=tuple(p))
    return SimpleNamespace(geom=geom, w_ref=w.float(), b_ref=b.float(), relu=relu)


def _conv64(x, w, geom):
    xin = x[..., :geom.cin].double().cpu().permute(0, 4, 1, 2, 3)
    return F.conv3d(xin, w, None, stride=tuple(geom.stride),
                    padding=tuple(geom.padding)).permute(0, 2, 3, 4, 1)


def span_bits(x, layer, bias=None, res=None, u_log2=U_LOG2) -> float:
    """log2 of the largest output span, sum |x| |w| + |bias| + |residual| in
    units of u, in fp64 on the CPU. Below SPAN_LIMIT_BITS every partial sum
    of every summation order is an exact fp32 number."""
    g = layer.geom
    bias = layer.b_ref if bias is None else bias
    span = _conv64(x.abs(), layer.w_ref.double().cpu().abs(), g)
    span = span + bias[:g.cout].double().cpu().abs()
    if res is not None:
        span = span + res[..., :g.cout].double().cpu().abs()
    return math.log2(max(float(span.max()), 2.0 ** -60) * 2.0 ** -u_log2)


def ref64(layer, x, res=None):
    """fp64 CPU conv of the layer, as tests/test_gpu_f32.py _ref64."""
    g = layer.geom
    y = _conv64(x, layer.w_ref.double().cpu(), g) + layer.b_ref.double().cpu()
    if res is not None:
        y = y + res[..., :g.cout].double().cpu()
    return torch.relu(y) if layer.relu else y


# -- Winograd F(2x2, 3x3), for the h3w span and the V split --------------------
WINO_G = torch.tensor(((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0)),
                      dtype=torch.float64)
WINO_BT = torch.tensor(((1.0, 0.0, -1.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, -1.0, 1.0, 0.0),
                        (0.0, 1.0, 0.0, -1.0)), dtype=torch.float64)


def wino_u(w):
    """U = G g G^T of [Cout, Cin, 1, 3, 3] weights, fp64 [Cout, Cin, 4, 4]."""
    g = w.double().cpu().reshape(w.shape[0], w.shape[1], 3, 3)
    return torch.einsum("ik,ockl,jl->ocij", WINO_G, g, WINO_G)


def wino_v(x):
    """V = B^T d B of every 4x4 input tile (stride 2, pad 1, frames padded up
    to whole tiles with zeros) of x [N, T, H, W, C], fp64
    [N, T, tiles_h, tiles_w, C, 4, 4]."""
    xd = x.double().cpu()
    n, t, h, w, c = xd.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = F.pad(xd.permute(0, 1, 4, 2, 3), (1, 2 * tw + 1 - w, 1, 2 * th + 1 - h))
    d = xp.unfold(3, 4, 2).unfold(4, 4, 2)                  # [n, t, c, th, tw, 4, 4]
    v = torch.einsum("ik,ntcabkl,jl->ntabcij", WINO_BT, d, WINO_BT)
    return v


def wino_span_bits(x, layer, res=None, u_log2=U_LOG2) -> float:
    """The h3w span: sum over channels and the 16 tile positions of |U| |V|
    (each of the four outputs of a tile adds a subset of the 16 products
    with coefficients +-1), + |bias| + |residual|, in units of u / 4 (U of
    integer weights is a multiple of 1/4)."""
    g = layer.geom
    m = torch.einsum("ocij,ntabcij->ntabo", wino_u(layer.w_ref[:, :g.cin]).abs(),
                     wino_v(x[..., :g.cin]).abs())
    span = float(m.max()) + float(layer.b_ref.double().abs().max())
    if res is not None:
        span += float(res[..., :g.cout].double().abs().max())
    return math.log2(max(span, 2.0 ** -60) * 2.0 ** -(u_log2 - 2))


# -- the cases -----------------------------------------------------------------
SPATIAL = ((1, 3, 3), (1, 1, 1), (0, 1, 1))
TEMPORAL = ((3, 1, 1), (1, 1, 1), (1, 0, 0))
TEMPORAL_S2 = ((3, 1, 1), (2, 1, 1), (1, 0, 0))
STEM = ((1, 7, 7), (1, 2, 2), (0, 3, 3))
POINT_S2 = ((1, 1, 1), (1, 2, 2), (0, 0, 0))


def _case(family, cin, cout, ksp, thw, n, vset=None, cin_pad16=False, relu=True):
    k, s, p = ksp
    kt = k[0] * k[1] * k[2] * cin
    return SimpleNamespace(family=family, cin=cin, cout=cout, k=k, s=s, p=p, thw=thw, n=n,
                           vset=vset or value_set_for(kt), cin_pad16=cin_pad16, relu=relu,
                           id="%s-%dx%d-k%s-s%s-%s-n%d" % (
                               family, cin, cout, "".join(map(str, k)), "".join(map(str, s)),
                               "x".join(map(str, thw)), n))


# temporal band shapes of test_h3_temporal_band_exact_integers_stats_and_affine
TEMPORAL_SHAPES = [((8, 9, 7), 80, 72), ((4, 14, 14), 64, 150), ((2, 7, 7), 144, 64),
                   ((8, 8, 8), 48, 130), ((8, 7, 9), 144, 64), ((2, 9, 8), 576, 256),
                   ((8, 4, 4), 144, 64), ((8, 8, 8), 83, 64), ((8, 4, 8), 80, 48),
                   ((4, 4, 8), 288, 128), ((4, 4, 4), 288, 64)]
# BAND_SHAPES of tests/test_gpu_h3p_band.py
BAND_SHAPES = [((16, 4, 4), 144, 64), ((16, 4, 8), 83, 64), ((32, 4, 4), 48, 64),
               ((8, 4, 8), 288, 128), ((16, 4, 4), 288, 64)]
# forced single pixel range (test_h3p_many_tasks_per_wave_cross_video)
SINGLE_RANGE_SHAPES = [((8, 12, 8), 144, 64), ((8, 12, 8), 83, 64), ((4, 12, 12), 288, 128)]

CASES = {
    "direct": [_case("direct", 64, 150, SPATIAL, (2, 15, 13), 1)],
    "direct_more": [_case("direct", 40, 72, TEMPORAL, (8, 9, 7), 3, relu=False),
                    _case("direct", 40, 72, TEMPORAL_S2, (4, 5, 6), 3, relu=False),
                    _case("direct", 40, 72, TEMPORAL, (1, 7, 7), 3, relu=False),
                    _case("direct", 3, 72, STEM, (2, 19, 17), 3, relu=False),
                    _case("direct", 64, 42, POINT_S2, (2, 8, 8), 3)],
    "splitk": [_case("splitk", 64, 150, SPATIAL, (1, 7, 7), 3),
               _case("splitk", 256, 150, TEMPORAL, (2, 7, 7), 3),
               _case("splitk", 64, 150, ((1, 3, 3), (1, 2, 2), (0, 1, 1)), (2, 14, 14), 3)],
    "h3r": [_case("h3r", 64, 150, SPATIAL, thw, 2)
            for thw in ((2, 15, 13), (2, 28, 28), (1, 7, 7), (3, 56, 56))]
    + [_case("h3r", 512, 150, SPATIAL, (1, 7, 7), 2)],
    "temporal": [_case("temporal", cin, cout, TEMPORAL, thw, 3, cin_pad16=True)
                 for thw, cin, cout in TEMPORAL_SHAPES],
    "h3p_single": [_case("h3p_single", cin, cout, TEMPORAL, thw, 5, cin_pad16=True)
                   for thw, cin, cout in SINGLE_RANGE_SHAPES],
    "h3p_band": [_case("h3p_band", cin, cout, TEMPORAL, thw, 3, cin_pad16=True)
                 for thw, cin, cout in BAND_SHAPES],
    "h3stem": [_case("h3stem", 3, 72, STEM, (1, 19, 17), 2),
               _case("h3stem", 3, 40, STEM, (2, 30, 112), 2)],
    "h3s": [_case("h3s", 64, 72, ((1, 3, 3), (1, 2, 2), (0, 1, 1)), (2, 13, 15), 2),
            _case("h3s", 32, 40, ((1, 3, 3), (1, 2, 2), (0, 1, 1)), (1, 7, 9), 2)],
    # h3w: Cin 32 and inputs in {-1, 0, 1} (the Winograd transforms grow both
    # operands: |V| <= 4 |d|, U in quarters)
    "h3w": [_case("h3w", 32, 150, SPATIAL, thw, 2, vset="h3w")
            for thw in ((2, 15, 13), (1, 7, 7), (2, 14, 14))],
}
VALUE_SETS["h3w"] = SimpleNamespace(w=(-1, 0, 0, 1), w_density=1.0, w_b=B_ODD, x=(-1, 0, 1))
VALUE_SETS["h3wa"] = SimpleNamespace(w=(-1, 0, 0, 1), w_density=0.25, w_b=B_ODD, x=(-1, 0, 1))
H3W_X_TWO_LEVEL_A = (-1, 1)
ALL_CASES = [c for fam in CASES.values() for c in fam]


def cin_p_of(case) -> int:
    """Channel padding of the case's input: 16 for the temporal layers built
    as the engine builds the stem's temporal conv, else fp32's 4."""
    return (case.cin + 15) // 16 * 16 if case.cin_pad16 else (case.cin + 3) // 4 * 4


def out_thw(case):
    return tuple((d + 2 * p - k) // s + 1 for d, p, k, s in zip(case.thw, case.p, case.k, case.s))


def make_data(case, which: int, u_log2=U_LOG2):
    """The tensors of one case, on the CPU: ``which`` = 1 puts the two-level
    values in the activations (integer weights), 2 in the weights (integer
    activations), 0 neither (the integer data of the existing tests, from
    the same value sets). Returns a namespace with w [Cout, Cin, kt, kh, kw],
    b [Cout], x [N, T, H, W, Cin_p] (padding channels zero), res [N, To, Ho,
    Wo, Cout] (integers), and the A levels of the two-level operand."""
    vs = VALUE_SETS[case.vset]
    wshape = (case.cout, case.cin) + tuple(case.k)
    xshape = (case.n,) + tuple(case.thw) + (case.cin,)
    a_w = a_x = None
    if which == 2:
        w, a_w = two_level(wshape, vs.w, vs.w_b, vs.w_density, seed=10, u_log2=u_log2)
    else:
        w = exact_ints(wshape, vs.w, vs.w_density, seed=10)
    if which == 1:
        xa = H3W_X_TWO_LEVEL_A if case.family == "h3w" else X_TWO_LEVEL_A
        xc, a_x = two_level(xshape, xa, seed=11, u_log2=u_log2)
    else:
        xc = exact_ints(xshape, vs.x, seed=11)
    cp = cin_p_of(case)
    x = torch.zeros(xshape[:-1] + (cp,), dtype=torch.float32)
    x[..., :case.cin] = xc
    b = exact_ints((case.cout,), (-4, -3, -2, -1, 0, 1, 2, 3, 4), seed=12)
    res = exact_ints((case.n,) + out_thw(case) + (case.cout,), (-3, -2, -1, 0, 1, 2, 3), seed=13)
    return SimpleNamespace(w=w, b=b, x=x, res=res, a_w=a_w, a_x=a_x)


def affine_case(case):
    """The case with at least three clips and the sparser weights."""
    c = SimpleNamespace(**vars(case))
    c.n, c.vset, c.id = max(case.n, 3), AFFINE_VSET[case.vset], case.id + "-affine"
    return c


def affine_seg(n):
    """Clip -> video map with a clip-less video 1: video 0 holds the first
    clip, video 2 the rest (small frames put both in one tile)."""
    return torch.tensor([0] + [2] * (n - 1), dtype=torch.int32)


def affine_rows(nvid, cin_p, seed=14):
    """Per-video, per-channel input BN rows [nvid, 2, Cin_p]: scale in {0.5,
    1, 2}, integer shift in {-2..2}. relu(x * scale + shift) of a two-level
    x is two-level at u / 2."""
    g = torch.Generator().manual_seed(seed)
    ss = torch.empty((nvid, 2, cin_p), dtype=torch.float32)
    ss[:, 0] = _choice((0.5, 1.0, 2.0), (nvid, cin_p), g).float()
    ss[:, 1] = _choice((-2, -1, 0, 1, 2), (nvid, cin_p), g).float()
    return ss


def apply_affine(x, ss, seg, cin):
    """relu(x * scale + shift) per clip's video; padding channels stay zero."""
    s = ss[seg.long()]
    xa = torch.relu(x * s[:, 0][:, None, None, None, :] + s[:, 1][:, None, None, None, :])
    xa[..., cin:] = 0
    return xa


def affine_level(xa):
    """The A level of an applied input: multiples of 1/2 (scale 0.5), the
    rest being the B part at u / 2."""
    return torch.round(xa.double() * 2) / 2
