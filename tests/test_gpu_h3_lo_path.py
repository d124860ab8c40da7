"""The lo half of the h3 data path, pinned as hard as the integer tests pin hi.

The bit-exact tests of tests/test_gpu_h3.py use small integers, whose fp16
split is hi = value, lo = 0: every lo LDS plane, lo fragment read, lo chunk of
the packed weights and lo half of the in-kernel split multiplies zeros there,
and the random-data tests' 1e-5 bound is one to two orders above the real h3
error. Here the data is two-level (tests/h3_two_level.py): v = A + B 2^-11
splits into non-zero hi and lo parts exactly, the other operand is fp16-exact,
and every output's span stays below 2^22 units, so the fp64 conv is the only
correct fp32 answer and every family and config is held to it bit for bit --
pass 1 with the two-level values in the activations (the in-kernel split, the
input BN on load), pass 2 with them in the weights (the host packers, every
weight-lo fragment read). Controls on the same data: the fp32-MFMA kernel and
every x6 direct config. A patched packer that zeroes or swaps lo chunks shows
that the test sees a lo fault and the integer data does not. Then the fp32-class
error bound of test_h3_error_is_fp32_class for every family, at amplitudes 1
and 1e-3 and at the documented range edges.

Every test prints its figures (span bits, lo coverage, errors) before it
asserts; profiles/h3_lo_path.txt is that output of one run.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import h3_two_level as tl
from test_gpu_f32 import DEV, _input, _layer, _ref64
from test_gpu_h3 import _h3_ids, _h3r_ids, _h3stem_ids, _tlayer

pytestmark = pytest.mark.gpu


# -- plumbing ------------------------------------------------------------------
def _build(case, d, relu=None):
    from rnb_amd.ops.conv import ConvGeom
    from rnb_amd.ops.conv_f32 import F32_ALIGN, ConvLayerF32, f32_geom
    relu = case.relu if relu is None else relu
    if case.cin_pad16 and case.cin % 16:
        geom = ConvGeom(cin=case.cin, cout=case.cout, kernel=case.k, stride=case.s,
                        padding=case.p, align=F32_ALIGN, cin_pad=tl.cin_p_of(case))
    else:
        geom = f32_geom(case.cin, case.cout, case.k, case.s, case.p)
    assert geom.cin_p == tl.cin_p_of(case)
    return ConvLayerF32(d.w, d.b, geom, relu, DEV, "h3lo")


def _pad_res(layer, res):
    out = torch.zeros(res.shape[:-1] + (layer.geom.cout_p,), dtype=torch.float32)
    out[..., :res.shape[-1]] = res
    return out.to(DEV)


def _ids(case, layer, shape):
    """Every built config or variant of the case's family that fits."""
    from rnb_amd.ops import conv_f32 as cf
    from rnb_amd.ops.native import kernels
    fam = case.family
    if fam == "direct":
        return _h3_ids()
    if fam == "splitk":
        return [c for c in range(cf.H3K_BASE, cf.H3K_BASE + len(cf.H3K_CONFIGS))
                if layer.ksplit_for(c, shape) > 1]
    if fam == "h3r":
        return [c for c in _h3r_ids() if layer.h3r_fits(c - cf.H3R_BASE, shape, efficient=False)]
    if fam == "h3stem":
        return _h3stem_ids(layer, shape)
    if fam == "h3w":
        return [cf.H3W_BASE + i for i in range(kernels().h3w_variants)]
    if fam == "h3s":
        return [cf.H3S_BASE + i for i in range(kernels().h3s_variants)
                if layer.h3s_ok(shape) and layer.h3s_fits(i, shape, efficient=False)]
    assert layer.h3t_ok(shape)
    h3p = [cf.H3P_BASE + i for i in range(len(cf.H3P_BPC))] if layer.h3p_ok(shape) else []
    if fam in ("h3p_single", "h3p_band"):
        return h3p
    assert fam == "temporal", fam
    return ([cf.H3T_BASE + i for i in range(kernels().h3t_variants) if layer.h3t_fits(i, shape)]
            + [cf.H3U_BASE + i for i in range(kernels().h3u_variants)
               if layer.h3u_fits(i, shape)] + h3p)


def _precondition(case, d, which, layer, x, res, u_log2=tl.U_LOG2):
    """Span < 22 bits and lo coverage >= 0.4 of the case's data, asserted
    before any kernel runs; returns (span bits, coverage)."""
    from rnb_amd.ops import conv_f32 as cf
    h3w = case.family == "h3w"
    span = (tl.wino_span_bits(x.cpu(), layer, res, u_log2) if h3w
            else tl.span_bits(x.cpu(), layer, None, res, u_log2))
    if which == 1:
        xc = x[..., :case.cin].cpu()
        if h3w:
            _, lo, _ = tl.split_fp16(tl.wino_v(xc).float(), cf.H3W_IN_LOG2)
            cov = tl.lo_coverage(tl.wino_v(d.a_x), lo)
        else:
            _, lo, _ = tl.split_fp16(xc, cf.H3_IN_LOG2)
            cov = tl.lo_coverage(d.a_x, lo)
    elif h3w:
        u = tl.wino_u(d.w)
        _, lo, _ = tl.split_fp16(u, cf.H3_W_TOP_LOG2 - int(math.floor(math.log2(
            float(u.abs().max())))))
        cov = tl.lo_coverage(tl.wino_u(d.a_w), lo)
    else:
        _, lo, _ = tl.split_fp16(d.w, cf.h3_weight_scale_log2(d.w))
        cov = tl.lo_coverage(d.a_w, lo)
    print("h3lo %s pass %d: span %.2f bits, lo coverage %.3f" % (case.id, which, span, cov))
    assert span < tl.SPAN_LIMIT_BITS, (case.id, which, span)
    assert cov >= tl.MIN_LO_COVERAGE, (case.id, which, cov)
    return span, cov


def _exact_ref(layer, x, res):
    """The fp64 conv, which the span makes an exact fp32 number."""
    ref64 = tl.ref64(layer, x.cpu(), res)
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64)
    return ref


def _run_exact(case, with_res=True):
    """Both passes of one case on every fitting config: bit-exact against the
    fp64 conv (residual + ReLU where the family has them), padding channels
    zero. Returns the config ids."""
    ran = []
    for which in (1, 2):
        d = tl.make_data(case, which)
        layer = _build(case, d)
        x = d.x.to(DEV)
        res = d.res if with_res else None
        _precondition(case, d, which, layer, x, res)
        ref = _exact_ref(layer, x, res)
        ids = _ids(case, layer, x.shape)
        assert ids, "no %s config fits %s" % (case.family, case.id)
        resd = _pad_res(layer, res) if with_res else None
        for cid in ids:
            y = layer.forward_hip(x, resd, config=cid)
            torch.cuda.synchronize()
            bad = (y[..., :case.cout].cpu() != ref).sum().item()
            assert bad == 0, (case.id, which, cid, bad, ref.numel())
            assert torch.all(y[..., case.cout:] == 0), (case.id, which, cid)
        ran = ids
    print("h3lo %s: exact on configs %s" % (case.id, ran))
    return ran


def _case_ids(fam):
    return [c.id for c in tl.CASES[fam]]


# -- the exact tests -----------------------------------------------------------
@pytest.mark.parametrize("case", tl.CASES["direct"] + tl.CASES["direct_more"],
                         ids=_case_ids("direct") + _case_ids("direct_more"))
def test_h3_direct_two_level_exact(case):
    """Every direct config: 64 -> 150 1x3x3 (odd M tail, padded Cout, K = 18
    steps), the temporal tap skip at Cin 40 (2.5 steps of 16 per tap), the
    stem's 3-channel 7x7 gather, a 1x1x1 stride-2 conv."""
    assert len(_run_exact(case)) == len(_h3_ids())


@pytest.mark.parametrize("case", tl.CASES["splitk"], ids=_case_ids("splitk"))
def test_h3_splitk_two_level_exact(case):
    """Split-K configs: partials scaled back per split, summed by the reduce
    kernel -- exact too, the span bounds every partial."""
    _run_exact(case)


@pytest.mark.parametrize("case", tl.CASES["h3r"], ids=_case_ids("h3r"))
def test_h3_rowband_two_level_exact(case):
    """Row-band kernels (conv_h3r_kernel, conv_h3q_kernel): every variant
    whose band fits the frame, and Cin 512 (K = 4608, 144 steps)."""
    _run_exact(case)


@pytest.mark.parametrize("case", tl.CASES["temporal"], ids=_case_ids("temporal"))
def test_h3_temporal_two_level_exact(case):
    """conv_h3t_kernel and conv_h3p_kernel (conv_h3u_kernel when built) on
    the temporal shape list, Cin_p % 32 == 16 included."""
    _run_exact(case)


@pytest.mark.parametrize("case", tl.CASES["h3p_single"], ids=_case_ids("h3p_single"))
def test_h3p_single_range_two_level_exact(monkeypatch, case):
    """conv_h3p_kernel with a forced single pixel range: the lo side of the
    register double buffer carried across tasks, clips and videos."""
    from rnb_amd.ops import conv_f32
    monkeypatch.setattr(conv_f32, "H3P_BPC", (-1, -3))
    _run_exact(case)


@pytest.mark.parametrize("case", tl.CASES["h3p_band"], ids=_case_ids("h3p_band"))
def test_h3p_band_two_level_exact(case):
    """The frame-band form of conv_h3p_kernel: the lo part of halo frames."""
    _run_exact(case)


@pytest.mark.parametrize("case", tl.CASES["h3stem"], ids=_case_ids("h3stem"))
def test_h3stem_two_level_exact(case):
    _run_exact(case, with_res=False)


@pytest.mark.parametrize("case", tl.CASES["h3s"], ids=_case_ids("h3s"))
def test_h3s_two_level_exact(case):
    from rnb_amd.ops.native import kernels
    if kernels().h3s_variants == 0:
        pytest.skip("conv_h3s is an experiment kernel (python -m rnb_amd.build --exp)")
    _run_exact(case)


@pytest.mark.parametrize("case", tl.CASES["h3w"], ids=_case_ids("h3w"))
def test_h3w_two_level_exact(case):
    """Winograd h3: U = G g G^T (quarters of u) and V = B^T d B both carry lo
    parts; the span is taken in the Winograd domain, in units of u / 4."""
    _run_exact(case)


def test_controls_two_level_exact():
    """The same data through the fp32-MFMA kernel (config 0) and every x6
    direct config (bf16 hi + mid, third part zero): bit-exact, so a failure
    above is the h3 kernels' and not the data's."""
    from rnb_amd.ops.conv_f32 import X6D_BASE
    from rnb_amd.ops.native import kernels
    case = tl.CASES["direct"][0]
    ids = [0] + [X6D_BASE + i for i in range(len(kernels().x6_configs))]
    for which in (1, 2):
        d = tl.make_data(case, which)
        layer = _build(case, d)
        x = d.x.to(DEV)
        for t in (d.x[..., :case.cin], d.w):
            h = t.bfloat16()
            m = (t - h.float()).bfloat16()
            assert torch.equal(h.float() + m.float(), t)
        ref = _exact_ref(layer, x, d.res)
        resd = _pad_res(layer, d.res)
        for cid in ids:
            y = layer.forward_hip(x, resd, config=cid)
            torch.cuda.synchronize()
            assert torch.equal(y[..., :case.cout].cpu(), ref), (which, cid)
    print("h3lo controls exact: configs %s" % ids)


# -- input BN on load ----------------------------------------------------------
AFFINE_CASES = [tl.affine_case(c) for fam in ("direct", "splitk", "h3r", "temporal", "h3p_single",
                                              "h3p_band", "h3w") for c in tl.CASES[fam]]


@pytest.mark.parametrize("case", AFFINE_CASES, ids=[c.id for c in AFFINE_CASES])
def test_h3_input_bn_on_load_two_level_exact(monkeypatch, case):
    """Pass 1 with the producer's BN + ReLU applied on load: scale in {0.5, 1,
    2} and integer shift per video and channel make relu(x s + t) two-level
    at u / 2; two videos in one tile and a clip-less video; bit-exact against
    the fp64 conv of the applied input with and without the epilogue
    statistics. Padding taps and, in the banded h3p form, halo frames outside
    the clip must contribute nothing although the BN would turn their zeros
    into relu(shift)."""
    if case.family == "h3p_single":
        from rnb_amd.ops import conv_f32
        monkeypatch.setattr(conv_f32, "H3P_BPC", (-1, -3))
    d = tl.make_data(case, 1)
    layer = _build(case, d, relu=False)
    seg = tl.affine_seg(case.n)
    ss = tl.affine_rows(3, layer.geom.cin_p)
    assert (ss[:, 1] > 0).any()
    xa = tl.apply_affine(d.x, ss, seg, case.cin)
    d.a_x = tl.affine_level(xa[..., :case.cin])
    _precondition(case, d, 1, layer, xa, None, u_log2=tl.U_LOG2 - 1)
    ref = _exact_ref(layer, xa, None)
    x, ss, seg = d.x.to(DEV), ss.to(DEV), seg.to(DEV)
    ids = [c for c in _ids(case, layer, x.shape) if layer.affine_ok(c, x.shape)]
    assert ids, case.id
    for cid in ids:
        sums = torch.zeros((3, 2, layer.geom.cout_p), dtype=torch.float64, device=DEV)
        for ost in (None, (sums, seg)):
            y = layer.forward_hip(x, config=cid, in_affine=(ss, seg), out_stats=ost)
            torch.cuda.synchronize()
            bad = (y[..., :case.cout].cpu() != ref).sum().item()
            assert bad == 0, (case.id, cid, ost is not None, bad)
    print("h3lo %s: exact on configs %s" % (case.id, ids))


# -- the test sees a lo fault, the integer data does not -----------------------
def _lo_chunks(row):
    from rnb_amd.ops.conv_f32 import _X6_S
    return [(2 * q + 1) ^ _X6_S[(row % 16) >> 1] for q in range(4)]


MUT_ROW, MUT_ROWS, MUT_STEP = 37, (34, 35), 7      # rows 34 / 35 share a swizzle


def _mutated_direct(orig, mode):
    def packer(wmat, sw):
        w = orig(wmat, sw).clone()                # [steps, rows, 8 chunks, 8]
        if mode == "zero":
            step = min(MUT_STEP, w.shape[0] - 1)
            for c in _lo_chunks(MUT_ROW):
                w[step, MUT_ROW, c] = 0
        else:
            a, b = MUT_ROWS
            assert _lo_chunks(a) == _lo_chunks(b)
            for c in _lo_chunks(a):
                t = w[:, a, c].clone()
                w[:, a, c] = w[:, b, c]
                w[:, b, c] = t
        return w
    return packer


def _mutated_h3w(orig, mode):
    def packer(w, cin_p, cout, tc):
        u, sw = orig(w, cin_p, cout, tc)          # [ci/16, nb, 16, ct, 4 chunks, 8 = Uh | Ul]
        u = u.clone()
        ct = u.shape[3]
        if mode == "zero":
            u[1, MUT_ROW // ct, :, MUT_ROW % ct, :, 4:] = 0
        else:
            a, b = MUT_ROWS
            assert a // ct == b // ct and (a % 16) >> 2 == (b % 16) >> 2
            t = u[:, a // ct, :, a % ct, :, 4:].clone()
            u[:, a // ct, :, a % ct, :, 4:] = u[:, b // ct, :, b % ct, :, 4:]
            u[:, b // ct, :, b % ct, :, 4:] = t
        return u, sw
    return packer


def _mutation_targets():
    from rnb_amd.ops import conv_f32 as cf
    return [("direct", tl.CASES["direct"][0], cf.H3D_BASE + 0),
            ("rowband", tl.CASES["h3r"][0], None),
            ("temporal", tl.CASES["temporal"][1], None),      # Cin 64: the h3d layout
            ("h3w", tl.CASES["h3w"][0], cf.H3W_BASE + 0)]


@pytest.mark.parametrize("mode", ["zero", "swap"])
@pytest.mark.parametrize("target", range(4), ids=["direct", "rowband", "temporal", "h3w"])
def test_two_level_data_sees_a_lo_fault_in_the_packer(monkeypatch, target, mode):
    """The packer, patched to zero the lo chunks of one 32-channel step of one
    output row (or to swap the lo chunks of two rows), on the unmodified
    kernel: pass 2 differs from the fp64 conv in exactly that output channel
    (those two) and equals it everywhere else -- while the integer data of the
    existing tests, through the same patched packer, still passes: the gap
    this file closes."""
    from rnb_amd.ops import conv_f32 as cf
    name, case, cid = _mutation_targets()[target]
    if name == "h3w":
        monkeypatch.setattr(cf, "h3w_weights", _mutated_h3w(cf.h3w_weights, mode))
    else:
        monkeypatch.setattr(cf, "h3_direct_weights", _mutated_direct(cf.h3_direct_weights, mode))
    d = tl.make_data(case, 2)
    layer = _build(case, d, relu=False)
    x = d.x.to(DEV)
    if cid is None:
        cid = _ids(case, layer, x.shape)[0]
    ref = _exact_ref(layer, x, None)
    y = layer.forward_hip(x, config=cid)
    torch.cuda.synchronize()
    diff = (y[..., :case.cout].cpu() != ref).reshape(-1, case.cout).any(0)
    hit = sorted(torch.nonzero(diff).flatten().tolist())
    print("h3lo mutation %s %s cid %d: channels that differ %s" % (name, mode, cid, hit))
    assert hit == ([MUT_ROW] if mode == "zero" else list(MUT_ROWS)), (name, mode, cid, hit)
    # the integer data of the existing exact tests (lo = 0 everywhere), layer
    # built through the same patched packer, cannot see it
    li = (_tlayer(64, 150, relu=True, integer=True) if name == "temporal"
          else _layer(64, 150, *tl.SPATIAL, relu=True, integer=True))
    xi = _input(2, case.thw, 64, 64, integer=True)
    ri = _input(2, case.thw, li.geom.cout_p, 150, integer=True, seed=3)
    yi = li.forward_hip(xi, ri, config=cid)
    torch.cuda.synchronize()
    assert torch.equal(yi[..., :150].cpu(), _ref64(li, xi, ri).float()), (name, mode, cid)


# -- fp32-class error, every family --------------------------------------------
def _err_layers():
    """(name, layer, clips, (T, H, W), families of config ids, fp32 baseline
    id) at the small shapes of the exact tests."""
    from rnb_amd.ops import conv_f32 as cf
    sp = tl.SPATIAL
    out = []
    lay = _layer(64, 150, *sp)
    out.append(("direct", lay, 2, (2, 15, 13), "direct", 0))
    out.append(("splitk", lay, 3, (1, 7, 7), "splitk", 0))
    out.append(("h3r", lay, 2, (2, 15, 13), "h3r", 0))
    out.append(("h3r", lay, 2, (2, 28, 28), "h3r", 0))
    out.append(("h3w", lay, 2, (2, 15, 13), "h3w", cf.WINO_DEFAULT))
    for thw, cin, cout, fam in (((8, 8, 8), 144, 64, "temporal"), ((4, 4, 8), 288, 128, "temporal"),
                                ((8, 8, 8), 83, 64, "temporal"),
                                ((16, 4, 4), 144, 64, "h3p_band")):
        out.append((fam, _tlayer(cin, cout), 3, thw, fam, 0))
    for thw, cout in (((1, 19, 17), 72), ((2, 30, 112), 40)):
        out.append(("h3stem", _layer(3, cout, *tl.STEM), 2, thw, "h3stem", 0))
    return out


def _band_input(n, thw, cin_p, cin, lo, hi, seed=1):
    """|a| uniform in [lo, hi], signs random."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) + thw + (cin_p,)
    x = lo + (hi - lo) * torch.rand(shape, generator=g)
    x = x * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    x[..., cin:] = 0
    return x.to(DEV)


ERR_INPUTS = [("amp 1", lambda n, thw, cp, c: _input(n, thw, cp, c)),
              ("amp 1e-3", lambda n, thw, cp, c: _input(n, thw, cp, c) * 1e-3),
              ("|a| in [2^-9, 2^-8]", lambda n, thw, cp, c: _band_input(
                  n, thw, cp, c, 2.0 ** -9, 2.0 ** -8)),
              ("|a| in [2^8, 2^9.9]", lambda n, thw, cp, c: _band_input(
                  n, thw, cp, c, 2.0 ** 8, 2.0 ** 9.9))]


ERR_IDS = ["direct", "splitk", "h3r-15x13", "h3r-28x28", "h3w", "temporal-144x64",
           "temporal-288x128", "temporal-83x64", "h3p_band", "h3stem-19x17", "h3stem-30x112"]


@pytest.mark.parametrize("which", range(len(ERR_IDS)), ids=ERR_IDS)
def test_h3_error_is_fp32_class_every_family(which):
    """test_h3_error_is_fp32_class for every family and config: the h3 error
    against fp64 within 8x the error of the fp32 kernel of the same algorithm
    (config 0; the fp32 Winograd F(2x2, 3x3) for h3w), and within 1e-5, at
    amplitudes 1 and 1e-3 and at the documented range edges -- |a| in [2^-9,
    2^-8], where lo parts are at the bottom of the normal fp16 range, and in
    [2^8, 2^9.9], the top of the input range, where an activated RangeGuard
    must not trip."""
    from rnb_amd.ops.conv_f32 import RangeGuard
    from rnb_amd.ops.native import kernels
    layers = _err_layers()
    assert len(layers) == len(ERR_IDS)
    name, layer, n, thw, fam, base = layers[which]
    g = layer.geom
    case = SimpleNamespace(family=fam)
    guard = RangeGuard()
    fails = []
    try:
        for label, make in ERR_INPUTS:
            x = make(n, thw, g.cin_p, g.cin)
            ids = _ids(case, layer, x.shape)
            assert ids, (name, thw)
            ref = _ref64(layer, x)
            scale = ref.abs().max().item()
            y32 = layer.forward_hip(x, config=base)
            torch.cuda.synchronize()
            e32 = (y32[..., :g.cout].double().cpu() - ref).abs().max().item() / scale
            top = label.startswith("|a| in [2^8")
            if top:
                guard.activate()
                guard.reset()
            for cid in ids:
                yh = layer.forward_hip(x, config=cid)
                torch.cuda.synchronize()
                eh = (yh[..., :g.cout].double().cpu() - ref).abs().max().item() / scale
                print("h3lo err %s %dx%d %s %s cid %d: eh %.3e e32 %.3e ratio %.2f" % (
                    name, g.cin, g.cout, "x".join(map(str, thw)), label, cid, eh, e32,
                    eh / max(e32, 2 ** -24)))
                if not (eh <= 1e-5 and eh <= 8 * max(e32, 2 ** -24)):
                    fails.append((label, cid, eh, e32))
            if top:
                assert not guard.tripped(), (name, thw)
                kernels().h3_set_range_flag(0)
    finally:
        kernels().h3_set_range_flag(0)
    assert not fails, fails
