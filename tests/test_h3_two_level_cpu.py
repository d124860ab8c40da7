"""The premises of tests/test_gpu_h3_lo_path.py, checked without a GPU.

Two-level data (tests/h3_two_level.py) only pins the h3 kernels' lo path if
its split is exact and non-trivial at the kernels' scales, if every output's
span leaves fp32 room for any summation order, if the host packers carry the
lo parts where the kernels read them, and if a lost or misplaced lo term
moves the answer by at least one fp32 ulp. Each is asserted here on the very
tensors the GPU tests use.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import h3_two_level as tl
from rnb_amd.ops import conv_f32 as cf

AFFINE_FAMILIES = ("direct", "splitk", "h3r", "temporal", "h3p_single", "h3p_band", "h3w")
AFFINE_CASES = [tl.affine_case(c) for fam in AFFINE_FAMILIES for c in tl.CASES[fam]]


def _host(case, d, relu=True):
    return tl.host_layer(d.w, d.b, case.k, case.s, case.p, relu)


def _u_scale_log2(u):
    return cf.H3_W_TOP_LOG2 - int(math.floor(math.log2(float(u.abs().max()))))


@pytest.mark.parametrize("case", tl.ALL_CASES, ids=[c.id for c in tl.ALL_CASES])
def test_two_level_split_is_exact_and_spans_fit(case):
    """hi + lo == v for the two-level operand at the kernels' scale (2^6 for
    activations, 2^4 for the Winograd V, h3_weight_scale_log2 for weights),
    lo == 0 for its fp16-exact partner, lo coverage >= 0.4, span < 22 bits."""
    h3w = case.family == "h3w"
    for which in (1, 2):
        d = tl.make_data(case, which)
        lay = _host(case, d)
        span = tl.wino_span_bits(d.x, lay, d.res) if h3w else tl.span_bits(d.x, lay, d.b, d.res)
        assert span < tl.SPAN_LIMIT_BITS, (which, span)
        x = d.x[..., :case.cin]
        xh, xl, xs = tl.split_fp16(x, cf.H3_IN_LOG2)
        wh, wl, ws = tl.split_fp16(d.w, cf.h3_weight_scale_log2(d.w))
        assert torch.equal(xh.float() + xl.float(), xs) and torch.equal(wh.float() + wl.float(), ws)
        assert float(ws.abs().max()) < 2.0 ** 14 and float(xs.abs().max()) < 65504
        if h3w:
            v = tl.wino_v(x)
            assert torch.equal(v.float().double(), v)           # V is exact in fp32
            vh, vl, vs = tl.split_fp16(v.float(), cf.H3W_IN_LOG2)
            assert torch.equal(vh.float() + vl.float(), vs)
            u = tl.wino_u(d.w)
            uh, ul, us = tl.split_fp16(u, _u_scale_log2(u))
            assert torch.equal(uh.double() + ul.double(), us)
        if which == 1:
            assert not wl.any()
            cov = (tl.lo_coverage(tl.wino_v(d.a_x), vl) if h3w else tl.lo_coverage(d.a_x, xl))
            # a lo part below fp16's normal range would depend on denormal handling
            lo = (vl if h3w else xl).float().abs()
            assert float(lo[lo > 0].min()) >= 2.0 ** -14
        else:
            assert not xl.any()
            cov = (tl.lo_coverage(tl.wino_u(d.a_w), ul) if h3w else tl.lo_coverage(d.a_w, wl))
        assert cov >= tl.MIN_LO_COVERAGE, (which, cov)
        # the answer itself is an fp32 number
        ref = tl.ref64(lay, d.x, d.res)
        assert torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize("case", AFFINE_CASES, ids=[c.id for c in AFFINE_CASES])
def test_affine_applied_input_is_two_level_at_half_u(case):
    """relu(x s + t) with s in {0.5, 1, 2} and integer t: multiples of u / 2,
    split exactly at the kernels' scale, span (units of u / 2) < 22 bits,
    lo coverage over its non-zero levels >= 0.4; some shift is positive, so a
    padding tap or halo frame run through the BN would show."""
    d = tl.make_data(case, 1)
    cp = d.x.shape[-1]
    ss = tl.affine_rows(3, cp)
    seg = tl.affine_seg(case.n)
    assert seg.tolist().count(1) == 0 and len(set(seg.tolist())) == 2
    assert (ss[:, 1] > 0).any() and set(ss[:, 0].flatten().tolist()) <= {0.5, 1.0, 2.0}
    xa = tl.apply_affine(d.x, ss, seg, case.cin)
    q = xa.double() * 2.0 ** (1 - tl.U_LOG2)
    assert torch.equal(q, q.round())
    lay = _host(case, d, relu=False)
    h3w = case.family == "h3w"
    span = (tl.wino_span_bits(xa, lay, None, tl.U_LOG2 - 1) if h3w
            else tl.span_bits(xa, lay, d.b, None, tl.U_LOG2 - 1))
    assert span < tl.SPAN_LIMIT_BITS, span
    t = tl.wino_v(xa[..., :case.cin]).float() if h3w else xa[..., :case.cin]
    h, lo, s = tl.split_fp16(t, cf.H3W_IN_LOG2 if h3w else cf.H3_IN_LOG2)
    assert torch.equal(h.float() + lo.float(), s)
    lvl = tl.affine_level(xa[..., :case.cin])
    assert tl.lo_coverage(tl.wino_v(lvl) if h3w else lvl, lo) >= tl.MIN_LO_COVERAGE


def _unpack_direct(packed, rows, k_pad):
    """h3_direct_weights' layout back to (hi, lo) [rows, K] fp16."""
    steps = k_pad // 32
    phys = packed.view(torch.float16).reshape(steps, rows, 8, 8).permute(1, 0, 2, 3)
    s = torch.tensor([cf._X6_S[(r % 16) >> 1] for r in range(rows)], dtype=torch.int64)
    idx = torch.arange(8, dtype=torch.int64)[None, :] ^ s[:, None]
    logical = phys.gather(2, idx[:, None, :, None].expand_as(phys))     # the xor is its own inverse
    chunks = logical.reshape(rows, steps, 4, 2, 8)                      # [.., quad, hi / lo, 8]

    def unlay(t):                  # [rows, steps, quad, (sub, 4)] -> [rows, K]
        return t.reshape(rows, steps, 4, 2, 4).permute(0, 1, 3, 2, 4).reshape(rows, k_pad)
    return unlay(chunks[..., 0, :]), unlay(chunks[..., 1, :])


@pytest.mark.parametrize("case", [tl.CASES["direct"][0], tl.CASES["h3r"][4], tl.CASES["temporal"][5]],
                         ids=["k576", "k4608", "k1728"])
def test_h3_direct_weights_carry_the_lo_parts(case):
    """h3_direct_weights on pass-2 weights: un-swizzled, hi + lo is the
    scaled weight exactly, and the lo plane is non-zero."""
    d = tl.make_data(case, 2)
    wmat = d.w.permute(0, 2, 3, 4, 1).reshape(case.cout, -1)          # k = tap * Cin + c
    k_pad = (wmat.shape[1] + 31) // 32 * 32
    rows = case.cout + 10
    full = torch.zeros(rows, k_pad)
    full[:case.cout, :wmat.shape[1]] = wmat
    sw = cf.h3_weight_scale_log2(full)
    hi, lo = _unpack_direct(cf.h3_direct_weights(full, sw), rows, k_pad)
    assert torch.equal(hi.float() + lo.float(), full * 2.0 ** sw)
    a = d.a_w.permute(0, 2, 3, 4, 1).reshape(case.cout, -1)
    assert tl.lo_coverage(a, lo[:case.cout, :a.shape[1]]) >= tl.MIN_LO_COVERAGE
    assert not lo[case.cout:].any()


@pytest.mark.parametrize("tc", [1, 2, 3])
def test_h3w_weights_carry_the_lo_parts(tc):
    """h3w_weights on pass-2 weights: un-swizzled, Uh + Ul is U * 2^sw
    exactly and the Ul halves are non-zero."""
    case = tl.CASES["h3w"][0]
    d = tl.make_data(case, 2)
    cin_p, ct = case.cin, 16 * tc
    packed, sw = cf.h3w_weights(d.w, cin_p, case.cout, tc)
    nb = (case.cout + ct - 1) // ct
    phys = packed.view(torch.float16).reshape(cin_p // 16, nb, 16, ct, 4, 8)
    s = torch.tensor([cf._WINO_SWZ[(r % 16) >> 2] for r in range(ct)], dtype=torch.int64)
    idx = torch.arange(4, dtype=torch.int64)[None, :] ^ s[:, None]
    logical = phys.gather(4, idx[None, None, None, :, :, None].expand_as(phys))

    def unlay(t):                   # [ci/16, nb, 16x, ct, quad, 4] -> [nb * ct, ci, 16x]
        return t.permute(1, 3, 0, 4, 5, 2).reshape(nb * ct, cin_p, 16)
    uh, ul = unlay(logical[..., :4]), unlay(logical[..., 4:])
    u = tl.wino_u(d.w).reshape(case.cout, case.cin, 16)
    assert sw == _u_scale_log2(u)
    assert torch.equal(uh[:case.cout].double() + ul[:case.cout].double(), u * 2.0 ** sw)
    assert not uh[case.cout:].any() and not ul[case.cout:].any()
    cov = tl.lo_coverage(tl.wino_u(d.a_w).reshape(case.cout, case.cin, 16), ul[:case.cout])
    assert cov >= tl.MIN_LO_COVERAGE, cov


def test_a_lost_or_swapped_lo_term_moves_the_answer_by_an_ulp():
    """The emulated three-product sum ah bh + al bh + ah bl (fp64) of the
    direct case equals the fp64 conv on both passes; dropping the weight-lo
    terms of one 32-channel step of one tap of one output row, or swapping
    the weight-lo terms of two rows, moves every output it moves at all by
    at least one fp32 ulp of the result -- torch.equal cannot miss it."""
    case = tl.CASES["direct"][0]
    conv = lambda x, w: F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.double(), None,      # noqa: E731
                                 stride=case.s, padding=case.p).permute(0, 2, 3, 4, 1)
    for which in (1, 2):
        d = tl.make_data(case, which)
        sw = cf.h3_weight_scale_log2(d.w)
        xh, xl, _ = tl.split_fp16(d.x[..., :case.cin], cf.H3_IN_LOG2)
        wh, wl, _ = tl.split_fp16(d.w, sw)
        unscale = 2.0 ** -(cf.H3_IN_LOG2 + sw)
        three = (conv(xh, wh) + conv(xl, wh) + conv(xh, wl)) * unscale
        lay = _host(case, d, relu=False)
        ref = tl.ref64(lay, d.x) - d.b.double()
        assert torch.equal(three, ref), which
        assert not (conv(xl, wl) != 0).any()                  # the fourth product is zero
        ulp = (torch.nextafter(tl.ref64(lay, d.x).float().abs(),
                               torch.tensor(float("inf"))) - tl.ref64(lay, d.x).float().abs()).double()
        if which == 1:
            # the activation-lo terms of channels 32..63: lost in the in-kernel split
            m = torch.zeros_like(xl)
            m[..., 32:] = xl[..., 32:]
            deltas = [conv(m, wh) * unscale]
        else:
            drop = torch.zeros_like(wl)
            drop[37, 32:, 0, 1, 0] = wl[37, 32:, 0, 1, 0]
            swap = torch.zeros_like(wl).double()
            swap[34] = wl[35].double() - wl[34].double()
            swap[35] = wl[34].double() - wl[35].double()
            deltas = [conv(xh, drop) * unscale, conv(xh, swap) * unscale]
        for delta in deltas:
            moved = delta != 0
            assert moved.any()
            assert (delta.abs()[moved] >= ulp[moved]).all()
