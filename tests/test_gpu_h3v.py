"""The volume-band h3 conv (csrc/conv_h3v.hip) on the GPU: the 3x3x3 convs of
torchvision's r3d_18 on every kernel config offered for them, against an fp64
conv (the shape of tests/test_gpu_tv_arch.py), and the range guard."""
import pytest
import torch

from test_gpu_f32 import DEV, _input, _ref64

pytestmark = pytest.mark.gpu

K333, K133 = (3, 3, 3), (1, 3, 3)
# name: (cin, cout, kernel, stride, padding, (T, H, W), clips)
GEOMS = {
    "v32_t3_7x5": (32, 48, K333, (1, 1, 1), (1, 1, 1), (3, 7, 5), 2),
    "v64_t2_9x16": (64, 64, K333, (1, 1, 1), (1, 1, 1), (2, 9, 16), 3),
    "v64_56": (64, 64, K333, (1, 1, 1), (1, 1, 1), (4, 56, 56), 1),
    "v128_28": (128, 128, K333, (1, 1, 1), (1, 1, 1), (4, 28, 28), 2),
    "v256_14": (256, 256, K333, (1, 1, 1), (1, 1, 1), (2, 14, 14), 3),
    "v512_7": (512, 512, K333, (1, 1, 1), (1, 1, 1), (2, 7, 7), 2),
    "s2_128": (64, 128, K333, (2, 2, 2), (1, 1, 1), (4, 12, 12), 2),
    # one frame: the engine runs the conv as its centre 1x3x3 slice
    "t1_512": (512, 512, K133, (1, 1, 1), (0, 1, 1), (1, 7, 7), 2),
}


def _layer(case, relu=True, integer=False, seed=0):
    from rnb_amd.ops.conv import ConvGeom
    from rnb_amd.ops.conv_f32 import F32_ALIGN, ConvLayerF32
    cin, cout, k, s, p, _, _ = case
    g = torch.Generator().manual_seed(seed)
    if integer:
        w = torch.randint(-2, 3, (cout, cin) + k, generator=g).float()
        b = torch.randint(-4, 5, (cout,), generator=g).float()
    else:
        w = torch.randn((cout, cin) + k, generator=g) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
    geom = ConvGeom(cin=cin, cout=cout, kernel=k, stride=s, padding=p, align=F32_ALIGN)
    return ConvLayerF32(w, b, geom, relu, DEV, "h3vtest")


def _ids(layer, x_shape):
    """candidates() plus every h3v variant that has a box at all."""
    from rnb_amd.ops.conv_f32 import H3V_BASE
    from rnb_amd.ops.native import kernels
    ids = layer.candidates(x_shape)
    if layer.h3v_ok(x_shape):
        ids = ids + [H3V_BASE + v for v in range(kernels().h3v_variants)
                     if H3V_BASE + v not in ids and layer.h3v_fits(v, x_shape, efficient=False)]
    return ids


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_every_candidate_of_every_r3d_geometry(name):
    """Every id: bit-equal to the fp64 conv on small integers (|w| <= 2, |x| <=
    3: partial sums <= 13 824 x 6 < 2^17) with a residual and ReLU; within 1e-5
    on normal data; pad channels zero; per-video epilogue sums. h3v is offered
    on the stride-1 cases with T >= 2 only; one frame gets the row bands."""
    from rnb_amd.ops.conv_f32 import is_h3r, is_h3v, is_x6d, WINO_ALL
    from rnb_amd.ops.native import kernels
    case = GEOMS[name]
    cin, cout, k, s, p, thw, n = case
    li, lf = _layer(case, integer=True), _layer(case, relu=False)
    cin_p, cout_p = li.geom.cin_p, li.geom.cout_p
    xi = _input(n, thw, cin_p, cin, integer=True)
    oshape = li.out_shape(xi.shape)
    res = _input(n, tuple(oshape[1:4]), cout_p, cout, integer=True, seed=3)
    ref_i = _ref64(li, xi, res).float().to(DEV)
    xf = _input(n, thw, cin_p, cin)
    ref_f = _ref64(lf, xf).to(DEV)
    scale = ref_f.abs().max().item()
    ids = _ids(li, xi.shape)
    assert len(ids) == len(set(ids))
    offered = [c for c in li.candidates(xi.shape) if is_h3v(c)]
    if k == K333 and s == (1, 1, 1):
        assert offered or any(is_h3v(c) for c in ids), "no h3v id for %s" % name
        if name in ("v128_28", "v256_14", "v512_7"):
            assert offered, "r3d_18's own shape %s has no efficient h3v variant" % name
    else:
        assert not any(is_h3v(c) for c in ids)
    if name == "t1_512":
        assert any(is_h3r(c) for c in ids)
    seg = torch.tensor([0] * (n // 2) + [1] * (n - n // 2), dtype=torch.int32, device=DEV)
    bounds = [(0, n // 2), (n // 2, n)]
    nf32 = len(kernels().f32_configs)
    err_of, failures = {}, []
    for cid in ids:
        y = li.forward_hip(xi, res, config=cid)
        if not torch.equal(y[..., :cout], ref_i):
            failures.append("cid %d: integers differ by up to %.3e"
                            % (cid, (y[..., :cout] - ref_i).abs().max().item()))
        if not torch.all(y[..., cout:] == 0):
            failures.append("cid %d: pad channels not zero (integers)" % cid)
        stats = cid in WINO_ALL or is_x6d(cid)
        sums = torch.zeros((2, 2, cout_p), dtype=torch.float64, device=DEV)
        y = lf.forward_hip(xf, config=cid, out_stats=(sums, seg) if stats else None)
        err_of[cid] = (y[..., :cout].double() - ref_f).abs().max().item() / scale
        if not torch.all(y[..., cout:] == 0):
            failures.append("cid %d: pad channels not zero" % cid)
        if stats:
            yd = y[..., :cout].double()
            for v, (a, b) in enumerate(bounds):
                part = yd[a:b].reshape(-1, cout)
                got = sums[v, :, :cout]
                if not ((got[0] - part.sum(0)).abs() <= 1e-6 * part.abs().sum(0) + 1e-9).all():
                    failures.append("cid %d: epilogue sums of video %d" % (cid, v))
                if not torch.allclose(got[1], (part * part).sum(0), rtol=1e-6, atol=1e-9):
                    failures.append("cid %d: epilogue square sums of video %d" % (cid, v))
    torch.cuda.synchronize()
    # 1e-5, the project's bound; on v512_7 (K = 13 824) twice the worst generic
    # fp32-MFMA config's error where that itself passes 1e-5 -- never from h3v
    worst_f32 = max(err_of[c] for c in ids if c < nf32)
    bound = 2 * worst_f32 if name == "v512_7" and worst_f32 > 1e-5 else 1e-5
    print("%s: %d ids, worst fp32-MFMA %.3e, worst h3v %.3e, bound %.1e"
          % (name, len(ids), worst_f32, max([err_of[c] for c in ids if is_h3v(c)] or [0.0]), bound))
    failures += ["cid %d: rel err %.3e > %.1e" % (c, e, bound) for c, e in err_of.items()
                 if e > bound]
    assert not failures, failures[:8]


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_range_guard_trips_on_every_variant(variant):
    """Amplitude 2^12 passes the fp16 range after the 2^6 input scale: the flag
    is set; inside ``full_range()`` the layer's config is not an h3 one."""
    from rnb_amd.ops.conv_f32 import H3V_BASE, RangeGuard, full_range, is_h3
    from rnb_amd.ops.native import kernels
    case = GEOMS["v64_t2_9x16"]
    cin, _, _, _, _, thw, n = case
    layer = _layer(case, relu=False)
    assert layer.h3v_fits(variant, (n,) + thw + (cin,), efficient=False)
    guard = RangeGuard()
    guard.activate()
    try:
        x = _input(n, thw, layer.geom.cin_p, cin)
        layer.forward_hip(x, config=H3V_BASE + variant)
        torch.cuda.synchronize()
        assert not guard.tripped()
        layer.forward_hip(x * 4096.0, config=H3V_BASE + variant)
        torch.cuda.synchronize()
        assert guard.tripped()
    finally:
        kernels().h3_set_range_flag(0)
    layer._config[tuple(x.shape[:4])] = H3V_BASE + variant
    assert is_h3(layer.config_for(x.shape))
    with full_range():
        assert not is_h3(layer.config_for(x.shape))
