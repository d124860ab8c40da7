"""``yuv420_to_clip(filter="antialias")``: the fp64 oracle of
``decode_oracle_aa.py`` against PIL and torch (implementations this project did
not write), the oracle's own properties, the CPU mirror against the oracle, the
stripe pattern that two taps turn into moire, the refusals, the two configs and
``MjpegDecoder(filter="antialias")`` against PIL's resized RGB.

The ``check_*`` functions take the device: ``test_gpu_decode_aa.py`` runs the
same cases, byte-identical inputs and the same bounds on the HIP kernel. Every
bound comes from the oracle (``tolerance_aa``) or is stated where it is used,
never from the code under test. Run with ``-s`` for the figures."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn
from PIL import Image

import decode_oracle as orc
import decode_oracle_aa as aa
from rnb_amd.config import load_pipeline
from rnb_amd.models.r2p1d.decoder import MjpegDecoder, Y4mDecoder, make_decoder
from rnb_amd.ops import video as vops
from rnb_amd.ops.video import FILTERS       # the feature under test: absent, nothing here runs
from rnb_amd.utils import mjpeg
from test_decode_oracle_cpu import sync, to_np
from test_mjpeg_cpu import GOLDEN, GOLDEN_STREAMS, frame_bytes

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (src_w, src_h, out_w, out_h, box): the shapes the definition was checked on
PLANE_SHAPES = [
    (340, 256, 112, 112, None),
    (340, 256, 112, 112, (42, 0, 256, 256)),
    (46, 34, 16, 12, (3.5, 1.25, 40, 30)),
    (23, 17, 16, 12, None),
    (16, 12, 40, 30, None),
    (480, 270, 28, 28, (10.5, 3.25, 400, 250)),
]
PLANE_IDS = ["%dx%d_to_%dx%d_%s" % (s[:4] + ("box" if s[4] else "full",)) for s in PLANE_SHAPES]
PIL_BOUND = 1e-4          # levels; PIL mixes fp32 and double: measured 1.34e-5, margin 8x
TORCH_BOUND = 1e-9        # levels; torch in fp64: measured 8.5e-14
PIL_DECODER_MARGIN = 0.05     # levels: anchor_bound's margin for rounding of the comparison


def noise_plane(w, h):
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (1, h, w), dtype=np.uint8)


def pil_resize(plane2d, out_w, out_h, box):
    """PIL's antialiased triangle filter on one float plane (mode ``F``)."""
    x, y, w, h = box
    img = Image.fromarray(np.ascontiguousarray(plane2d, dtype=np.float32), "F")
    return np.asarray(img.resize((out_w, out_h), Image.BILINEAR, box=(x, y, x + w, y + h)),
                      dtype=np.float64)


# -- the oracle against PIL and torch -------------------------------------------------------
@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=PLANE_IDS)
def test_oracle_against_pil(shape):
    w, h, ow, oh, box = shape
    p = noise_plane(w, h)
    box = box or (0, 0, w, h)
    err = float(np.abs(aa.resample_aa(p, ow, oh, box)[0] - pil_resize(p[0], ow, oh, box)).max())
    print("oracle vs PIL %s: max %.3g levels" % (shape, err))
    assert err <= PIL_BOUND, err


@pytest.mark.parametrize("shape", [s for s in PLANE_SHAPES if s[4] is None],
                         ids=[i for s, i in zip(PLANE_SHAPES, PLANE_IDS) if s[4] is None])
def test_oracle_against_torch_fp64(shape):
    w, h, ow, oh, _ = shape
    p = noise_plane(w, h)
    want = Fn.interpolate(torch.from_numpy(p.astype(np.float64))[None], size=(oh, ow),
                          mode="bilinear", antialias=True, align_corners=False)[0, 0].numpy()
    err = float(np.abs(aa.resample_aa(p, ow, oh, (0, 0, w, h))[0] - want).max())
    print("oracle vs torch fp64 %s: max %.3g levels" % (shape, err))
    assert err <= TORCH_BOUND, err


def test_aa_matrix_is_the_bilinear_matrix_when_not_downscaling():
    """scale <= 1 on a box inside the plane: today's hat with edge replication."""
    for args in ((6, 17, 0, 6), (4, 9, 0, 4), (1, 3, 0, 1), (1, 3, 0, 0.5), (23, 24, 1.5, 18),
                 (46, 46, 0, 46), (34, 40, 0, 34), (12, 30, 0.25, 11.5)):
        assert args[3] / args[1] <= 1
        diff = np.abs(aa.aa_matrix(*args) - orc.resample_matrix(*args)).max()
        assert diff <= 1e-12, (args, diff)


def test_aa_matrix_rows_and_truncation():
    """Every row sums to 1 and is non-negative; the matrix has exactly n_src
    columns (nothing beyond the true samples can carry weight), and rows whose
    support reaches past an edge are renormalised, not edge-replicated."""
    for args in ((46, 16, 0, 46), (46, 16, 3.5, 40), (17, 12, 1.25, 15), (98, 5, 0, 98),
                 (62, 3, 0, 62), (3, 1, 0, 3), (23, 16, 0, 23), (1, 1, 0, 1), (48, 16, 0, 45)):
        M = aa.aa_matrix(*args)
        assert M.shape == (args[1], args[0]) and M.min() >= 0
        assert np.allclose(M.sum(axis=1), 1.0, atol=1e-12), args
    # 3 -> 1: s = 1, fs = 3, weights (2/3, 1, 2/3) / (7/3); replication would add the
    # outer samples' weight 1/3 twice to the edges: (3/9, 3/9, 3/9)
    assert np.allclose(aa.aa_matrix(3, 1, 0, 3)[0], [2 / 7, 3 / 7, 2 / 7], atol=1e-15)
    # 45 true samples (in a surface 48 wide): the last row, s = 43.09 and fs = 2.8125,
    # would reach sample 45; it is cut at 44
    M = aa.aa_matrix(45, 16, 0, 45)
    assert np.nonzero(M[-1])[0].tolist() == [41, 42, 43, 44]
    with pytest.raises(AssertionError):
        aa.aa_matrix(46, 4, -40, 8)


def test_oracle_aa_module_takes_nothing_from_the_ops():
    import ast
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), "decode_oracle_aa.py")).read())
    imports = [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
    seen = sorted((getattr(n, "module", ""), a.name) for n in imports for a in n.names)
    assert seen == [("", "decode_oracle"), ("", "math"), ("", "numpy")]
    used = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)} | \
        {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)}
    assert not used & {"_antialias_weights", "_antialias_torch", "_planes_to_clip",
                       "yuv420_to_clip", "torch", "vops", "__import__", "importlib"}


# -- running the op under test ---------------------------------------------------------------
def make_runner(layout, matrix, y, u, v, out_w, out_h, crop, device, clips=1,
                filter="antialias"):
    """``run(dtype, out=None)`` -> [frames, out_h, out_w, C] on ``device``."""
    frames, h, w = y.shape
    data, stride, pl = orc.PACKERS[layout](y, u, v)
    buf = torch.from_numpy(data).to(device)
    F = frames // clips
    offs = [c * F * stride for c in range(clips)]

    def run(dtype, out=None):
        if out is not None:
            out = out.view((clips, F) + tuple(out.shape[1:]))
        res = vops.yuv420_to_clip(buf, offs, F, w, h, stride, pl, out_w, out_h, crop=crop,
                                  dtype=dtype, out=out, matrix=matrix, filter=filter)
        return res.view(frames, out_h, out_w, res.shape[-1])
    return run


@functools.lru_cache(maxsize=None)
def reference(name):
    """One case's planes and oracle, computed once: ``(y, u, v, ref, d, tol)``."""
    _, _, matrix, w, h, ow, oh, crop, _ = aa.case(name)
    y, u, v = aa.case_planes(name)
    ref, _, d, tol = aa.tolerance_aa(y, u, v, ow, oh, crop, matrix)
    assert tol <= orc.TOL_CEILING, (name, tol)
    for a in (y, u, v, ref):
        a.setflags(write=False)
    return y, u, v, ref, d, tol


def check_against_oracle(got, ref, d, tol, device, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape[:3] + (4,), got.shape
    err = float(np.abs(to_np(got)[..., :3] - ref).max())
    print("%s on %s: d = %.3g, tolerance = %.3g, max |op - oracle| = %.3g"
          % (what, device.type, d, tol, err))
    assert err <= tol, (what, err, tol)
    assert torch.all(got[..., 3] == 0)


def check_bf16_is_rne(run, shape3, device, what):
    """bf16 is the fp32 result rounded to nearest even, bit for bit; the padding
    channels are zero; nothing is written past the clips of an ``out=`` buffer."""
    f32 = run(torch.float32)
    n = int(np.prod(shape3))
    raw = torch.full(((n * 8 + 64) * 2,), 0xA5, dtype=torch.uint8, device=device)
    flat = raw.view(torch.bfloat16)
    got = run(torch.bfloat16, out=flat[:n * 8].view(shape3 + (8,)))
    sync(device)
    assert got.data_ptr() == flat.data_ptr() and got.dtype == torch.bfloat16
    assert torch.all(raw[n * 8 * 2:] == 0xA5), what + ": bytes past the clips changed"
    assert torch.all(got[..., 3:] == 0), what
    want = f32[..., :3].to(torch.bfloat16)
    assert torch.equal(got[..., :3].view(torch.int16), want.view(torch.int16)), what


def check_case(name, device, bf16=False):
    _, layout, matrix, _, _, ow, oh, crop, _ = aa.case(name)
    y, u, v, ref, d, tol = reference(name)
    run = make_runner(layout, matrix, y, u, v, ow, oh, crop, device)
    if bf16:
        check_bf16_is_rne(run, ref.shape[:3], device, name)
        return
    got = run(torch.float32)
    sync(device)
    check_against_oracle(got, ref, d, tol, device, name)
    if name in aa.UP_ONLY:
        # scale <= 1: the bilinear op computes the same function; each is within its
        # own tolerance of its oracle and the two oracles agree to 1e-12
        _, _, d2, tol2 = orc.tolerance(y, u, v, ow, oh, crop, matrix)
        bil = make_runner(layout, matrix, y, u, v, ow, oh, crop, device, filter="bilinear")(
            torch.float32)
        sync(device)
        err = float((got - bil).abs().max())
        print("%s on %s: |antialias - bilinear| = %.3g, bound %.3g + %.3g"
              % (name, device.type, err, tol, tol2))
        assert err <= tol + tol2, (name, err)


def check_two_clips(device):
    """2 clips x 3 frames of 46x34 at non-monotonic offsets (the second clip
    first in the buffer, a gap between them)."""
    y, u, v = orc.noise_planes(46, 34, 6, 6021)
    ref, _, d, tol = aa.tolerance_aa(y, u, v, 16, 12, (3.5, 1.25, 40, 30), "bt601")
    assert tol <= orc.TOL_CEILING
    data, stride, pl = orc.pack_i420(y, u, v)
    buf = np.full(7 * stride + 11, 0xEE, dtype=np.uint8)
    offs = [4 * stride + 11, 3]
    for c, o in enumerate(offs):
        buf[o:o + 3 * stride] = data[c * 3 * stride:(c + 1) * 3 * stride]
    got = vops.yuv420_to_clip(torch.from_numpy(buf).to(device), offs, 3, 46, 34, stride, pl, 16,
                              12, crop=(3.5, 1.25, 40, 30), filter="antialias")
    sync(device)
    assert tuple(got.shape) == (2, 3, 12, 16, 4)
    check_against_oracle(got.view(6, 12, 16, 4), ref, d, tol, device, "2 clips x 3 frames")


def check_table(matrix, device, n=33):
    """``n`` one-frame 8x6 clips -> 4x3 at shuffled offsets, equal to two launches
    of fewer clips bit for bit. On the GPU, 65 clips are past the 64 rows of the
    kernel-argument tables: the device tables."""
    y, u, v, data, offs, fb, pl = orc.table_case(matrix, n)
    ref, _, d, tol = aa.tolerance_aa(y, u, v, 4, 3, None, matrix)
    assert tol <= orc.TOL_CEILING
    buf = torch.from_numpy(data).to(device)

    def run(o, dtype):
        return vops.yuv420_to_clip(buf, o, 1, 8, 6, fb, pl, 4, 3, dtype=dtype, matrix=matrix,
                                   filter="antialias")
    got = run(offs, torch.float32)
    sync(device)
    assert tuple(got.shape) == (n, 1, 3, 4, 4)
    check_against_oracle(got.view(n, 3, 4, 4), ref, d, tol, device, "offset table " + matrix)
    for dtype in (torch.float32, torch.bfloat16):
        whole = run(offs, dtype)
        parts = torch.cat([run(offs[:20], dtype), run(offs[20:], dtype)])
        sync(device)
        assert torch.equal(whole.view(torch.uint8), parts.view(torch.uint8)), dtype


def check_jpeg_surface(device):
    """45x33 inside a 3x3-MCU JPEG surface (strides 48 / 24): the result is the
    oracle's on the true samples, and bit for bit the same whatever the stride
    and MCU padding hold."""
    y, u, v = orc.noise_planes(45, 33, 2, 4533, "jfif")
    ref, _, d, tol = aa.tolerance_aa(y, u, v, 16, 12, None, "jfif")
    assert tol <= orc.TOL_CEILING
    pl = vops.jpeg_surface_planes(3, 3)
    assert (pl.y_stride, pl.u_stride, pl.v_stride) == (48, 24, 24)
    outs = []
    for fill in (0xEE, 0x11):
        data, stride = aa.pack_jpeg_surface(y, u, v, 3, 3, fill)
        got = vops.yuv420_to_clip(torch.from_numpy(data).to(device), [0], 2, 45, 33, stride, pl,
                                  16, 12, matrix="jfif", filter="antialias")
        sync(device)
        outs.append(got)
    check_against_oracle(outs[0].view(2, 12, 16, 4), ref, d, tol, device, "jpeg surface")
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8))


@functools.lru_cache(maxsize=None)
def stripe_reference():
    y, u, v = aa.stripe_planes()
    ref, _, d, tol = aa.tolerance_aa(y, u, v, 112, 112, None, "jfif")
    assert tol <= orc.TOL_CEILING
    bil, _ = orc.clip_oracle(y, u, v, 112, 112, None, "jfif")
    return y, u, v, ref, d, tol, aa.r_spread(ref), aa.r_spread(bil)


def check_stripes(device):
    """One-pixel black / white columns, 340x256 -> 112x112: the area average is
    nearly flat; two taps give moire over almost the whole range."""
    y, u, v, ref, d, tol, spread_aa, spread_bil = stripe_reference()
    assert spread_aa <= 40.0, spread_aa                       # measured 26.2
    assert spread_bil >= 200.0, spread_bil                    # measured 245.8
    got = make_runner("i420", "jfif", y, u, v, 112, 112, None, device)(torch.float32)
    sync(device)
    check_against_oracle(got, ref, d, tol, device, "stripes")
    spread = aa.r_spread(to_np(got))
    print("stripes on %s: R spread oracle %.2f (bilinear oracle %.2f), op %.2f levels"
          % (device.type, spread_aa, spread_bil, spread))
    # the spread within tol (normalised, as levels of R) of the oracle's: tighter than
    # what two extremes each within tol would allow
    assert abs(spread - spread_aa) <= tol / orc.NORM_PER_LEVEL[0], (spread, spread_aa)


# -- the tests: the CPU mirror ------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", [c[0] for c in aa.AA_CASES])
def test_mirror_against_oracle(name, bf16):
    check_case(name, CPU, bf16)


def test_mirror_two_clips_at_non_monotonic_offsets():
    check_two_clips(CPU)


@pytest.mark.parametrize("matrix", ["bt601", "jfif"])
def test_mirror_33_clips_at_shuffled_offsets(matrix):
    check_table(matrix, CPU)


def test_mirror_ignores_the_padding_of_a_jpeg_surface():
    check_jpeg_surface(CPU)


def test_mirror_stripes():
    check_stripes(CPU)


def test_default_filter_is_bilinear():
    y, u, v = orc.noise_planes(46, 34, 3, 77)
    a = make_runner("i420", "bt601", y, u, v, 16, 12, None, CPU, filter="bilinear")
    data, stride, pl = orc.pack_i420(y, u, v)
    for dtype in (torch.float32, torch.bfloat16):
        b = vops.yuv420_to_clip(torch.from_numpy(data), [0], 3, 46, 34, stride, pl, 16, 12,
                                dtype=dtype)
        assert torch.equal(a(dtype).view(torch.uint8).reshape(-1), b.view(torch.uint8).reshape(-1))
    assert FILTERS == ("bilinear", "antialias")


def check_refusals(device):
    y, u, v = orc.noise_planes(46, 34, 1, 5)
    data, stride, pl = orc.pack_i420(y, u, v)
    buf = torch.from_numpy(data).to(device)
    with pytest.raises(ValueError, match="inside"):
        vops.yuv420_to_clip(buf, [0], 1, 46, 34, stride, pl, 16, 12, crop=(-2, -1, 50, 37),
                            filter="antialias")
    for box in ((0, 0, 46.5, 34), (0, 0.5, 46, 34), (3, 2, 0, 10)):
        with pytest.raises(ValueError, match="inside"):
            vops.yuv420_to_clip(buf, [0], 1, 46, 34, stride, pl, 16, 12, crop=box,
                                filter="antialias")
    # the bilinear filter still takes the box (edge replication)
    vops.yuv420_to_clip(buf, [0], 1, 46, 34, stride, pl, 16, 12, crop=(-2, -1, 50, 37))
    with pytest.raises(ValueError, match="bilinear.*antialias"):
        vops.yuv420_to_clip(buf, [0], 1, 46, 34, stride, pl, 16, 12, filter="bicubic")
    for cls in (Y4mDecoder, MjpegDecoder):
        with pytest.raises(ValueError, match="bilinear.*antialias"):
            cls(device, filter="lanczos")
    sync(device)


def test_refusals():
    check_refusals(CPU)


@pytest.mark.parametrize("kind", ["y4m", "mjpeg"])
def test_antialias_configs_load(kind):
    """Each config is its parent plus the one key."""
    base = json.load(open(os.path.join(ROOT, "configs", "r2p1d-whole-%s.json" % kind)))
    path = os.path.join(ROOT, "configs", "r2p1d-whole-%s-antialias.json" % kind)
    cfg = json.load(open(path))
    assert cfg["pipeline"][0].pop("decoder_args") == {"filter": "antialias"}
    assert cfg == base
    spec = load_pipeline(path)
    assert spec.steps[0].kwargs["decoder"] == kind
    assert spec.steps[0].kwargs["decoder_args"] == {"filter": "antialias"}
    dec = make_decoder(kind, CPU, decoder_args=spec.steps[0].kwargs["decoder_args"])
    assert dec.filter == "antialias"
    assert make_decoder(kind, CPU).filter == "bilinear"


# -- MjpegDecoder against PIL's resized RGB ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pil_target(name):
    """(PIL's golden RGB resized per channel to (w // 3, h // 3) with PIL's mode
    ``F`` triangle filter [2, oh, ow, 3]; the maximum distance from it of the
    reference path: decode_reference's planes -> clip_oracle_aa, JFIF, fp64)."""
    W, H, _ = GOLDEN_STREAMS[name]
    ow, oh = W // 3, H // 3
    rgb = np.load(os.path.join(GOLDEN, name + "_rgb.npy"))
    assert rgb.shape == (2, H, W, 3) and rgb.dtype == np.uint8
    want = np.stack([np.stack([pil_resize(rgb[i, :, :, c], ow, oh, (0, 0, W, H))
                               for c in range(3)], axis=-1) for i in range(2)])
    path = os.path.join(GOLDEN, name + ".mjpeg")
    data = np.fromfile(path, dtype=np.uint8)
    idx = mjpeg.read_index(path)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    worst = 0.0
    for i in range(2):
        py, pu, pv = mjpeg.decode_reference(frame_bytes(data, idx, i))["planes_u8"]
        _, ref = aa.clip_oracle_aa(np.asarray(py)[None, :H, :W], np.asarray(pu)[None, :ch, :cw],
                                   np.asarray(pv)[None, :ch, :cw], ow, oh, None, "jfif")
        worst = max(worst, float(np.abs(np.clip(ref[0], 0, 255) - want[i]).max()))
    want.setflags(write=False)
    return want, worst


def check_pil_resized_rgb(name, device, **decoder_args):
    """The decoder may exceed the reference path's own maximum distance from
    PIL's target by ``PIL_DECODER_MARGIN``. Returns (reference, decoder) maxima."""
    W, H, _ = GOLDEN_STREAMS[name]
    want, worst = pil_target(name)
    dec = MjpegDecoder(device, clip_length=2, height=H // 3, width=W // 3, dtype=torch.float32,
                       crop="full", filter="antialias", **decoder_args)
    vid, n = dec.probe(os.path.join(GOLDEN, name + ".mjpeg"))
    assert n == 2
    got = dec.decode(vid, [0])
    dec.drain()
    sync(device)
    assert tuple(got.shape) == (1, 2, H // 3, W // 3, 4)
    err = float(np.abs(orc.denormalise(to_np(got)[0]) - want).max())
    print("%s %dx%d -> %dx%d on %s %s: |reference path - PIL| max %.4f, |decoder - PIL| max "
          "%.4f levels" % (name, W, H, W // 3, H // 3, device.type, decoder_args, worst, err))
    assert err <= worst + PIL_DECODER_MARGIN, (name, err, worst)
    return worst, err


def test_cpu_decoder_against_pils_resized_rgb():
    lines = []
    for name in sorted(GOLDEN_STREAMS):
        worst, err = check_pil_resized_rgb(name, CPU)
        lines.append("%s: reference path %.4f, MjpegDecoder(cpu) %.4f" % (name, worst, err))
    print("\n".join(lines))       # the figures recorded in profiles/clip_antialias.txt
