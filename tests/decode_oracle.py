"""An independent reference for the decode-side clip kernels (``nv12_clip_kernel``,
``yuv420_clip_kernel``) and their torch mirrors: numpy, fp64, written from the
definition of the operation and in a different shape from the kernels.

A helper module for ``test_decode_oracle_cpu.py`` and
``test_gpu_decode_oracle.py``: it holds no test. From ``rnb_amd/ops/video.py``
it takes the Kinetics constants and the ``YuvPlanes`` tuple and nothing else:
no sampler, no mirror.

The operation. A 4:2:0 frame (Y of w x h, Cb and Cr at half resolution) is
resampled to out_w x out_h from the box ``crop = (x, y, w, h)`` in luma
pixels, bilinear with align_corners = false and edge replication, converted to
RGB, clamped to [0, 255] and normalised, ``(v / 255 - mean) / std``.

* Resampling is a separable matrix product, ``My @ P @ Mx.T``. Along one axis
  output ``o`` looks at source coordinate ``s_o = start + (o + 0.5) size / n_out
  - 0.5`` of the edge-replicated plane, whose sample ``j`` (any integer) is
  sample ``clip(j, 0, n_src - 1)``; its weight is the hat function
  ``max(0, 1 - |s_o - j|)``. No floor, no pair of taps, no clamp of ``s_o``.

* Chroma siting. Chroma sample ``j`` sits at luma coordinate ``2 j + 0.5``: the
  centre of its 2 x 2 luma block, the JPEG / MPEG-1 siting, in both directions.
  The luma box ``(x, y, w, h)`` is therefore the chroma box ``(x / 2, y / 2,
  w / 2, h / 2)`` on a plane of ``w // 2 x h // 2`` samples (BT.601 path, even
  sizes) or ``ceil(w / 2) x ceil(h / 2)`` (JFIF path, any size). That is what
  the kernels implement. A YUV4MPEG2 file tagged ``C420mpeg2`` (chroma
  co-sited with the left luma column) is read with the same centre siting;
  that is documented here and not changed.

* Colour. BT.601 video range: ``Y' = 1.164 (Y - 16)``, ``R = Y' + 1.596 Cr'``,
  ``G = Y' - 0.392 Cb' - 0.813 Cr'``, ``B = Y' + 2.017 Cb'`` with ``Cb' = Cb -
  128``. JFIF full range: ``R = Y + 1.402 Cr'``, ``G = Y - 0.344136 Cb' -
  0.714136 Cr'``, ``B = Y + 1.772 Cb'``.

The forward transforms (RGB -> YCbCr) are the standards' own coefficients and
serve the anchor-colour test, the one check of the matrix constants against
numbers this project did not write.

``dtype=np.float32`` evaluates the same expressions with every array and
scalar in fp32; the distance between the two evaluations is what the tests
derive their tolerance from (``tolerance``)."""
import numpy as np

from rnb_amd.ops.video import KINETICS_MEAN, KINETICS_STD, YuvPlanes

TOL_FLOOR = 4e-6          # a few fp32 ulps of a normalised value of magnitude ~2.6
TOL_CEILING = 1e-3        # 0.06 of an 8-bit level; one matrix coefficient off by 0.001 is ~2e-3
NORM_PER_LEVEL = [1.0 / (255.0 * s) for s in KINETICS_STD]


# -- resampling ---------------------------------------------------------------------
def resample_matrix(n_src, n_out, start, size, dtype=np.float64):
    """M [n_out, n_src]: hat-function weights of the edge-replicated samples."""
    t = dtype
    o = np.arange(n_out).astype(t)
    s = t(start) + (o + t(0.5)) * (t(size) / t(n_out)) - t(0.5)
    lo = int(np.floor(float(s.min()))) - 1
    hi = int(np.ceil(float(s.max()))) + 1
    M = np.zeros((n_out, n_src), dtype=t)
    for j in range(lo, hi + 1):
        M[:, min(max(j, 0), n_src - 1)] += np.maximum(t(0), t(1) - np.abs(s - t(j)))
    return M


def source_coords(n_out, start, size):
    """fp64 source coordinate of every output sample along one axis."""
    return start + (np.arange(n_out, dtype=np.float64) + 0.5) * (size / n_out) - 0.5


def resample(plane, out_w, out_h, box, dtype=np.float64):
    """plane [F, h, w] -> [F, out_h, out_w] from ``box`` = (x, y, w, h)."""
    _, h, w = plane.shape
    Mx = resample_matrix(w, out_w, box[0], box[2], dtype)
    My = resample_matrix(h, out_h, box[1], box[3], dtype)
    return np.matmul(np.matmul(My, plane.astype(dtype)), Mx.T)


# -- colour --------------------------------------------------------------------------
def to_rgb(y, cb, cr, matrix, dtype=np.float64):
    """Unclamped RGB [..., 3] of sampled Y, Cb, Cr."""
    t = dtype
    cb, cr = cb - t(128), cr - t(128)
    if matrix == "jfif":
        rgb = (y + t(1.402) * cr, y - t(0.344136) * cb - t(0.714136) * cr, y + t(1.772) * cb)
    elif matrix == "bt601":
        yy = t(1.164) * (y - t(16))
        rgb = (yy + t(1.596) * cr, yy - t(0.392) * cb - t(0.813) * cr, yy + t(2.017) * cb)
    else:
        raise ValueError(matrix)
    return np.stack(rgb, axis=-1)


def normalise(rgb, dtype=np.float64):
    t = dtype
    mean = np.array(KINETICS_MEAN).astype(t)
    std = np.array(KINETICS_STD).astype(t)
    return (np.clip(rgb, t(0), t(255)) / t(255) - mean) / std


def denormalise(x):
    """Normalised [..., >= 3] -> 8-bit levels [..., 3], fp64."""
    x = np.asarray(x, dtype=np.float64)[..., :3]
    return (x * np.array(KINETICS_STD) + np.array(KINETICS_MEAN)) * 255.0


def clip_oracle(y, u, v, out_w, out_h, crop=None, matrix="bt601", dtype=np.float64):
    """uint8 planes Y [F, h, w], U, V [F, ch, cw] -> (normalised [F, out_h,
    out_w, 3], unclamped RGB of the same shape), both in ``dtype``."""
    F, h, w = y.shape
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if matrix == "jfif" else (w // 2, h // 2)
    assert u.shape == (F, ch, cw) and v.shape == (F, ch, cw), (u.shape, (F, ch, cw))
    box = tuple(float(c) for c in (crop or (0, 0, w, h)))
    cbox = tuple(c / 2.0 for c in box)
    rgb = to_rgb(resample(y, out_w, out_h, box, dtype), resample(u, out_w, out_h, cbox, dtype),
                 resample(v, out_w, out_h, cbox, dtype), matrix, dtype)
    return normalise(rgb, dtype), rgb


def tolerance(y, u, v, out_w, out_h, crop, matrix):
    """The fp32 rule: ``(ref64, rgb64, d, tol)`` with ``d = max |oracle in fp32 -
    oracle in fp64|`` and ``tol = max(4 d, TOL_FLOOR)``. The factor 4 covers
    another operation order and FMA contraction in the code under test."""
    ref, rgb = clip_oracle(y, u, v, out_w, out_h, crop, matrix)
    r32, _ = clip_oracle(y, u, v, out_w, out_h, crop, matrix, np.float32)
    assert r32.dtype == np.float32
    d = float(np.abs(r32.astype(np.float64) - ref).max())
    return ref, rgb, d, max(4.0 * d, TOL_FLOOR)


# -- forward transforms, from the standards ---------------------------------------------
def rgb_to_bt601(rgb):
    """8-bit RGB [..., 3] -> BT.601 video-range Y, Cb, Cr, rounded to uint8."""
    p = np.asarray(rgb, dtype=np.float64) / 255.0
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    ycc = np.stack([16.0 + 65.481 * r + 128.553 * g + 24.966 * b,
                    128.0 - 37.797 * r - 74.203 * g + 112.0 * b,
                    128.0 + 112.0 * r - 93.786 * g - 18.214 * b], axis=-1)
    return np.clip(np.rint(ycc), 0, 255).astype(np.uint8)


def rgb_to_jfif(rgb):
    """8-bit RGB [..., 3] -> full-range JFIF Y, Cb, Cr, rounded to uint8."""
    p = np.asarray(rgb, dtype=np.float64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    ycc = np.stack([0.299 * r + 0.587 * g + 0.114 * b,
                    128.0 - 0.168736 * r - 0.331264 * g + 0.5 * b,
                    128.0 + 0.5 * r - 0.418688 * g - 0.081312 * b], axis=-1)
    return np.clip(np.rint(ycc), 0, 255).astype(np.uint8)


FORWARD = {"bt601": rgb_to_bt601, "jfif": rgb_to_jfif}


# -- buffer packers ----------------------------------------------------------------------
def pack_i420(y, u, v, header=6):
    """Planar frames, each behind ``header`` bytes -> (flat uint8 buffer, frame
    stride, YuvPlanes). The chroma planes are as wide as they are given."""
    F, h, w = y.shape
    _, ch, cw = u.shape
    head = np.frombuffer((b"FRAME\n" * header)[:header], dtype=np.uint8)
    buf = np.concatenate([np.concatenate([head, y[f].reshape(-1), u[f].reshape(-1),
                                          v[f].reshape(-1)]) for f in range(F)])
    stride = header + w * h + 2 * cw * ch
    pl = YuvPlanes(header, header + w * h, header + w * h + cw * ch, w, cw, cw, 1)
    return buf, stride, pl


def pack_nv12(y, u, v, header=7):
    """Semi-planar frames (Y, then interleaved UV rows), each behind ``header``
    bytes -> (flat uint8 buffer, frame stride, YuvPlanes)."""
    F, h, w = y.shape
    _, ch, cw = u.shape
    head = np.full(header, 0x5A, dtype=np.uint8)
    uv = np.stack([u, v], axis=-1)                                  # [F, ch, cw, 2]
    buf = np.concatenate([np.concatenate([head, y[f].reshape(-1), uv[f].reshape(-1)])
                          for f in range(F)])
    stride = header + w * h + 2 * cw * ch
    pl = YuvPlanes(header, header + w * h, header + w * h + 1, w, 2 * cw, 2 * cw, 2)
    return buf, stride, pl


def pack_nv12_surface(y, u, v):
    """Decoder surfaces for ``nv12_to_clip``: uint8 [F, h * 3 / 2, w]."""
    F, h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0 and u.shape == (F, h // 2, w // 2)
    uv = np.stack([u, v], axis=-1).reshape(F, h // 2, w)
    return np.ascontiguousarray(np.concatenate([y, uv], axis=1))


PACKERS = {"i420": pack_i420, "nv12": pack_nv12}


# -- inputs --------------------------------------------------------------------------------
def noise_planes(w, h, frames, seed, matrix="bt601"):
    """Seeded uint8 noise: Y [F, h, w], U, V at the matrix's chroma size."""
    rng = np.random.default_rng(seed)
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if matrix == "jfif" else (w // 2, h // 2)
    return (rng.integers(0, 256, (frames, h, w), dtype=np.uint8),
            rng.integers(0, 256, (frames, ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (frames, ch, cw), dtype=np.uint8))


RAMP_W, RAMP_H = 48, 32
# (out_w, out_h, crop) of the two ramp resizes
RAMP_RESIZES = [(24, 16, (4, 4, 36, 24)), (31, 19, None)]


def luma_ramp_planes(frames=3):
    """Y = 20 + 3 x + 2 y (inside [16, 235]), U = V = 128."""
    yy, xx = np.mgrid[0:RAMP_H, 0:RAMP_W]
    y = np.broadcast_to((20 + 3 * xx + 2 * yy).astype(np.uint8), (frames, RAMP_H, RAMP_W))
    c = np.full((frames, RAMP_H // 2, RAMP_W // 2), 128, dtype=np.uint8)
    return np.ascontiguousarray(y), c, c.copy()


def chroma_ramp_planes(frames=3):
    """Y = 128, U = 60 + 4 j across the chroma plane, V = 200 - 6 i down it."""
    ci, cj = np.mgrid[0:RAMP_H // 2, 0:RAMP_W // 2]
    shape = (frames, RAMP_H // 2, RAMP_W // 2)
    return (np.full((frames, RAMP_H, RAMP_W), 128, dtype=np.uint8),
            np.ascontiguousarray(np.broadcast_to((60 + 4 * cj).astype(np.uint8), shape)),
            np.ascontiguousarray(np.broadcast_to((200 - 6 * ci).astype(np.uint8), shape)))


def ramp_expectations(out_w, out_h, crop, matrix):
    """What the two ramps must give, from the mapping alone (no resampling code):
    ``(luma [out_h, out_w, 3], luma_mask, chroma [out_h, out_w, 3], b_mask,
    r_mask)`` in normalised units. ``luma``: R = G = B of the luma ramp, valid
    where the source coordinate lies inside the luma plane. ``chroma``: B in
    channel 2 and R in channel 0 of the chroma ramp (channel 1 is not
    checked), valid where the chroma coordinate lies inside the chroma plane
    and the value is not clamped: with BT.601, B = 130.368 + 2.017 (Cb - 128)
    is below 0 for Cb < 63.4, the plane's leftmost 0.84 sample."""
    box = tuple(float(c) for c in (crop or (0, 0, RAMP_W, RAMP_H)))
    sx = source_coords(out_w, box[0], box[2])[None, :]
    sy = source_coords(out_h, box[1], box[3])[:, None]
    inside = (sx >= 0) & (sx <= RAMP_W - 1) & (sy >= 0) & (sy <= RAMP_H - 1)
    yv = 20.0 + 3.0 * sx + 2.0 * sy
    grey = yv if matrix == "jfif" else 1.164 * (yv - 16.0)
    luma = normalise(np.stack([grey, grey, grey], axis=-1))
    cx, cy = (sx + 0.5) / 2.0 - 0.5, (sy + 0.5) / 2.0 - 0.5
    cin = (cx >= 0) & (cx <= RAMP_W // 2 - 1) & (cy >= 0) & (cy <= RAMP_H // 2 - 1)
    cb = 60.0 + 4.0 * cx + 0.0 * cy
    cr = 200.0 - 6.0 * cy + 0.0 * cx
    y0 = 128.0 if matrix == "jfif" else 1.164 * (128.0 - 16.0)
    kb, kr = (1.772, 1.402) if matrix == "jfif" else (2.017, 1.596)
    b = y0 + kb * (cb - 128.0)
    r = y0 + kr * (cr - 128.0)
    chroma = normalise(np.stack([r, np.zeros_like(r), b], axis=-1))
    return (luma, inside, chroma, cin & (b >= 1.0) & (b <= 254.0),
            cin & (r >= 1.0) & (r <= 254.0))


def anchor_grid():
    """The 6 x 6 x 6 RGB grid {0, 51, ..., 255}^3: uint8 [216, 3]."""
    g = np.arange(6, dtype=np.int64) * 51
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(216, 3).astype(np.uint8)


def anchor_planes(matrix):
    """(grid [216, 3], triples [216, 3], Y [216, 4, 4], U, V [216, 2, 2]):
    every grid colour through the standard's forward transform, rounded, as a
    constant 4 x 4 frame."""
    grid = anchor_grid()
    ycc = FORWARD[matrix](grid)
    ones = np.ones((216, 4, 4), dtype=np.uint8)
    return (grid, ycc, ones * ycc[:, 0, None, None], ones[:, :2, :2] * ycc[:, 1, None, None],
            ones[:, :2, :2] * ycc[:, 2, None, None])


def anchor_bound(matrix):
    """(bound in levels, the oracle's own maximum): the fp64 inverse matrix on
    the rounded triples against the grid, + 0.05 level."""
    grid, ycc, _, _, _ = anchor_planes(matrix)
    t = ycc.astype(np.float64)
    rgb = np.clip(to_rgb(t[:, 0], t[:, 1], t[:, 2], matrix), 0, 255)
    worst = float(np.abs(rgb - grid).max())
    return worst + 0.05, worst


# -- case tables ---------------------------------------------------------------------------
# (id, src_w, src_h, out_w, out_h, crop, frames)
NV12_CASES = [
    ("46x34_full", 46, 34, 24, 16, None, 3),               # non-square output, npix % 256 != 0
    ("46x34_dyadic", 46, 34, 24, 16, (3, 2, 36, 28), 3),   # scales 1.5 / 1.75
    ("46x34_outside", 46, 34, 24, 16, (-2, -1, 50, 37), 3),   # all four edge clamps
    ("2x2_up", 2, 2, 5, 3, None, 3),                       # 1 x 1 chroma plane, every tap clamped
    ("6x4_up", 6, 4, 17, 9, None, 3),                      # upscaling, right / bottom x1, y1 clamps
    ("340x256_workload", 340, 256, 112, 112, (20, 8, 256, 240), 1),
]
# (id, layout, matrix, src_w, src_h, out_w, out_h, crop, frames)
YUV420_CASES = [("%s_%s_%s" % (layout, matrix, c[0][6:]), layout, matrix) + c[1:]
                for layout, matrix in (("i420", "bt601"), ("nv12", "bt601"), ("i420", "jfif"))
                for c in NV12_CASES[:3]] + [
    ("i420_jfif_45x33", "i420", "jfif", 45, 33, 24, 16, None, 3),
    ("i420_jfif_1x1", "i420", "jfif", 1, 1, 3, 3, None, 3),
]


def case_seed(name):
    if name == "i420_jfif_1x1":
        # three frames of one sample are nine RGB values: a seed whose nine reach both
        # clamps and leave five unclamped (most seeds miss one of the three conditions)
        return 0
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


def table_case(matrix, n=33, w=8, h=6, slot=77, shift=5):
    """``n`` (33 unless given) one-frame clips of 8 x 6 at distinct, shuffled,
    non-monotonic byte offsets (I420, 72 bytes each in slots of 77 behind 5 bytes):
    ``(y, u, v, buffer, offsets, frame stride, YuvPlanes)``; planes in clip
    order."""
    y, u, v = noise_planes(w, h, n, 4100 + (matrix == "jfif"), matrix)
    fb = w * h + 2 * u.shape[1] * u.shape[2]
    perm = np.random.default_rng(33).permutation(n)
    assert (np.diff(perm) < 0).any() and (np.diff(perm) > 0).any()
    buf = np.full(shift + n * slot, 0xEE, dtype=np.uint8)
    offs = []
    for c in range(n):
        o = shift + int(perm[c]) * slot
        buf[o:o + fb] = np.concatenate([y[c].reshape(-1), u[c].reshape(-1), v[c].reshape(-1)])
        offs.append(o)
    ch, cw = u.shape[1:]
    return y, u, v, buf, offs, fb, YuvPlanes(0, w * h, w * h + cw * ch, w, cw, cw, 1)


def check_clamp_coverage(rgb, what):
    """A noise case reaches both clamps and leaves at least half unclamped."""
    clamped = float(((rgb < 0) | (rgb > 255)).mean())
    assert (rgb < 0).any() and (rgb > 255).any() and clamped <= 0.5, (what, clamped)
    return clamped
