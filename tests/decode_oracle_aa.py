"""An independent reference for ``yuv420_to_clip(filter="antialias")``
(``yuv420_clip_aa_kernel`` and its torch mirror): numpy, fp64 or fp32, written
from the definition of the operation and in a different shape from both.

A helper module for ``test_decode_aa_cpu.py`` and ``test_gpu_decode_aa.py``: it
holds no test. Colour, normalisation, packers, inputs and the tolerance rule are
``decode_oracle.py``'s; from ``rnb_amd/ops/video.py`` it takes nothing beyond
what that module already takes.

The operation is ``decode_oracle.py``'s except for the resampling weights. Along
one axis of one plane with ``n_src`` samples, output sample ``o`` of ``n_out``
from the box ``(start, size)``::

    scale = size / n_out          fs = max(scale, 1)
    s_o   = start + (o + 0.5) * scale - 0.5
    w_j   = max(0, 1 - |j - s_o| / fs)      for j = 0 .. n_src - 1 only
    out_o = sum_j w_j p_j / sum_j w_j

The hat is widened by the downscale factor, its support is cut at the plane's
true samples, and the weights are renormalised. The 2-D filter is separable;
each axis has its own ``fs``. A chroma plane is resampled from the chroma box
(luma box / 2) by the same rule applied to that box on that plane. The box must
lie inside the frame: then no row of weights is empty.

``aa_matrix`` walks each output sample's support sample by sample (no
broadcast over the whole plane, no clamp of a weight array), so that it shares
no expression with the mirror's ``_antialias_weights``."""
import math

import numpy as np

import decode_oracle as orc


def aa_matrix(n_src, n_out, start, size, dtype=np.float64):
    """M [n_out, n_src]: renormalised widened-hat weights over the true samples."""
    t = dtype
    scale = t(size) / t(n_out)
    fs = scale if scale > t(1) else t(1)
    M = np.zeros((n_out, n_src), dtype=t)
    for o in range(n_out):
        s = t(start) + (t(o) + t(0.5)) * scale - t(0.5)
        first = max(int(math.floor(float(s - fs))), 0)
        last = min(int(math.ceil(float(s + fs))), n_src - 1)
        total = t(0)
        for j in range(first, last + 1):
            w = t(1) - abs(t(j) - s) / fs
            if w > t(0):
                M[o, j] = w
                total = total + w
        assert total > 0, "empty row of weights: the box leaves the plane"
        M[o, first:last + 1] = M[o, first:last + 1] / total
    return M


def box_inside(box, w, h):
    x, y, bw, bh = box
    return x >= 0 and y >= 0 and bw > 0 and bh > 0 and x + bw <= w and y + bh <= h


def resample_aa(plane, out_w, out_h, box, dtype=np.float64):
    """plane [F, h, w] -> [F, out_h, out_w] from ``box`` = (x, y, w, h)."""
    _, h, w = plane.shape
    Mx = aa_matrix(w, out_w, box[0], box[2], dtype)
    My = aa_matrix(h, out_h, box[1], box[3], dtype)
    return np.matmul(np.matmul(My, plane.astype(dtype)), Mx.T)


def clip_oracle_aa(y, u, v, out_w, out_h, crop=None, matrix="bt601", dtype=np.float64):
    """uint8 planes Y [F, h, w], U, V [F, ch, cw] -> (normalised [F, out_h,
    out_w, 3], unclamped RGB of the same shape), both in ``dtype``."""
    F, h, w = y.shape
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if matrix == "jfif" else (w // 2, h // 2)
    assert u.shape == (F, ch, cw) and v.shape == (F, ch, cw), (u.shape, (F, ch, cw))
    box = tuple(float(c) for c in (crop or (0, 0, w, h)))
    assert box_inside(box, w, h), box
    cbox = tuple(c / 2.0 for c in box)
    rgb = orc.to_rgb(resample_aa(y, out_w, out_h, box, dtype),
                     resample_aa(u, out_w, out_h, cbox, dtype),
                     resample_aa(v, out_w, out_h, cbox, dtype), matrix, dtype)
    return orc.normalise(rgb, dtype), rgb


def tolerance_aa(y, u, v, out_w, out_h, crop, matrix):
    """``decode_oracle.tolerance``'s rule on this oracle: ``(ref64, rgb64, d,
    tol)`` with ``d = max |oracle in fp32 - oracle in fp64|`` and ``tol =
    max(4 d, TOL_FLOOR)``."""
    ref, rgb = clip_oracle_aa(y, u, v, out_w, out_h, crop, matrix)
    r32, _ = clip_oracle_aa(y, u, v, out_w, out_h, crop, matrix, np.float32)
    assert r32.dtype == np.float32
    d = float(np.abs(r32.astype(np.float64) - ref).max())
    return ref, rgb, d, max(4.0 * d, orc.TOL_FLOOR)


# -- the case table ------------------------------------------------------------------------
# (id, layout, matrix, src_w, src_h, out_w, out_h, crop, frames)
AA_CASES = [
    ("i420_bt601_46x34_full", "i420", "bt601", 46, 34, 16, 12, None, 3),   # 2.875 / 2.833
    ("nv12_bt601_46x34_full", "nv12", "bt601", 46, 34, 16, 12, None, 3),
    ("i420_jfif_46x34_full", "i420", "jfif", 46, 34, 16, 12, None, 3),
    ("i420_bt601_46x34_box", "i420", "bt601", 46, 34, 16, 12, (3.5, 1.25, 40, 30), 3),  # 2.5
    ("nv12_bt601_46x34_box", "nv12", "bt601", 46, 34, 16, 12, (3.5, 1.25, 40, 30), 3),
    ("i420_jfif_46x34_box", "i420", "jfif", 46, 34, 16, 12, (3.5, 1.25, 40, 30), 3),
    ("i420_bt601_46x34_down_up", "i420", "bt601", 46, 34, 16, 40, None, 3),   # down in x, up in y
    ("i420_bt601_6x4_up", "i420", "bt601", 6, 4, 17, 9, None, 3),
    ("i420_jfif_1x1_up", "i420", "jfif", 1, 1, 3, 3, None, 3),
    ("i420_jfif_45x33", "i420", "jfif", 45, 33, 16, 12, None, 3),          # rounded-up chroma
    ("i420_jfif_3x3_to_1x1", "i420", "jfif", 3, 3, 1, 1, None, 3),         # one sample, whole frame
    ("i420_bt601_98x62_to_5x3", "i420", "bt601", 98, 62, 5, 3, None, 3),   # 19.6 / 20.7: row chunks
    # wider than one column tile of the kernel (128): two tiles, the second partly filled,
    # and a second row band of one row; fractional box
    ("i420_bt601_410x26_to_200x9", "i420", "bt601", 410, 26, 200, 9, (2.5, 0.5, 400, 25), 2),
    ("i420_bt601_340x256_workload", "i420", "bt601", 340, 256, 112, 112, (42, 0, 256, 256), 1),
]
UP_ONLY = ("i420_bt601_6x4_up", "i420_jfif_1x1_up")     # scale <= 1: also the bilinear kernel's result


def case(name):
    return next(c for c in AA_CASES if c[0] == name)


def case_planes(name):
    _, _, matrix, w, h, _, _, _, frames = case(name)
    return orc.noise_planes(w, h, frames, orc.case_seed(name), matrix)


def stripe_planes(w=340, h=256, matrix="jfif"):
    """One frame: Y = 0 / 255 in alternating columns, U = V = 128."""
    y = np.zeros((1, h, w), dtype=np.uint8)
    y[:, :, 1::2] = 255
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if matrix == "jfif" else (w // 2, h // 2)
    c = np.full((1, ch, cw), 128, dtype=np.uint8)
    return y, c, c.copy()


def r_spread(normalised):
    """max - min of the R channel in 8-bit levels."""
    r = orc.denormalise(normalised)[..., 0]
    return float(r.max() - r.min())


def pack_jpeg_surface(y, u, v, mw, mh, fill):
    """Planes inside ``jpeg_idct``'s padded surface layout (Y [16 mh, 16 mw],
    then Cb, Cr [8 mh, 8 mw] per frame), every byte outside the true samples set
    to ``fill``: (flat uint8 buffer, frame stride)."""
    F, h, w = y.shape
    _, ch, cw = u.shape
    n = mw * mh
    buf = np.full((F, 384 * n), fill, dtype=np.uint8)
    ys = buf[:, :256 * n].reshape(F, 16 * mh, 16 * mw)
    us = buf[:, 256 * n:320 * n].reshape(F, 8 * mh, 8 * mw)
    vs = buf[:, 320 * n:].reshape(F, 8 * mh, 8 * mw)
    ys[:, :h, :w] = y
    us[:, :ch, :cw] = u
    vs[:, :ch, :cw] = v
    return buf.reshape(-1), 384 * n
