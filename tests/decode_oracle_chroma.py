"""The fp64 clip oracles of ``decode_oracle.py`` (bilinear) and
``decode_oracle_aa.py`` (antialias) for 4:2:2 and 4:4:4 frames.

A helper module for ``test_chroma_cpu.py`` and ``test_gpu_chroma.py``: it holds
no test. Resampling, colour, normalisation and the tolerance rule are those two
modules', imported; nothing here comes from a kernel or a torch mirror.

The one thing added is the chroma geometry. With luma sampling factors
``(Hs, Vs)`` = (2, 2), (2, 1), (1, 1) for ``"420"``, ``"422"``, ``"444"``, chroma
sample ``j`` sits at luma coordinate ``Hs j + (Hs - 1) / 2`` (the centre of the
luma samples it covers; for a factor of 1 that is the luma sample itself). The
luma box ``(x, y, w, h)`` is therefore the chroma box ``(x / Hs, y / Vs, w / Hs,
h / Vs)`` on a plane of ``ceil(w / Hs) x ceil(h / Vs)`` samples (JFIF) or
``w / Hs x h / Vs`` (BT.601; ``w`` even only when Hs = 2, ``h`` even only when
Vs = 2)."""
import numpy as np

import decode_oracle as orc
import decode_oracle_aa as aa

from rnb_amd.ops.video import YuvPlanes

FACTORS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}


def chroma_size(w, h, sampling, matrix):
    hs, vs = FACTORS[sampling]
    if matrix == "jfif":
        return -(-w // hs), -(-h // vs)
    assert w % hs == 0 and h % vs == 0, (w, h, sampling)
    return w // hs, h // vs


def chroma_box(box, sampling):
    hs, vs = FACTORS[sampling]
    return (box[0] / hs, box[1] / vs, box[2] / hs, box[3] / vs)


def clip_oracle(y, u, v, out_w, out_h, crop=None, matrix="bt601", sampling="420",
                filter="bilinear", dtype=np.float64):
    """uint8 planes Y [F, h, w], U, V [F, ch, cw] -> (normalised [F, out_h,
    out_w, 3], unclamped RGB of the same shape), both in ``dtype``."""
    F, h, w = y.shape
    cw, ch = chroma_size(w, h, sampling, matrix)
    assert u.shape == (F, ch, cw) and v.shape == (F, ch, cw), (u.shape, (F, ch, cw))
    box = tuple(float(c) for c in (crop or (0, 0, w, h)))
    cbox = chroma_box(box, sampling)
    if filter == "antialias":
        assert aa.box_inside(box, w, h), box
        res = aa.resample_aa
    else:
        res = orc.resample
    rgb = orc.to_rgb(res(y, out_w, out_h, box, dtype), res(u, out_w, out_h, cbox, dtype),
                     res(v, out_w, out_h, cbox, dtype), matrix, dtype)
    return orc.normalise(rgb, dtype), rgb


def tolerance(y, u, v, out_w, out_h, crop, matrix, sampling, filter="bilinear"):
    """``decode_oracle.tolerance``'s rule: ``(ref64, rgb64, d, tol)`` with ``d =
    max |oracle in fp32 - oracle in fp64|`` and ``tol = max(4 d, TOL_FLOOR)``;
    the callers assert ``tol <= TOL_CEILING``."""
    ref, rgb = clip_oracle(y, u, v, out_w, out_h, crop, matrix, sampling, filter)
    r32, _ = clip_oracle(y, u, v, out_w, out_h, crop, matrix, sampling, filter, np.float32)
    assert r32.dtype == np.float32
    d = float(np.abs(r32.astype(np.float64) - ref).max())
    return ref, rgb, d, max(4.0 * d, orc.TOL_FLOOR)


def noise_planes(w, h, frames, seed, matrix, sampling):
    rng = np.random.default_rng(seed)
    cw, ch = chroma_size(w, h, sampling, matrix)
    return (rng.integers(0, 256, (frames, h, w), dtype=np.uint8),
            rng.integers(0, 256, (frames, ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (frames, ch, cw), dtype=np.uint8))


def pack_planar(y, u, v, header=7):
    """Planar frames (Y, U, V), each behind ``header`` bytes (odd by default, so
    no plane is aligned) -> (flat uint8 buffer, frame stride, YuvPlanes)."""
    return orc.pack_i420(y, u, v, header)


def pack_jpeg_surface(y, u, v, mw, mh, sampling, fill):
    """Planes inside ``jpeg_idct``'s padded surface layout (Y [8 Vs mh, 8 Hs mw],
    then Cb, Cr [8 mh, 8 mw] per frame), every byte outside the true samples
    set to ``fill``: (flat uint8 buffer, frame stride, YuvPlanes)."""
    hs, vs = FACTORS[sampling]
    F, h, w = y.shape
    _, ch, cw = u.shape
    n, ny = mw * mh, hs * vs
    buf = np.full((F, 64 * (ny + 2) * n), fill, dtype=np.uint8)
    ys = buf[:, :64 * ny * n].reshape(F, 8 * vs * mh, 8 * hs * mw)
    us = buf[:, 64 * ny * n:64 * (ny + 1) * n].reshape(F, 8 * mh, 8 * mw)
    vs_ = buf[:, 64 * (ny + 1) * n:].reshape(F, 8 * mh, 8 * mw)
    ys[:, :h, :w] = y
    us[:, :ch, :cw] = u
    vs_[:, :ch, :cw] = v
    pl = YuvPlanes(0, 64 * ny * n, 64 * (ny + 1) * n, 8 * hs * mw, 8 * mw, 8 * mw, 1)
    return buf.reshape(-1), 64 * (ny + 2) * n, pl


# -- the siting ramp -------------------------------------------------------------------------
RAMP_W, RAMP_H = 48, 32


def chroma_ramp_planes(sampling, frames=2):
    """Y = 128, U = 60 + 2 Hs j across the chroma plane, V = 200 - 3 Vs i down it
    (BT.601 sizes): per luma pixel the slopes are 2 and -3 whatever the sampling."""
    hs, vs = FACTORS[sampling]
    cw, ch = RAMP_W // hs, RAMP_H // vs
    ci, cj = np.mgrid[0:ch, 0:cw]
    shape = (frames, ch, cw)
    return (np.full((frames, RAMP_H, RAMP_W), 128, dtype=np.uint8),
            np.ascontiguousarray(np.broadcast_to((60 + 2 * hs * cj).astype(np.uint8), shape)),
            np.ascontiguousarray(np.broadcast_to((200 - 3 * vs * ci).astype(np.uint8), shape)))


def chroma_ramp_expectation(out_w, out_h, crop, matrix, sampling):
    """From the mapping alone: ``(expected [out_h, out_w, 3], b_mask, r_mask)`` in
    normalised units; B (channel 2) follows Cb, R (channel 0) follows Cr. Along
    an axis with factor 1 the chroma coordinate is the luma coordinate; along
    one with factor 2 it is ``(s + 0.5) / 2 - 0.5``."""
    hs, vs = FACTORS[sampling]
    box = tuple(float(c) for c in (crop or (0, 0, RAMP_W, RAMP_H)))
    sx = orc.source_coords(out_w, box[0], box[2])[None, :]
    sy = orc.source_coords(out_h, box[1], box[3])[:, None]
    cx = (sx + 0.5) / 2.0 - 0.5 if hs == 2 else sx
    cy = (sy + 0.5) / 2.0 - 0.5 if vs == 2 else sy
    cin = (cx >= 0) & (cx <= RAMP_W // hs - 1) & (cy >= 0) & (cy <= RAMP_H // vs - 1)
    cb = 60.0 + 2.0 * hs * cx + 0.0 * cy
    cr = 200.0 - 3.0 * vs * cy + 0.0 * cx
    y0 = 128.0 if matrix == "jfif" else 1.164 * (128.0 - 16.0)
    kb, kr = (1.772, 1.402) if matrix == "jfif" else (2.017, 1.596)
    b = y0 + kb * (cb - 128.0)
    r = y0 + kr * (cr - 128.0)
    exp = orc.normalise(np.stack([r, np.zeros_like(r), b], axis=-1))
    return exp, cin & (b >= 1.0) & (b <= 254.0), cin & (r >= 1.0) & (r <= 254.0)


# -- case tables -------------------------------------------------------------------------------
# (id, matrix, filter, src_w, src_h, out_w, out_h, crop, frames); every case runs for "422"
# and "444". 46 x 33 (BT.601) and 45 x 33 (JFIF): non-square, odd where the sampling allows.
def cases(sampling):
    odd_w = 45 if sampling == "444" else 46            # BT.601 needs even w only for Hs = 2
    return [
        ("bt601_bil_full", "bt601", "bilinear", odd_w, 33, 24, 16, None, 2),
        ("bt601_bil_outside", "bt601", "bilinear", odd_w, 33, 24, 16, (-2, -1, 50, 36), 2),
        ("bt601_bil_up", "bt601", "bilinear", 6, 3, 17, 9, None, 2),
        ("jfif_bil_45x33", "jfif", "bilinear", 45, 33, 24, 16, (3, 2, 36, 28), 2),
        ("jfif_bil_1x1", "jfif", "bilinear", 1, 1, 3, 3, None, 2),
        ("bt601_aa_full", "bt601", "antialias", odd_w, 33, 16, 12, None, 2),
        ("jfif_aa_box", "jfif", "antialias", 45, 33, 16, 12, (3.5, 1.25, 40, 30), 2),
        ("jfif_aa_up", "jfif", "antialias", 7, 5, 17, 9, None, 2),
        # wider than one column tile of the antialias kernel (128): two tiles, the second
        # partly filled, and a second row band of one row
        ("bt601_aa_wide", "bt601", "antialias", 410, 13, 200, 9, (2.5, 0.5, 400, 12), 1),
    ]


def case_seed(name, sampling):
    return orc.case_seed(name + sampling)
