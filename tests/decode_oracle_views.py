"""The crop boxes of the short-side resize + window protocol, from its definition.

A helper module for ``test_views_cpu.py`` and ``test_gpu_views.py``: it holds no
test and shares no code with ``rnb_amd/models/r2p1d/decoder.py``.

The protocol. A ``W`` x ``H`` frame is resized, aspect kept, so that its short
side ``m = min(W, H)`` becomes ``S``; then windows of the output size ``ow`` x
``oh`` are cut from the resized frame. Seen from the source frame the resize
factor is ``m / S`` source pixels per resized pixel, so a window covers
``ow m / S`` x ``oh m / S`` source pixels, and what is left over along an axis
(the free length) is the frame's size minus the window's. One window sits in the
middle of both free lengths. Three windows sit at the start, the middle and the
end of the larger free length (x when they are equal) and in the middle of the
other: left / centre / right for a landscape frame, top / centre / bottom for a
portrait one.

Everything here is plain Python floats (fp64); ``inside_f32`` is the antialias
launcher's own acceptance test applied to a box as the kernel receives it."""
import numpy as np


def window(W, H, ow, oh, S):
    """(width, height) of one window in source pixels."""
    short = W if W < H else H
    return ow * short / S, oh * short / S


def fits(W, H, ow, oh, S):
    w, h = window(W, H, ow, oh, S)
    return w <= W and h <= H


def boxes(W, H, ow, oh, S, V):
    """The ``V`` boxes (x, y, w, h), view 0 first; ``None`` if a window is larger
    than the frame."""
    if not fits(W, H, ow, oh, S):
        return None
    w, h = window(W, H, ow, oh, S)
    free = [W - w, H - h]
    mid = [free[0] / 2, free[1] / 2]
    if V == 1:
        return [(mid[0], mid[1], w, h)]
    assert V == 3
    axis = 1 if free[1] > free[0] else 0
    out = []
    for frac in (0.0, 0.5, 1.0):
        pos = list(mid)
        pos[axis] = frac * free[axis]
        out.append((pos[0], pos[1], w, h))
    return out


def axis_of(W, H, ow, oh, S):
    """'x' or 'y': the axis three views are spread along."""
    w, h = window(W, H, ow, oh, S)
    return "y" if H - h > W - w else "x"


def inside_f32(box, W, H):
    """The box rounded to fp32 each number (as a ``float*`` argument carries it)
    passes ``x >= 0, y >= 0, w > 0, h > 0, (double) x + w <= W, (double) y + h <= H``."""
    x, y, w, h = (float(np.float32(c)) for c in box)
    return x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= W and y + h <= H


def is_f32(box):
    return all(float(np.float32(c)) == float(c) for c in box)


def close(box, ref, ulps=2):
    """Every number of ``box`` within ``ulps`` fp32 ulps (at the frame's scale:
    the larger of the number and the box's far edge) of the exact one."""
    for k in range(4):
        scale = max(abs(ref[k]), abs(ref[k % 2] + ref[k % 2 + 2]), 1.0)
        if abs(box[k] - ref[k]) > ulps * float(np.spacing(np.float32(scale))):
            return False
    return True
