"""Loader, head and reduction ops: HIP kernels + bit-exact/fp32 torch mirrors.

GPU tensors dispatch to ``librnb_kernels.so``; CPU tensors run the torch
mirror (the mirrors are what the numerics tests compare the kernels with).
"""
from __future__ import annotations

import itertools
import math
import numbers
import struct
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

# Kinetics-400 normalisation used by R(2+1)D
KINETICS_MEAN = (0.43216, 0.394666, 0.37645)
KINETICS_STD = (0.22803, 0.22145, 0.216989)
IN_CHANNELS_P = 8   # RGB padded to 8 channels (16-byte NDHWC bf16 pixels)
IN_CHANNELS_P_F32 = 4   # RGB padded to 4 channels (16-byte NDHWC fp32 pixels)


def clip_channels(dtype) -> int:
    """Channels per pixel of a clip of ``dtype``: every pixel is 16 bytes."""
    return IN_CHANNELS_P_F32 if dtype == torch.float32 else IN_CHANNELS_P

_M32 = 0xFFFFFFFF


def _pixel_hash_torch(vid: torch.Tensor, frame: torch.Tensor, pix: torch.Tensor,
                      c: torch.Tensor) -> torch.Tensor:
    h = (vid * 0x9E3779B1 + frame * 0x85EBCA77 + pix * 0xC2B2AE3D + c * 0x27D4EB2F) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & _M32
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & _M32
    h = h ^ (h >> 15)
    return (h >> 24).to(torch.uint8)


def clipgen_u8(vids: torch.Tensor, starts: torch.Tensor, F: int, H: int, W: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Synthetic decoded clips: uint8 [n, F, H, W, 3], deterministic."""
    n = int(vids.numel())
    if vids.is_cuda:
        from .native import kernels
        if out is None:
            out = torch.empty((n, F, H, W, 3), dtype=torch.uint8, device=vids.device)
        vids = vids.to(torch.int32).contiguous()
        starts = starts.to(torch.int32).contiguous()
        kernels().clipgen_u8(out.data_ptr(), vids.data_ptr(), starts.data_ptr(), n, F, H, W,
                             torch.cuda.current_stream(vids.device).cuda_stream)
        return out
    v = vids.to(torch.int64).view(n, 1, 1, 1, 1)
    f = starts.to(torch.int64).view(n, 1, 1, 1, 1) + torch.arange(F).view(1, F, 1, 1, 1)
    pix = torch.arange(H * W, dtype=torch.int64).view(1, 1, H, W, 1)
    c = torch.arange(3, dtype=torch.int64).view(1, 1, 1, 1, 3)
    res = _pixel_hash_torch(v, f, pix, c)
    if out is not None:
        out.copy_(res)
        return out
    return res.contiguous()


def _clip_frame_offsets(F: int, step) -> torch.Tensor:
    """``(f * p) // q`` for the F frames of a clip (``sampler.clip_frames``)."""
    p, q = int(step[0]), int(step[1])
    if p < 1 or q < 1:
        raise ValueError("step (p, q) must be positive integers, got %r" % (step,))
    return torch.tensor([(f * p) // q for f in range(F)], dtype=torch.int64)


def clipgen_video(vid: int, starts, F: int, H: int, W: int, device,
                  out: Optional[torch.Tensor] = None, step=(1, 1)) -> torch.Tensor:
    """One video's synthetic clips (uint8 [n, F, H, W, 3]); the start frames
    travel as kernel arguments, so nothing is uploaded and the host never
    waits (the per-video form of ``clipgen_u8``; same pixels). ``step`` =
    ``(p, q)``: frame ``f`` of a clip is frame ``start + (f * p) // q`` of the
    video (``sampler.clip_frames``)."""
    n = len(starts)
    stepped = tuple(step) != (1, 1)
    if device.type == "cuda":
        from .native import kernels
        if out is None:
            out = torch.empty((n, F, H, W, 3), dtype=torch.uint8, device=device)
        if stepped:          # the device-array form has no step: 32 clips per launch
            stream = torch.cuda.current_stream(device).cuda_stream
            for i in range(0, n, 32):
                kernels().clipgen_video_step(out[i:].data_ptr(), vid, list(starts[i:i + 32]),
                                             F, H, W, step, stream)
            return out
        if n > 32:
            return clipgen_u8(torch.full((n,), vid, dtype=torch.int32, device=device),
                              torch.as_tensor(list(starts), dtype=torch.int32).to(device),
                              F, H, W, out=out)
        kernels().clipgen_video(out.data_ptr(), vid, list(starts), F, H, W,
                                torch.cuda.current_stream(device).cuda_stream)
        return out
    if stepped:
        # every frame as a one-frame clip at its own source frame: same pixels
        fr = (torch.as_tensor(list(starts), dtype=torch.int64).view(n, 1)
              + _clip_frame_offsets(F, step).view(1, F)).reshape(-1)
        res = clipgen_u8(torch.full((n * F,), vid, dtype=torch.int32), fr, 1, H, W)
        res = res.view(n, F, H, W, 3)
        if out is not None:
            out.copy_(res)
            return out
        return res
    return clipgen_u8(torch.full((n,), vid, dtype=torch.int32),
                      torch.as_tensor(list(starts), dtype=torch.int32), F, H, W, out=out)


# ---------------------------------------------------------------------------
# NV12 decoder surfaces (VCN / NVDEC output format) -> normalised clips
# ---------------------------------------------------------------------------
SOURCE_W, SOURCE_H = 340, 256      # Kinetics-400 videos as usually stored


def nv12_frame_bytes(W: int, H: int) -> int:
    return W * H * 3 // 2


def nv12gen(vids, starts, F: int, H: int, W: int, device,
            out: Optional[torch.Tensor] = None, step=(1, 1)) -> torch.Tensor:
    """Synthetic decoder surfaces: uint8 [n*F, H*3/2, W] NV12 frames (Y rows,
    then interleaved UV rows), deterministic per (video, frame). ``vids`` may
    be one id (start frames then go in kernel arguments) or a per-clip array.
    ``step`` = ``(p, q)`` (one id only): frame ``f`` of a clip is frame
    ``start + (f * p) // q`` of the video (``sampler.clip_frames``)."""
    single = isinstance(vids, int)
    n = len(starts)
    shape = (n * F, H * 3 // 2, W)
    stepped = tuple(step) != (1, 1)
    if stepped and not single:
        raise ValueError("nv12gen: a step goes with one video id, not a per-clip array")
    if device.type == "cuda":
        from .native import kernels
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream
        if stepped:          # the device-array form has no step: 32 clips per launch
            for i in range(0, n, 32):
                kernels().nv12gen_video_step(out[i * F:].data_ptr(), vids,
                                             list(starts[i:i + 32]), F, H, W, step, stream)
        elif single and n <= 32:
            kernels().nv12gen_video(out.data_ptr(), vids, list(starts), F, H, W, stream)
        else:
            v = torch.full((n,), vids, dtype=torch.int32, device=device) if single else \
                vids.to(device=device, dtype=torch.int32).contiguous()
            st = starts if isinstance(starts, torch.Tensor) else \
                torch.as_tensor(list(starts), dtype=torch.int32)
            st = st.to(device=device, dtype=torch.int32).contiguous()
            kernels().nv12gen(out.data_ptr(), v.data_ptr(), st.data_ptr(), n, F, H, W, stream)
        return out
    # CPU mirror of nv12gen_kernel
    v = torch.full((n,), vids, dtype=torch.int64) if single else \
        torch.as_tensor(vids, dtype=torch.int64).view(-1)
    st = torch.as_tensor(list(starts) if not isinstance(starts, torch.Tensor) else starts,
                         dtype=torch.int64).view(-1)
    fr = (st.view(n, 1) + _clip_frame_offsets(F, step).view(1, F)).reshape(-1)   # [n*F]
    vv = v.view(n, 1).expand(n, F).reshape(-1)
    ypix = torch.arange(H * W, dtype=torch.int64).view(1, -1)
    y = _pixel_hash_torch(vv.view(-1, 1), fr.view(-1, 1), ypix, torch.zeros(1, dtype=torch.int64))
    c = torch.arange(H * W // 2, dtype=torch.int64).view(1, -1)
    uv = _pixel_hash_torch(vv.view(-1, 1), fr.view(-1, 1), c >> 1, 1 + (c & 1))
    uv = (64 + (uv.to(torch.int64) >> 1)).to(torch.uint8)
    res = torch.cat([y.view(-1, H, W), uv.view(-1, H // 2, W)], dim=1).contiguous()
    if out is not None:
        out.copy_(res)
        return out
    return res


def _norm32(mean, std):
    """Normalisation constants as the kernels compute them (fp32 arithmetic)."""
    m32 = torch.tensor(mean, dtype=torch.float32)
    s32 = torch.tensor(std, dtype=torch.float32)
    return torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(255.0) * s32), -m32 / s32


def _bilinear_torch(plane: torch.Tensor, sx: torch.Tensor, sy: torch.Tensor) -> torch.Tensor:
    """plane [F, h, w] float; sample at (sy[:, None], sx[None, :]) with edge clamp."""
    Fn, h, w = plane.shape
    sx = sx.clamp(0, w - 1)
    sy = sy.clamp(0, h - 1)
    x0, y0 = sx.floor().long(), sy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    fx, fy = (sx - x0.float()).view(1, 1, -1), (sy - y0.float()).view(1, -1, 1)
    p00 = plane[:, y0][:, :, x0]
    p01 = plane[:, y0][:, :, x1]
    p10 = plane[:, y1][:, :, x0]
    p11 = plane[:, y1][:, :, x1]
    top = p00 + (p01 - p00) * fx
    bot = p10 + (p11 - p10) * fx
    return top + (bot - top) * fy


def nv12_to_clip(nv12: torch.Tensor, src_w: int, src_h: int, out_w: int = 112,
                 out_h: int = 112, crop=None, dtype=torch.float32, mean=KINETICS_MEAN,
                 std=KINETICS_STD, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NV12 frames [frames, H*3/2, W] -> normalised NDHWC frames
    [frames, out_h, out_w, C] (fp32 C=4 / bf16 C=8): bilinear scaling of the
    ``crop`` box (x, y, w, h; default the whole frame) with align_corners =
    false, BT.601 video-range YUV -> RGB, clamp, Kinetics normalisation (what
    NVVL does after NVDEC; reference model.py:123-125)."""
    frames = nv12.shape[0]
    crop = tuple(float(c) for c in (crop or (0, 0, src_w, src_h)))
    shape = (frames, out_h, out_w, clip_channels(dtype))
    if nv12.is_cuda:
        from .native import kernels
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=nv12.device)
        elif out.dtype != dtype or not out.is_contiguous() or out.numel() != math.prod(shape):
            raise ValueError("nv12_to_clip: out must be contiguous %s %s" % (dtype, shape))
        kernels().nv12_to_clip(nv12.data_ptr(), out.data_ptr(), frames, src_w, src_h, out_w,
                               out_h, crop, mean, std, dtype == torch.bfloat16,
                               torch.cuda.current_stream(nv12.device).cuda_stream)
        return out
    y_plane = nv12[:, :src_h].float()
    uv = nv12[:, src_h:].float().view(frames, src_h // 2, src_w // 2, 2)
    return _planes_to_clip(y_plane, uv[..., 0], uv[..., 1], shape, crop, dtype, mean, std, out)


MATRICES = ("bt601", "jfif")
FILTERS = ("bilinear", "antialias")


def _antialias_weights(n_src: int, n_out: int, start: float, size: float) -> torch.Tensor:
    """fp32 [n_out, n_src]: the triangle filter widened by the downscale factor,
    over the plane's own samples only, every row renormalised to 1."""
    scale = torch.tensor(size, dtype=torch.float32) / n_out
    fs = scale.clamp(min=1.0)
    s = start + (torch.arange(n_out, dtype=torch.float32) + 0.5) * scale - 0.5
    j = torch.arange(n_src, dtype=torch.float32)
    w = (1.0 - (j.view(1, -1) - s.view(-1, 1)).abs() / fs).clamp(min=0.0)
    return w / w.sum(dim=1, keepdim=True)


def _antialias_torch(plane: torch.Tensor, out_w: int, out_h: int, box) -> torch.Tensor:
    """plane [F, h, w] float -> [F, out_h, out_w]: rows first, then columns, as
    ``yuv420_clip_aa_kernel`` does (horizontal pass into LDS, vertical sum)."""
    _, h, w = plane.shape
    mx = _antialias_weights(w, out_w, box[0], box[2])
    my = _antialias_weights(h, out_h, box[1], box[3])
    return torch.matmul(my, torch.matmul(plane, mx.t()))


def _planes_to_clip(y_plane, u_plane, v_plane, shape, crop, dtype, mean, std, out,
                    matrix="bt601", filter="bilinear", factors=(2, 2)):
    """CPU mirror shared by ``nv12_to_clip`` and ``yuv420_to_clip``: float Y
    [frames, h, w] and U, V [frames, h/2, w/2] planes -> ``shape`` =
    [..., out_h, out_w, C] normalised frames. ``matrix``: ``"bt601"`` (video
    range) or ``"jfif"`` (full-range JFIF YCbCr). ``filter``: ``"bilinear"``
    (two taps) or ``"antialias"`` (``_antialias_torch``; chroma from the chroma
    box = luma box / 2 on the chroma plane). ``factors``: the luma sampling
    factors (Hs, Vs); along an axis with factor 1 the chroma plane has the luma
    size and the chroma coordinate is the luma coordinate."""
    out_h, out_w = shape[-3], shape[-2]
    hs, vs = factors
    if filter == "antialias":
        cbox = tuple(c / 2.0 if f == 2 else c for c, f in zip(crop, (hs, vs, hs, vs)))
        yv = _antialias_torch(y_plane, out_w, out_h, crop)
        u = _antialias_torch(u_plane, out_w, out_h, cbox) - 128.0
        v = _antialias_torch(v_plane, out_w, out_h, cbox) - 128.0
    else:
        ox = torch.arange(out_w, dtype=torch.float32)
        oy = torch.arange(out_h, dtype=torch.float32)
        sx = crop[0] + (ox + 0.5) * (crop[2] / out_w) - 0.5
        sy = crop[1] + (oy + 0.5) * (crop[3] / out_h) - 0.5
        yv = _bilinear_torch(y_plane, sx, sy)
        cx = (sx + 0.5) * 0.5 - 0.5 if hs == 2 else sx
        cy = (sy + 0.5) * 0.5 - 0.5 if vs == 2 else sy
        u = _bilinear_torch(u_plane, cx, cy) - 128.0
        v = _bilinear_torch(v_plane, cx, cy) - 128.0
    if matrix == "jfif":
        rgb = torch.stack([yv + 1.402 * v, yv - 0.344136 * u - 0.714136 * v, yv + 1.772 * u],
                          dim=-1)
    else:
        yy = 1.164 * (yv - 16.0)
        rgb = torch.stack([yy + 1.596 * v, yy - 0.392 * u - 0.813 * v, yy + 2.017 * u], dim=-1)
    scale, shift = _norm32(mean, std)
    rgb = rgb.clamp(0.0, 255.0) * scale + shift
    res = torch.zeros(shape, dtype=torch.float32)
    res.view(-1, out_h, out_w, shape[-1])[..., :3] = rgb
    res = res.to(dtype)
    if out is not None:
        out.copy_(res.view(out.shape))
        return out
    return res


SAMPLINGS = ("420", "422", "444")
# luma sampling factors (Hs, Vs) of each; both chroma planes are 1x1
SAMPLING_FACTORS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}


def sampling_factors(sampling: str, who: str = "sampling_factors") -> Tuple[int, int]:
    """(Hs, Vs) of ``sampling``; ``ValueError`` naming the argument otherwise."""
    if sampling not in SAMPLING_FACTORS:
        raise ValueError("%s: sampling must be one of %s, got %r" % (who, SAMPLINGS, sampling))
    return SAMPLING_FACTORS[sampling]


class YuvPlanes(NamedTuple):
    """Where a frame's planar YUV samples lie, in bytes from the frame's start:
    offsets and row strides of the Y, U and V planes, and the distance between
    chroma samples (1: planar, 2: interleaved UV with ``v = u + 1``)."""
    y: int
    u: int
    v: int
    y_stride: int
    u_stride: int
    v_stride: int
    c_step: int = 1


def i420_planes(W: int, H: int, header: int = 0) -> YuvPlanes:
    """Planar I420 (Y, then U, then V) behind ``header`` bytes, e.g. the 6-byte
    ``FRAME\\n`` marker of a YUV4MPEG2 frame."""
    return YuvPlanes(header, header + W * H, header + W * H + (W // 2) * (H // 2),
                     W, W // 2, W // 2, 1)


def i422_planes(W: int, H: int, header: int = 0) -> YuvPlanes:
    """Planar 4:2:2 (Y, then U, then V of W/2 x H) behind ``header`` bytes."""
    return YuvPlanes(header, header + W * H, header + W * H + (W // 2) * H,
                     W, W // 2, W // 2, 1)


def i444_planes(W: int, H: int, header: int = 0) -> YuvPlanes:
    """Planar 4:4:4 (Y, then U, then V, all W x H) behind ``header`` bytes."""
    return YuvPlanes(header, header + W * H, header + 2 * W * H, W, W, W, 1)


def nv12_planes(W: int, H: int, header: int = 0) -> YuvPlanes:
    """NV12 (Y, then interleaved UV rows of W bytes) behind ``header`` bytes."""
    return YuvPlanes(header, header + W * H, header + W * H + 1, W, W, W, 2)


BOX_ROWS_IN_ARGS = 64      # rows whose offset and box travel in the kernel arguments


def _crop_boxes(crop, n: int):
    """``None`` for no crop or one box (x, y, w, h); a list of ``n`` float
    4-tuples for a sequence of boxes, one per clip (``ValueError`` otherwise)."""
    if crop is None:
        return None
    if isinstance(crop, (torch.Tensor, np.ndarray)):
        crop = crop.tolist()
    crop = list(crop)
    if crop and all(isinstance(c, numbers.Real) for c in crop):
        return None
    boxes = [tuple(float(c) for c in box) for box in crop]
    if len(boxes) != n or any(len(b) != 4 for b in boxes):
        raise ValueError("yuv420_to_clip: crop must be one box (x, y, w, h) or one box per "
                         "clip: %d boxes for %d clips" % (len(boxes), n))
    return boxes


def _first_box_outside(boxes, src_w: int, src_h: int):
    """The first box that does not lie inside the frame, or ``None``: the boxes as
    the kernel gets them (fp32), summed in double, the launcher's own check."""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    ok = ((b[:, 0] >= 0) & (b[:, 1] >= 0) & (b[:, 2] > 0) & (b[:, 3] > 0)
          & (b[:, 0] + b[:, 2] <= src_w) & (b[:, 1] + b[:, 3] <= src_h))
    return None if ok.all() else tuple(boxes[int(np.argmin(ok))])


def yuv420_to_clip(buf: torch.Tensor, clip_offsets, F: int, src_w: int, src_h: int,
                   frame_stride: int, planes: YuvPlanes, out_w: int = 112, out_h: int = 112,
                   crop=None, dtype=torch.float32, mean=KINETICS_MEAN, std=KINETICS_STD,
                   out: Optional[torch.Tensor] = None, matrix: str = "bt601",
                   filter: str = "bilinear", sampling: str = "420") -> torch.Tensor:
    """4:2:0 frames inside a byte buffer -> normalised NDHWC clips
    [n, F, out_h, out_w, C] (fp32 C=4 / bf16 C=8), with ``nv12_to_clip``'s
    arithmetic. ``buf`` is a flat uint8 tensor (uploaded file spans); clip ``c``
    is the ``F`` frames that start at byte ``clip_offsets[c]`` and lie
    ``frame_stride`` bytes apart; ``planes`` (``YuvPlanes``) locates the samples
    within a frame. No alignment of any offset is assumed. One kernel launch
    for all clips; every span is checked against ``buf`` before it.
    ``matrix="bt601"`` is ``nv12_to_clip``'s video-range matrix and needs even
    frame sizes; ``matrix="jfif"`` is the full-range JFIF YCbCr of JPEG frames
    (R = Y + 1.402 (Cr - 128), G = Y - 0.344136 (Cb - 128) - 0.714136 (Cr - 128),
    B = Y + 1.772 (Cb - 128)) and takes any size, with chroma planes of
    ceil(w / 2) x ceil(h / 2).

    ``filter="bilinear"`` (default) samples two taps per axis, whatever the
    scale. ``filter="antialias"`` is the triangle filter widened by the
    downscale factor, PIL's ``resize(BILINEAR)`` / torch's ``antialias=True``:
    per axis ``scale = size / n_out``, ``fs = max(scale, 1)``, weights
    ``max(0, 1 - |j - s_o| / fs)`` over the plane's own samples, renormalised
    (``yuv420_clip_aa_kernel``; for ``scale <= 1`` the same as bilinear). It
    needs ``crop`` inside the frame and raises ``ValueError`` otherwise.

    ``sampling``: ``"420"`` (default), ``"422"`` or ``"444"``, luma factors
    (Hs, Vs) = (2, 2), (2, 1), (1, 1). The chroma planes are ceil(w / Hs) x
    ceil(h / Vs) (JFIF) or w / Hs x h / Vs (BT.601, even size needed only along
    an axis with factor 2); chroma sample j sits at luma Hs j + (Hs - 1) / 2.

    ``crop``: ``None`` (the whole frame), one box ``(x, y, w, h)`` for every
    clip, or a sequence of ``n`` boxes, one per entry of ``clip_offsets``. With
    a sequence, entries may repeat an offset: several views of one clip read
    one uploaded span, in one launch. ``filter="antialias"`` checks every box.

    On the GPU every form is one ``rnb_yuv_to_clip_boxes`` launch with a box per
    row; one box (or ``None``) is that box in every row. Up to
    ``BOX_ROWS_IN_ARGS`` = 64 rows travel in the kernel arguments; more go
    through two device tables, uploaded here (a ``clip_offsets`` that is a
    tensor on ``buf``'s device is the offset table as it stands). One box used
    to switch to a device table past 32 rows; it now does so past 64, like a
    box per row."""
    hs, vs = sampling_factors(sampling, "yuv420_to_clip")
    if matrix not in MATRICES:
        raise ValueError("yuv420_to_clip: matrix must be one of %s, got %r" % (MATRICES, matrix))
    if filter not in FILTERS:
        raise ValueError("yuv420_to_clip: filter must be one of %s, got %r" % (FILTERS, filter))
    jfif = matrix == "jfif"
    offsets = [int(o) for o in (clip_offsets.tolist() if isinstance(clip_offsets, torch.Tensor)
                                else clip_offsets)]
    n = len(offsets)
    planes = YuvPlanes(*planes)
    boxes = _crop_boxes(crop, n)
    if boxes is None:
        crop = tuple(float(c) for c in (crop if crop is not None else (0, 0, src_w, src_h)))
    shape = (n, F, out_h, out_w, clip_channels(dtype))
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
        raise ValueError("yuv420_to_clip: buf must be a flat contiguous uint8 tensor")
    if out is not None and (out.dtype != dtype or not out.is_contiguous()
                            or out.numel() != math.prod(shape)):
        raise ValueError("yuv420_to_clip: out must be contiguous %s %s" % (dtype, shape))
    antialias = filter == "antialias"
    if antialias:
        bad = _first_box_outside([crop] if boxes is None else boxes, src_w, src_h)
        if bad is not None:
            raise ValueError("yuv420_to_clip: filter='antialias' needs the crop box inside "
                             "the %d x %d frame, got %r" % (src_w, src_h, bad))
    if buf.is_cuda:
        from .native import kernels
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=buf.device)
        # the rows' boxes as packed fp32: the cheapest table to build per call
        flat = struct.pack("4f", *crop) * n if boxes is None else \
            struct.pack("%df" % (4 * n), *itertools.chain.from_iterable(boxes))
        table = box_table = None
        if n > BOX_ROWS_IN_ARGS:       # past the kernel-argument tables: both in device memory
            table = clip_offsets if isinstance(clip_offsets, torch.Tensor) else \
                torch.tensor(offsets, dtype=torch.int64)
            table = table.to(device=buf.device, dtype=torch.int64).contiguous()
            box_table = torch.frombuffer(bytearray(flat), dtype=torch.float32).to(buf.device)
        kernels().yuv_to_clip_boxes(buf.data_ptr(), buf.numel(), offsets,
                                    None if table is None else table.data_ptr(), F, src_w,
                                    src_h, frame_stride, planes[:3], planes[3:6], planes.c_step,
                                    out.data_ptr(), out_w, out_h, flat,
                                    None if box_table is None else box_table.data_ptr(), mean,
                                    std, dtype == torch.bfloat16,
                                    torch.cuda.current_stream(buf.device).cuda_stream,
                                    matrix=1 if jfif else 0, antialias=antialias,
                                    sampling=SAMPLINGS.index(sampling))
        return out
    if (not jfif and ((hs == 2 and src_w % 2) or (vs == 2 and src_h % 2))) \
            or planes.c_step not in (1, 2):
        raise ValueError("yuv420_to_clip: even frame sizes and a chroma step of 1 or 2")
    if any(o < 0 or o + F * frame_stride > buf.numel() for o in offsets):
        raise ValueError("yuv420_to_clip: a clip span lies outside the buffer")
    cw = (src_w + jfif) // 2 if hs == 2 else src_w
    ch = (src_h + jfif) // 2 if vs == 2 else src_h
    base = (torch.tensor(offsets, dtype=torch.int64).view(n, 1)
            + torch.arange(F, dtype=torch.int64).view(1, F) * frame_stride).view(-1, 1, 1)

    def gather(off, stride, rows, cols, step):
        idx = base + off + torch.arange(rows).view(1, rows, 1) * stride \
            + torch.arange(cols).view(1, 1, cols) * step
        return buf[idx].float()
    yp = gather(planes.y, planes.y_stride, src_h, src_w, 1)
    up = gather(planes.u, planes.u_stride, ch, cw, planes.c_step)
    vp = gather(planes.v, planes.v_stride, ch, cw, planes.c_step)
    if boxes is None:
        return _planes_to_clip(yp, up, vp, shape, crop, dtype, mean, std, out, matrix, filter,
                               (hs, vs))
    res = torch.stack([_planes_to_clip(yp[c * F:(c + 1) * F], up[c * F:(c + 1) * F],
                                       vp[c * F:(c + 1) * F], shape[1:], boxes[c], dtype, mean,
                                       std, None, matrix, filter, (hs, vs))
                       for c in range(n)]) if n else torch.zeros(shape, dtype=dtype)
    if out is not None:
        out.copy_(res.view(out.shape))
        return out
    return res


# ---------------------------------------------------------------------------
# MJPEG frame records (utils/mjpeg.py) -> padded I420 surfaces
# ---------------------------------------------------------------------------
JPEG_REDUCES = (1, 2, 4, 8)


def jpeg_reduce_points(reduce, who: str = "jpeg_reduce_points") -> int:
    """N = 8 / ``reduce``, the samples a block keeps per axis at a reduced-size
    decode; ``ValueError`` naming the argument for what is not 1, 2, 4 or 8."""
    if isinstance(reduce, bool) or reduce not in JPEG_REDUCES:
        raise ValueError("%s: reduce must be one of %s, got %r" % (who, JPEG_REDUCES, reduce))
    return 8 // int(reduce)


def jpeg_surface_planes(mw: int, mh: int, sampling: str = "420", reduce: int = 1) -> YuvPlanes:
    """Where ``jpeg_idct`` puts a frame's planes: Y [8 Vs mh, 8 Hs mw], then Cb
    and Cr [8 mh, 8 mw]; frame stride ``64 B mw mh``, B = Hs Vs + 2 (4:2:0:
    ``384 mw mh``). With ``reduce`` = s, N = 8 / s: Y [N Vs mh, N Hs mw], Cb and
    Cr [N mh, N mw], frame stride ``N^2 B mw mh``."""
    hs, vs = sampling_factors(sampling, "jpeg_surface_planes")
    N = jpeg_reduce_points(reduce, "jpeg_surface_planes")
    n, ny = mw * mh, hs * vs
    return YuvPlanes(0, N * N * ny * n, N * N * (ny + 1) * n, N * hs * mw, N * mw, N * mw, 1)


def jpeg_frame_bytes(mw: int, mh: int, sampling: str = "420", reduce: int = 1) -> Tuple[int, int]:
    """(frame record bytes, surface frame bytes) of an ``mw`` x ``mh`` MCU grid;
    the records do not depend on ``reduce``, the surface is ``(8 / reduce)^2 B
    mw mh`` bytes."""
    hs, vs = sampling_factors(sampling, "jpeg_frame_bytes")
    N = jpeg_reduce_points(reduce, "jpeg_frame_bytes")
    nb = hs * vs + 2
    return 384 + 128 * nb * mw * mh, N * N * nb * mw * mh


def jpeg_idct(records: torch.Tensor, nframes: int, mw: int, mh: int,
              out: Optional[torch.Tensor] = None,
              record_bytes: Optional[int] = None, sampling: str = "420",
              reduce: int = 1) -> torch.Tensor:
    """Dequantise + 8x8 inverse DCT of ``nframes`` frame records (flat uint8
    tensor, ``record_bytes`` apart, default ``384 + 768 mw mh``; layout in
    ``utils/mjpeg.py``) into 8-bit planar frames at the padded size: per frame
    Y [16 mh, 16 mw], then Cb and Cr [8 mh, 8 mw], ``384 mw mh`` bytes. ``out``:
    a flat uint8 surface to write into (the result is its leading part). fp32
    arithmetic, + 128, round to nearest, clamp. On the GPU one
    ``jpeg_idct_kernel`` launch, after the launcher checked both buffers
    against the geometry; on the CPU a torch mirror.

    ``sampling`` ``"422"`` / ``"444"``: records of ``384 + 128 B mw mh`` bytes
    (B = 4 / 3 blocks per MCU, the Y blocks over the ``Vs mh x Hs mw`` grid)
    into frames of Y [8 Vs mh, 8 Hs mw], Cb, Cr [8 mh, 8 mw], ``64 B mw mh``
    bytes.

    ``reduce`` = s in 1, 2, 4, 8 (``ValueError`` otherwise): the reduced-size
    decode of libjpeg's ``scale_denom`` / PIL's ``draft``. With N = 8 / s a
    block gives N x N samples, each the s x s box mean of the unrounded,
    unclamped full-size samples (the same separable transform with the basis
    averaged over s rows), then + 128, round, clamp: frames of Y
    [N Vs mh, N Hs mw], Cb, Cr [N mh, N mw], ``N^2 B mw mh`` bytes; the frame's
    ``ceil(W / s) x ceil(H / s)`` corner is the picture. The records are the
    same. ``reduce=1`` is the code path and the bytes of the full-size decode;
    the others run ``jpeg_idct_reduced_kernel`` (s = 2, 4) or
    ``jpeg_idct_dc_kernel`` (s = 8: ``F[0][0] / 8 + 128``)."""
    hs, vs = sampling_factors(sampling, "jpeg_idct")
    N = jpeg_reduce_points(reduce, "jpeg_idct")
    n, ny = mw * mh, hs * vs
    rb_min, fbytes = jpeg_frame_bytes(mw, mh, sampling, reduce)
    rb = rb_min if record_bytes is None else int(record_bytes)
    need = nframes * fbytes
    if records.dtype != torch.uint8 or records.dim() != 1 or not records.is_contiguous():
        raise ValueError("jpeg_idct: records must be a flat contiguous uint8 tensor")
    if out is not None and (out.dtype != torch.uint8 or out.dim() != 1
                            or not out.is_contiguous() or out.device != records.device):
        raise ValueError("jpeg_idct: out must be a flat contiguous uint8 tensor on %s"
                         % (records.device,))
    if records.is_cuda:
        from .native import kernels
        if out is None:
            out = torch.empty(need, dtype=torch.uint8, device=records.device)
        kernels().jpeg_idct(records.data_ptr(), records.numel(), rb, nframes, mw, mh,
                            out.data_ptr(), out.numel(),
                            torch.cuda.current_stream(records.device).cuda_stream,
                            sampling=SAMPLINGS.index(sampling), reduce=int(reduce))
        return out[:need]
    if mw < 1 or mh < 1 or rb < rb_min or nframes * rb > records.numel() \
            or (out is not None and out.numel() < need):
        raise ValueError("jpeg_idct: a record or a frame lies outside its buffer")
    rec = records[:nframes * rb].view(nframes, rb)
    qt = rec[:, :384].contiguous().view(torch.int16).view(nframes, 3, 1, 64).float()
    co = rec[:, 384:rb_min].contiguous().view(torch.int16).view(nframes, (ny + 2) * n, 64).float()
    u = torch.arange(8, dtype=torch.float64)
    basis = 0.5 * torch.cos((2.0 * u.view(8, 1) + 1.0) * u.view(1, 8) * math.pi / 16.0)
    basis[:, 0] *= math.sqrt(0.5)
    if N != 8:                                              # Bs[i][u]: the mean of 8 / N rows
        basis = basis.view(N, 8 // N, 8).mean(dim=1)
    basis = basis.float()                                   # [x][u], as the kernel's table
    planes = []
    for c, (lo, hi, rows, cols) in enumerate(((0, ny * n, vs * mh, hs * mw),
                                              (ny * n, (ny + 1) * n, mh, mw),
                                              ((ny + 1) * n, (ny + 2) * n, mh, mw))):
        f = (co[:, lo:hi] * qt[:, c]).view(nframes, -1, 8, 8)           # [frame, block, u, v]
        s = torch.einsum("xu,fbuv,yv->fbxy", basis, f, basis) + 128.0
        s = s.round().clamp(0, 255).to(torch.uint8)
        planes.append(s.view(nframes, rows, cols, N, N).permute(0, 1, 3, 2, 4)
                      .reshape(nframes, -1))
    res = torch.cat(planes, dim=1).reshape(-1)
    if out is not None:
        out[:need].copy_(res)
        return out[:need]
    return res


def jpeg_huff(scans: torch.Tensor, scan_offs, nframes: int, mw: int, mh: int,
              out: Optional[torch.Tensor] = None, record_bytes: Optional[int] = None,
              status: Optional[torch.Tensor] = None,
              offs_dev: Optional[torch.Tensor] = None, subseq_bytes: int = 0,
              rounds: Optional[torch.Tensor] = None,
              sampling: str = "420") -> Tuple[torch.Tensor, torch.Tensor]:
    """Huffman-decode ``nframes`` packed scan records (``utils/mjpeg.py:
    pack_scans``; flat uint8 tensor ``scans``, record ``i`` at
    ``scan_offs[i] : scan_offs[i + 1]``, ``scan_offs`` a host table of
    ``nframes + 1`` int64 offsets) into frame records ``record_bytes`` apart
    (default ``384 + 768 mw mh``). Returns ``(records, status)``: the leading
    ``nframes`` records of ``out`` (a flat uint8 tensor, allocated if not
    given) and an int32 tensor with 0 or the code of each frame's
    lowest-numbered failing interval (``mjpeg.status_field``); a frame or an
    interval that fails has zero blocks. Every block is written.

    On the GPU one ``jpeg_huff_kernel`` launch, one workgroup per frame and one
    lane per restart interval, asynchronous: ``status`` is read by whoever
    synchronises. ``offs_dev``: the offset table on the device (int64, e.g. a
    view of the upload); uploaded here when not given. The launcher refuses
    (``RuntimeError``) without launching when a record would reach outside its
    buffer or is misaligned. On the CPU ``rnb_jpeg_decode_scans_host``, the
    same decode loop.

    ``subseq_bytes`` > 0 (a multiple of 16 in 16..4096, else ``ValueError``
    before anything is launched) selects ``jpeg_huff_subseq_kernel``: a frame
    whose scan is one interval (no restart markers) is cut into subsequences
    of that many scan bytes, which the lanes of its workgroup decode in
    parallel and synchronise (``csrc/jpeg_huff.h``); frames with restart
    markers go lane per interval as above. Records and status are the same
    byte for byte. ``rounds``: an int32 tensor of >= ``nframes`` on the
    device of ``scans`` that receives each frame's synchronisation rounds
    (allocated and dropped when not given). On the CPU the kernel's host
    emulation, ``rnb_jpeg_decode_scans_subseq_host``.

    ``sampling``: the geometry ``mw`` / ``mh`` count MCUs of (records default to
    ``384 + 128 B mw mh`` bytes). The kernels take it from here, never from the
    scan record; a record whose sampling word differs gets the status
    'scan record'."""
    import numpy as np
    from ..utils import mjpeg
    subseq_bytes = mjpeg.check_subseq_bytes(subseq_bytes, "jpeg_huff")
    sampling_factors(sampling, "jpeg_huff")
    rb = jpeg_frame_bytes(mw, mh, sampling)[0] if record_bytes is None else int(record_bytes)
    offs = np.ascontiguousarray(scan_offs.numpy() if isinstance(scan_offs, torch.Tensor)
                                else scan_offs, dtype=np.int64)
    if offs.ndim != 1 or offs.size != nframes + 1:
        raise ValueError("jpeg_huff: scan_offs must hold nframes + 1 = %d offsets" % (nframes + 1))
    if scans.dtype != torch.uint8 or scans.dim() != 1 or not scans.is_contiguous():
        raise ValueError("jpeg_huff: scans must be a flat contiguous uint8 tensor")
    if out is not None and (out.dtype != torch.uint8 or out.dim() != 1
                            or not out.is_contiguous() or out.device != scans.device):
        raise ValueError("jpeg_huff: out must be a flat contiguous uint8 tensor on %s"
                         % (scans.device,))
    if status is not None and (status.dtype != torch.int32 or status.dim() != 1
                               or not status.is_contiguous() or status.device != scans.device
                               or status.numel() < nframes):
        raise ValueError("jpeg_huff: status must be a contiguous int32 tensor of >= %d on %s"
                         % (nframes, scans.device))
    if rounds is not None and (rounds.dtype != torch.int32 or rounds.dim() != 1
                               or not rounds.is_contiguous() or rounds.device != scans.device
                               or rounds.numel() < nframes):
        raise ValueError("jpeg_huff: rounds must be a contiguous int32 tensor of >= %d on %s"
                         % (nframes, scans.device))
    if rounds is None and subseq_bytes:
        rounds = torch.zeros(nframes, dtype=torch.int32, device=scans.device)
    if out is None:
        out = torch.empty(nframes * rb, dtype=torch.uint8, device=scans.device)
    if status is None:
        status = torch.zeros(nframes, dtype=torch.int32, device=scans.device)
    if scans.is_cuda:
        from .native import kernels
        if offs_dev is None:
            offs_dev = torch.from_numpy(offs).to(scans.device)
        elif offs_dev.dtype != torch.int64 or offs_dev.device != scans.device \
                or not offs_dev.is_contiguous() or offs_dev.numel() < nframes + 1:
            raise ValueError("jpeg_huff: offs_dev must be >= %d contiguous int64 on %s"
                             % (nframes + 1, scans.device))
        stream = torch.cuda.current_stream(scans.device).cuda_stream
        if subseq_bytes:
            kernels().jpeg_huff_subseq(scans.data_ptr(), scans.numel(), offs, offs_dev.data_ptr(),
                                       nframes, mw, mh, out.data_ptr(), out.numel(), rb,
                                       status.data_ptr(), subseq_bytes, rounds.data_ptr(), stream,
                                       sampling=SAMPLINGS.index(sampling))
        else:
            kernels().jpeg_huff(scans.data_ptr(), scans.numel(), offs, offs_dev.data_ptr(),
                                nframes, mw, mh, out.data_ptr(), out.numel(), rb,
                                status.data_ptr(), stream, sampling=SAMPLINGS.index(sampling))
        return out[:nframes * rb], status[:nframes]
    try:
        got = mjpeg.decode_scans_host(scans.numpy(), offs, nframes, mw, mh, out.numpy(), rb,
                                      status.numpy(), subseq_bytes=subseq_bytes,
                                      return_rounds=True, sampling=sampling)
    except mjpeg.JpegError:
        raise ValueError("jpeg_huff: a scan record or a frame record lies outside its buffer, "
                         "or is misaligned")
    if rounds is not None:
        rounds[:nframes].copy_(torch.from_numpy(got[2]))
    return out[:nframes * rb], status[:nframes]


def preprocess(frames_u8: torch.Tensor, mean=KINETICS_MEAN, std=KINETICS_STD,
               out: Optional[torch.Tensor] = None, packed: bool = False,
               dtype=torch.bfloat16) -> torch.Tensor:
    """uint8 [n, F, H, W, 3] -> normalised bf16 [n, F, H, W, 8] (NDHWC).

    ``packed=True`` writes the stem conv's zero-bordered pixel-pair layout
    [n, F, H+6, (W+6)/2, 8] instead (``ops.conv.stem_pack`` of the NDHWC
    result, in one pass: ``video_ops.hip: preprocess_packed_kernel``).
    ``dtype=torch.float32`` (the reference precision) writes fp32
    [n, F, H, W, 4] (``preprocess_f32_kernel``).
    """
    n, F, H, W, C = frames_u8.shape
    assert C == 3
    if dtype == torch.float32:
        if packed:
            raise ValueError("the packed stem layout is bf16 only")
        return _preprocess_f32(frames_u8, mean, std, out)
    if packed:
        return _preprocess_packed(frames_u8, mean, std, out)
    if frames_u8.is_cuda:
        from .native import kernels
        if out is None:
            out = torch.empty((n, F, H, W, IN_CHANNELS_P), dtype=torch.bfloat16,
                              device=frames_u8.device)
        kernels().preprocess(frames_u8.contiguous().data_ptr(), out.data_ptr(),
                             n * F * H * W, mean, std,
                             torch.cuda.current_stream(frames_u8.device).cuda_stream)
        return out
    scale = torch.tensor([1.0 / (255.0 * s) for s in std], dtype=torch.float32)
    shift = torch.tensor([-m / s for m, s in zip(mean, std)], dtype=torch.float32)
    y = frames_u8.float() * scale + shift
    res = torch.zeros((n, F, H, W, IN_CHANNELS_P), dtype=torch.bfloat16)
    res[..., :3] = y.to(torch.bfloat16)
    if out is not None:
        out.copy_(res)
        return out
    return res


def _preprocess_f32(frames_u8, mean, std, out):
    n, F, H, W, _ = frames_u8.shape
    shape = (n, F, H, W, IN_CHANNELS_P_F32)
    if frames_u8.is_cuda:
        from .native import kernels
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=frames_u8.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("fp32 preprocess: out must be contiguous fp32 %s" % (shape,))
        kernels().preprocess_f32(frames_u8.contiguous().data_ptr(), out.data_ptr(),
                                 n * F * H * W, mean, std,
                                 torch.cuda.current_stream(frames_u8.device).cuda_stream)
        return out
    # same arithmetic as the kernel, which contracts x * scale + shift into one
    # fp32 fma (single rounding): the product of a u8 and an fp32 scale is exact
    # in fp64, so the fp64 sum rounded once to fp32 is the fma's result
    # (the launcher computes scale/shift in fp32 arithmetic, as here)
    m32 = torch.tensor(mean, dtype=torch.float32)
    s32 = torch.tensor(std, dtype=torch.float32)
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(255.0) * s32)
    shift = -m32 / s32
    res = torch.zeros(shape, dtype=torch.float32)
    res[..., :3] = (frames_u8.double() * scale.double() + shift.double()).float()
    if out is not None:
        out.copy_(res)
        return out
    return res


def packed_input_shape(n: int, F: int, H: int, W: int) -> Tuple[int, ...]:
    """Shape of the stem's pair-packed input for n clips of F x H x W."""
    return (n, F, H + 6, (W + 6) // 2, IN_CHANNELS_P)


def _preprocess_packed(frames_u8, mean, std, out):
    n, F, H, W, _ = frames_u8.shape
    if W % 2:
        raise ValueError("packed preprocess needs an even frame width, got %d" % W)
    shape = packed_input_shape(n, F, H, W)
    if frames_u8.is_cuda:
        from .native import kernels
        if out is None:
            out = torch.empty(shape, dtype=torch.bfloat16, device=frames_u8.device)
        elif tuple(out.shape) != shape or out.dtype != torch.bfloat16 or not out.is_contiguous():
            raise ValueError("packed preprocess: out must be contiguous bf16 %s" % (shape,))
        kernels().preprocess_packed(frames_u8.contiguous().data_ptr(), out.data_ptr(),
                                    n * F, H, W, mean, std,
                                    torch.cuda.current_stream(frames_u8.device).cuda_stream)
        return out
    from .conv import stem_pack
    res = stem_pack(preprocess(frames_u8, mean, std))
    if out is not None:
        out.copy_(res)
        return out
    return res


def ndhwc_to_ncdhw(x: torch.Tensor, channels: int) -> torch.Tensor:
    """Boundary tensor -> reference NCDHW float32 layout."""
    return x[..., :channels].permute(0, 4, 1, 2, 3).float().contiguous()


def ncdhw_to_ndhwc(x: torch.Tensor, channels_p: int, dtype=torch.bfloat16) -> torch.Tensor:
    """Reference NCDHW tensor -> NDHWC with channels padded to ``channels_p``."""
    y = x.permute(0, 2, 3, 4, 1)
    if y.shape[-1] != channels_p:
        y = torch.nn.functional.pad(y, (0, channels_p - y.shape[-1]))
    return y.to(dtype).contiguous()


class Head:
    """AdaptiveAvgPool3d(1) + Linear(C -> classes) on an NDHWC bf16 tensor."""

    def __init__(self, linear: torch.nn.Linear, device: torch.device):
        self.weight = linear.weight.detach().float().to(device).contiguous()
        # the kernel reads the transposed [C][classes] matrix (coalesced per class)
        self.weight_t = self.weight.t().contiguous()
        self.bias = linear.bias.detach().float().to(device).contiguous()
        self.num_classes, self.channels = self.weight.shape

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        N, T, H, W, Cs = x.shape
        if x.is_cuda:
            from .native import kernels
            if out is None:
                out = torch.empty((N, self.num_classes), dtype=torch.float32, device=x.device)
            pooled = torch.empty((N, self.channels), dtype=torch.float32, device=x.device)
            fn = kernels().head_f32 if x.dtype == torch.float32 else kernels().head
            if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
                raise ValueError("head: expected a contiguous fp32/bf16 NDHWC tensor")
            fn(x.data_ptr(), self.weight_t.data_ptr(), self.bias.data_ptr(),
               out.data_ptr(), pooled.data_ptr(), N, T * H * W, self.channels, Cs,
               self.num_classes, torch.cuda.current_stream(x.device).cuda_stream)
            return out
        return self.forward_torch(x)

    def forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        pooled = x[..., :self.channels].float().mean(dim=(1, 2, 3))
        return pooled @ self.weight.to(x.device).t() + self.bias.to(x.device)


def video_reduce(logits: torch.Tensor, offsets: torch.Tensor,
                 sums: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Sum clip logits per video ([offsets[v], offsets[v+1]) rows) + argmax."""
    nvid = offsets.numel() - 1
    ncls = logits.shape[1]
    if logits.is_cuda:
        from .native import kernels
        if sums is None:
            sums = torch.empty((nvid, ncls), dtype=torch.float32, device=logits.device)
        arg = torch.empty((nvid,), dtype=torch.int32, device=logits.device)
        kernels().video_reduce(logits.contiguous().data_ptr(),
                               offsets.to(torch.int32).contiguous().data_ptr(),
                               sums.data_ptr(), arg.data_ptr(), nvid, ncls,
                               torch.cuda.current_stream(logits.device).cuda_stream)
        return sums, arg
    off = offsets.tolist()
    out = torch.stack([logits[off[v]:off[v + 1]].sum(0) for v in range(nvid)]) \
        if nvid else torch.zeros((0, ncls))
    arg = torch.tensor([int(torch.argmax(out[v])) if off[v + 1] > off[v] else -1
                        for v in range(nvid)], dtype=torch.int32)
    return out, arg


SCORE_KINDS = ("logit_sum", "logit_mean", "softmax_sum", "softmax_mean")
SCORE_MAX_CLASSES = 4096
SCORE_MAX_K = 16


def check_score_args(scores: str, top_k: int, ncls: Optional[int] = None) -> None:
    """The limits of the video_scores kernel, shared with its CPU mirror."""
    if scores not in SCORE_KINDS:
        raise ValueError("video_scores: scores = %r, expected one of %s"
                         % (scores, ", ".join(SCORE_KINDS)))
    if ncls is not None and not 1 <= ncls <= SCORE_MAX_CLASSES:
        raise ValueError("video_scores: argument ncls = %d is outside 1..%d"
                         % (ncls, SCORE_MAX_CLASSES))
    if not 1 <= top_k <= SCORE_MAX_K or (ncls is not None and top_k > ncls):
        raise ValueError("video_scores: argument k = %d is outside 1..min(%d, ncls%s)"
                         % (top_k, SCORE_MAX_K, "" if ncls is None else " = %d" % ncls))


def top_k_stable(scores: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k largest per row, descending, ties to the lower index (a stable
    sort: ``torch.topk`` promises no tie order). Returns (values, int32 indices)."""
    order = torch.sort(scores, dim=1, descending=True, stable=True)[1][:, :k]
    return scores.gather(1, order), order.to(torch.int32)


def video_scores(logits: torch.Tensor, offsets: torch.Tensor, scores: str = "softmax_mean",
                 top_k: int = 5, out=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-video class scores over the rows [offsets[v], offsets[v+1]) + top-k.

    ``scores``: "logit_sum" / "logit_mean" add the rows as they are,
    "softmax_sum" / "softmax_mean" add each row's softmax; "_mean" divides by
    the row count. Returns (scores [nvid][ncls] fp32, top_val [nvid][k] fp32,
    top_idx [nvid][k] int32): the k largest scores, descending, ties to the
    lower class index. An empty video has scores 0, top_idx -1 and top_val 0.
    ``out``: the three tensors preallocated (graph capture). On a GPU this is
    one launch of the video_scores kernel; on the CPU a torch fp32 mirror."""
    nvid = offsets.numel() - 1
    ncls = int(logits.shape[1])
    k = int(top_k)
    check_score_args(scores, k, None)
    softmax, mean = scores.startswith("softmax"), scores.endswith("mean")
    if logits.is_cuda:
        from .native import kernels
        if logits.dtype != torch.float32:
            raise ValueError("video_scores: logits must be fp32, got %s" % logits.dtype)
        dev = logits.device
        if out is None:
            out = (torch.empty((nvid, ncls), dtype=torch.float32, device=dev),
                   torch.empty((nvid, k), dtype=torch.float32, device=dev),
                   torch.empty((nvid, k), dtype=torch.int32, device=dev))
        sc, tv, ti = out
        if sc.shape[0] < nvid or sc.shape[1] != ncls or tuple(tv.shape) != (sc.shape[0], k) \
                or tuple(ti.shape) != (sc.shape[0], k) or ti.dtype != torch.int32 \
                or sc.dtype != torch.float32 or tv.dtype != torch.float32 \
                or not (sc.is_contiguous() and tv.is_contiguous() and ti.is_contiguous()):
            raise ValueError("video_scores: out must be contiguous (fp32 [>=%d][%d], "
                             "fp32 [n][%d], int32 [n][%d])" % (nvid, ncls, k, k))
        kernels().video_scores(logits.contiguous().data_ptr(),
                               offsets.to(torch.int32).contiguous().data_ptr(),
                               sc.data_ptr(), tv.data_ptr(), ti.data_ptr(), nvid, ncls, k,
                               softmax, mean, torch.cuda.current_stream(dev).cuda_stream)
        return sc, tv, ti
    check_score_args(scores, k, ncls)
    off = offsets.tolist()
    rows = logits.float()
    if softmax:
        rows = torch.softmax(rows, dim=1)
    sc = torch.zeros((nvid, ncls), dtype=torch.float32)
    for v in range(nvid):
        n = off[v + 1] - off[v]
        if n > 0:
            sc[v] = rows[off[v]:off[v + 1]].sum(0)
            if mean:
                sc[v] /= n
    tv, ti = top_k_stable(sc, k)
    for v in range(nvid):
        if off[v + 1] <= off[v]:
            tv[v] = 0.
            ti[v] = -1
    if out is not None:
        for dst, src in zip(out, (sc, tv, ti)):
            dst[:nvid].copy_(src)
        return out
    return sc, tv, ti
