"""Clip decoders for the R(2+1)D loader stage.

The reference decodes with NVVL's ``RnBLoader`` (ffmpeg demux + NVDEC + CUDA
colour/resize kernels; reference model.py:116-158, README.md:42-110). On the
MI355X pool there is neither a video decoder library (rocDecode is not
installed) nor a dataset, so the default backend synthesises the decoder's
output surfaces on the GPU -- NV12 frames at the source resolution, 340x256,
deterministic per (video, frame) -- and runs the per-frame work a real
decoder's output goes through in NVVL: colour conversion and scaling to
112x112 (``nv12_to_clip`` HIP kernel). ``synthetic-rgb`` generates 112x112 RGB
frames directly (``clipgen`` + ``preprocess``). ``NpyDecoder`` is a real-I/O backend that
reads pre-decoded ``uint8 [frames, H, W, 3]`` ``.npy`` files (memory-mapped,
so only the sampled frames are read) and uploads them. ``Y4mDecoder`` reads raw
YUV4MPEG2 (``.y4m``) files at their source resolution: it uploads only the
sampled frames' file spans and scales / colour-converts them on the GPU
(``yuv420_to_clip`` HIP kernel, the planar-chroma sibling of ``nv12_to_clip``).
``MjpegDecoder`` reads Motion-JPEG streams (``.mjpeg``), the one compressed
format decoded here: Huffman decode on the host (``librnb_jpeg.so``), then
dequantisation and inverse DCT (``jpeg_idct`` HIP kernel) and the same
``yuv420_to_clip`` kernel with the full-range JFIF matrix on the GPU;
``reduce=2 | 4 | 8 | "auto"`` has the IDCT write the frame at 1/2, 1/4 or 1/8
size (libjpeg's ``scale_denom``).

A clip is ``clip_length`` frames of the file taken at a step: every ``decode``
takes ``step=(p, q)`` and reads the source frames ``sampler.clip_frames(start,
F, step)``, frame ``f`` at ``start + (f * p) // q``. ``(1, 1)``, the default,
is consecutive frames. ``source_fps_of(vid)`` is the file's frame rate as an
``(n, d)`` pair where one is known (the Y4M header's ``F`` field, else the
``source_fps`` constructor argument), which the loader turns into a step for a
target ``fps``.

Every decoder returns NDHWC clips normalised with the Kinetics mean/std:
``fp32 [n, 8, 112, 112, 4]`` (reference precision) or ``bf16 [n, 8, 112, 112, 8]``
(the layouts the fp32 / bf16 stem conv kernels consume).
"""
from __future__ import annotations

import contextlib
import math
import mmap
import numbers
import os
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ...ops import video as vops
from ...utils import mjpeg, y4m
from ...video_path_provider import parse_synthetic_path
from .sampler import clip_frames, clip_span, parse_rate


def _rate_pair(source_fps, name: str) -> Optional[Tuple[int, int]]:
    """A decoder's ``source_fps`` argument (a number or ``"n:d"``) as ``(n, d)``."""
    try:
        rate = parse_rate(source_fps, "source_fps")
    except ValueError as err:
        raise ValueError("%s: %s" % (name, err))
    return None if rate is None else (rate.numerator, rate.denominator)


class Decoder:
    dtype = torch.bfloat16
    views = 1                # output rows per clip (file-backed decoders: crop={"views": 3})
    source_fps = None        # (n, d) frames per second of the files, where it was given

    def probe(self, path: str) -> Tuple[int, int]:
        """(video id, number of frames)."""
        raise NotImplementedError

    def empty(self):
        return torch.zeros((0, self.F, self.H, self.W, vops.clip_channels(self.dtype)),
                           dtype=self.dtype, device=self.device)

    def warmup(self, n: int) -> None:
        """Run the decode kernels once per warm-up round (no probe needed)."""
        for i in range(n):
            self._decode_surface(torch.zeros((1, self.F, self.H, self.W, 3),
                                             dtype=torch.uint8, device=self.device))

    def _decode_surface(self, surf, out=None):
        return vops.preprocess(surf, out=out, dtype=self.dtype)

    def source_fps_of(self, vid: int) -> Optional[Tuple[int, int]]:
        """Frame rate of a probed video as ``(n, d)``, or ``None`` if unknown."""
        return self.source_fps

    def decode(self, vid: int, starts: Sequence[int], out: Optional[torch.Tensor] = None,
               step=(1, 1)) -> torch.Tensor:
        """Clips of ``clip_frames(start, F, step)`` for every start."""
        raise NotImplementedError


class SyntheticDecoder(Decoder):
    """Synthetic video source on the GPU.

    ``source="nv12"`` (default): per video, the sampled frames are produced as
    NV12 decoder surfaces at the source resolution (340x256, as Kinetics is
    stored; ``nv12gen``) and then go through the same per-frame work NVVL
    does after NVDEC: bilinear scaling to 112x112, BT.601 YUV -> RGB,
    normalisation, written straight into the output (slot) layout
    (``nv12_to_clip``). ``source="rgb"``: 112x112 RGB frames directly
    (``clipgen`` + ``preprocess``; the round-1 loader)."""

    def __init__(self, device: torch.device, clip_length: int = 8, height: int = 112,
                 width: int = 112, dtype=torch.bfloat16, source: str = "nv12",
                 src_width: int = vops.SOURCE_W, src_height: int = vops.SOURCE_H,
                 source_fps=None):
        if source not in ("nv12", "rgb"):
            raise ValueError("unknown synthetic source %r" % (source,))
        self.source_fps = _rate_pair(source_fps, "SyntheticDecoder")
        self.device = device
        self.F, self.H, self.W = clip_length, height, width
        self.dtype = dtype
        self.source = source
        self.src_w, self.src_h = src_width, src_height
        self._surface = None

    def probe(self, path):
        return parse_synthetic_path(path)

    def decode(self, vid, starts, out=None, step=(1, 1)):
        n = len(starts)
        if n == 0:
            return self.empty()
        if self.source == "nv12":
            return self._decode_nv12(vid, starts, out, step)
        surf = None
        if self.device.type == "cuda":
            # one reusable decoder surface: uses of it are ordered on the stream
            if self._surface is None or self._surface.shape[0] < n:
                self._surface = torch.empty((max(n, 15), self.F, self.H, self.W, 3),
                                            dtype=torch.uint8, device=self.device)
            surf = self._surface[:n]
        surf = vops.clipgen_video(vid, starts, self.F, self.H, self.W, self.device, out=surf,
                                  step=step)
        return vops.preprocess(surf, out=out, dtype=self.dtype)

    def warmup(self, n: int) -> None:
        for i in range(n):
            self.decode(i, [0])

    def _decode_nv12(self, vid, starts, out, step=(1, 1)):
        n = len(starts)
        surf = None
        if self.device.type == "cuda":
            rows = self.src_h * 3 // 2
            if self._surface is None or self._surface.shape[0] < n * self.F:
                self._surface = torch.empty((max(n, 15) * self.F, rows, self.src_w),
                                            dtype=torch.uint8, device=self.device)
            surf = self._surface[:n * self.F]
        surf = vops.nv12gen(int(vid), list(starts), self.F, self.src_h, self.src_w,
                            self.device, out=surf, step=step)
        if out is None:
            out = torch.empty((n, self.F, self.H, self.W, vops.clip_channels(self.dtype)),
                              dtype=self.dtype, device=self.device)
        vops.nv12_to_clip(surf, self.src_w, self.src_h, self.W, self.H, dtype=self.dtype,
                          out=out)
        return out


class NpyDecoder(Decoder):
    """Pre-decoded ``.npy`` videos (uint8 [frames, H, W, 3])."""

    def __init__(self, device: torch.device, clip_length: int = 8, height: int = 112,
                 width: int = 112, dtype=torch.bfloat16, source_fps=None):
        self.device = device
        self.F, self.H, self.W = clip_length, height, width
        self.dtype = dtype
        self.source_fps = _rate_pair(source_fps, "NpyDecoder")
        self._ids = {}
        self._paths = {}           # video id -> path
        self._arrays = {}          # video id -> memory-mapped frames

    def probe(self, path):
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
        if arr.ndim != 4 or arr.shape[1:] != (self.H, self.W, 3) or arr.dtype != np.uint8:
            raise ValueError("%s: expected uint8 [F, %d, %d, 3], got %s %s"
                             % (path, self.H, self.W, arr.dtype, arr.shape))
        vid = self._ids.setdefault(path, len(self._ids))
        self._paths[vid] = path
        self._arrays[vid] = arr
        return vid, arr.shape[0]

    def decode(self, vid, starts, out=None, step=(1, 1)):
        if len(starts) == 0:
            return self.empty()
        arr = self._arrays.get(vid)
        if arr is None:
            raise KeyError("video id %r was not probed" % (vid,))
        if tuple(step) == (1, 1):
            clips = np.stack([np.asarray(arr[s:s + self.F]) for s in starts])
        else:
            span = clip_span(self.F, step)
            for s in starts:
                if s < 0 or s + span > arr.shape[0]:
                    raise ValueError("%s: clip at frame %d (span %d at step %d/%d) is outside "
                                     "the %d frames" % (self._paths[vid], s, span, step[0],
                                                        step[1], arr.shape[0]))
            clips = np.stack([np.asarray(arr[clip_frames(s, self.F, step)]) for s in starts])
        t = torch.from_numpy(clips)
        if self.device.type == "cuda":
            t = t.pin_memory().to(self.device, non_blocking=True)
        return self._decode_surface(t, out)


class _UploadEntry:
    """One request's staging: pinned host bytes, their device copy, and the
    event recorded behind the kernel that reads the device copy."""

    def __init__(self, nbytes: int, device: torch.device):
        self.pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.host = self.pinned.numpy()
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.event = torch.cuda.Event()
        self.in_flight = False
        self.pending = None      # MjpegDecoder(entropy="gpu"): status words not yet looked at

    def acquire(self) -> None:
        """The copies and the kernel of this entry's last request are done."""
        if self.in_flight:
            self.event.synchronize()
            self.in_flight = False


def _f32_towards(x: float, up: bool) -> float:
    """The nearest fp32 value that is >= ``x`` (``up``) or <= ``x``."""
    f = np.float32(x)
    if (float(f) < x) if up else (float(f) > x):
        f = np.nextafter(f, np.float32(np.inf if up else -np.inf))
    return float(f)


def view_boxes(W: int, H: int, out_w: int, out_h: int, short_side: float, views: int):
    """The crop boxes (x, y, w, h) of ``views`` windows of a ``W`` x ``H`` frame
    resized so that its short side is ``short_side``, each ``out_w`` x ``out_h``
    after the resize; ``None`` if such a window is larger than the frame.

    In source pixels a window is ``out * min(W, H) / short_side`` per axis. One
    view is centred. Three lie along the axis with the larger free length (a tie
    goes to x) at 0, 1/2 and 1 of it -- left / centre / right or top / centre /
    bottom -- and are centred along the other. Every number is rounded to fp32
    towards the interior of the box, so that the box the kernel gets (fp32) lies
    inside the frame by the antialias launcher's own test (``x + w`` summed in
    double against ``W``) whenever the exact box does."""
    m = min(W, H)
    bw, bh = out_w * m / short_side, out_h * m / short_side
    if bw > W or bh > H:
        return None
    fx, fy = W - bw, H - bh
    if views == 1:
        at = [(fx / 2.0, fy / 2.0)]
    elif fx >= fy:
        at = [(t * fx, fy / 2.0) for t in (0.0, 0.5, 1.0)]
    else:
        at = [(fx / 2.0, t * fy) for t in (0.0, 0.5, 1.0)]

    def axis(lo, size, n):
        lo32 = _f32_towards(max(lo, 0.0), True)
        size32 = _f32_towards(min(lo + size, float(n)) - lo32, False)
        while lo32 + size32 > n:              # two fp32 values: their double sum is exact
            size32 = float(np.nextafter(np.float32(size32), np.float32(-np.inf)))
        return lo32, size32
    boxes = []
    for x, y in at:
        (x32, w32), (y32, h32) = axis(x, bw, W), axis(y, bh, H)
        boxes.append((x32, y32, w32, h32))
    return boxes


class _StagedFileDecoder(Decoder):
    """What the file-backed decoders that upload bytes share: an LRU of memory
    maps, a ring of ``depth`` pinned staging / device upload buffers
    (``_UploadEntry``) ordered by HIP events, and the crop geometry.

    ``crop``: ``"full"`` scales the whole frame to the output, ``"center"`` the
    centred square of the short side. ``{"short_side": S, "views": V}`` is the
    evaluation protocol of the R(2+1)D family: the frame is resized, aspect
    kept, so that its short side is ``S`` (a positive number) and ``V`` windows
    of the output size are taken from it, 1 (default; centred) or 3 (along the
    long side: ``view_boxes``). ``decode`` then returns ``views`` = ``V`` rows
    per clip, the views of a clip adjacent. All views of a clip read one staged
    and uploaded span, in one launch (``yuv420_to_clip`` with a box per row). A
    file whose frames are smaller than the window is refused at ``probe``."""

    WARMUP_W, WARMUP_H = vops.SOURCE_W, vops.SOURCE_H
    MAX_OPEN = 64            # memory maps kept open (least recently used first out)

    def __init__(self, device: torch.device, clip_length: int = 8, height: int = 112,
                 width: int = 112, dtype=torch.bfloat16, depth: int = 4, crop: str = "full",
                 filter: str = "bilinear", source_fps=None):
        name = type(self).__name__
        self.source_fps = _rate_pair(source_fps, name)
        self.views, self.short_side = 1, None
        if isinstance(crop, dict):
            unknown = sorted(set(crop) - {"short_side", "views"})
            if unknown or "short_side" not in crop:
                raise ValueError("%s: crop takes the keys 'short_side' and 'views', got %r"
                                 % (name, sorted(crop)))
            side, views = crop["short_side"], crop.get("views", 1)
            if isinstance(side, bool) or not isinstance(side, numbers.Real) \
                    or not (side > 0 and math.isfinite(side)):
                raise ValueError("%s: crop 'short_side' must be a positive number, got %r"
                                 % (name, side))
            if isinstance(views, bool) or views not in (1, 3):
                raise ValueError("%s: crop 'views' must be 1 or 3, got %r" % (name, views))
            self.views, self.short_side = int(views), float(side)
            crop = {"short_side": side, "views": int(views)}
        elif crop not in ("full", "center"):
            raise ValueError("%s: crop must be 'full', 'center' or {'short_side': S, "
                             "'views': 1 or 3}, got %r" % (name, crop))
        if filter not in vops.FILTERS:
            raise ValueError("%s: filter must be one of %s, got %r"
                             % (name, vops.FILTERS, filter))
        if depth < 1:
            raise ValueError("%s: ring depth must be >= 1, got %r" % (name, depth))
        self.device = device
        self.F, self.H, self.W = clip_length, height, width
        self.dtype = dtype
        self.depth = int(depth)
        self.crop = crop
        self.filter = filter
        self._ids = {}
        self._videos = {}          # video id -> (path, header / index)
        self._boxes = {}           # video id -> view boxes (crop={"short_side": ...})
        self._maps = OrderedDict()  # video id -> (mmap, uint8 view), LRU
        self._ring: List[_UploadEntry] = []
        self._ring_bytes = 0
        self._next = 0

    # -- files ------------------------------------------------------------
    EMPTY_FIELD = None       # the field an empty file is reported under

    def _parse(self, path: str, mm, data):
        """Header / index of the file just mapped (``mm``: the map, ``data``: its
        uint8 view); ``ValueError`` naming file and field for what is not read."""
        raise NotImplementedError

    def probe(self, path):
        vid = self._ids.get(path)
        if vid is not None:
            return vid, self._videos[vid][1].num_frames
        if os.path.getsize(path) == 0:
            raise ValueError("%s: empty file (field %r)" % (path, self.EMPTY_FIELD))
        vid = len(self._ids)
        mm, data = self._map(vid, path)
        try:
            hdr = self._parse(path, mm, data)
            boxes = self._probe_boxes(path, hdr)
        except ValueError:
            del self._maps[vid]
            raise
        self._ids[path] = vid
        self._videos[vid] = (path, hdr)
        self._boxes[vid] = boxes
        return vid, hdr.num_frames

    def _check_starts(self, path: str, starts, num_frames: int, step=(1, 1)) -> None:
        span = clip_span(self.F, step)
        for s in starts:
            if s < 0 or s + span > num_frames:
                raise ValueError("%s: clip at frame %d (span %d at step %d/%d) is outside the "
                                 "%d frames" % (path, s, span, step[0], step[1], num_frames))

    def _map(self, vid: int, path: str):
        got = self._maps.get(vid)
        if got is not None:
            self._maps.move_to_end(vid)
            return got
        with open(path, "rb") as fp:
            mm = mmap.mmap(fp.fileno(), 0, access=mmap.ACCESS_READ)
        got = (mm, np.frombuffer(mm, dtype=np.uint8))
        self._maps[vid] = got
        while len(self._maps) > self.MAX_OPEN:
            self._maps.popitem(last=False)       # unmapped once its views are gone
        return got

    def _crop_box(self, hdr):
        if self.crop == "full":
            return None
        side = min(hdr.width, hdr.height)
        return ((hdr.width - side) / 2.0, (hdr.height - side) / 2.0, float(side), float(side))

    def _probe_boxes(self, path: str, hdr):
        """The view boxes of a file just probed (``None`` for the string crops);
        ``ValueError`` naming file and field if the window does not fit."""
        if self.short_side is None:
            return None
        boxes = view_boxes(hdr.width, hdr.height, self.W, self.H, self.short_side, self.views)
        if boxes is None:
            m = min(hdr.width, hdr.height)
            raise ValueError("%s: a %d x %d frame resized to short side %g is smaller than the "
                             "%d x %d window (field 'crop': short_side must be >= %g)"
                             % (path, hdr.width, hdr.height, self.short_side, self.W, self.H,
                                max(self.W * m / hdr.width, self.H * m / hdr.height)))
        return boxes

    def _rows(self, starts, views):
        """``(clips, rows)`` of a request: the start frames to stage, each once,
        and per output row (index into ``clips``, view). ``views=None``: every
        view of every entry of ``starts``, clip-major. Else one view index per
        entry of ``starts``: exactly those rows, equal starts sharing a clip."""
        if views is None:
            return list(starts), [(i, v) for i in range(len(starts)) for v in range(self.views)]
        views = [int(v) for v in views]
        if len(views) != len(starts):
            raise ValueError("%s: %d view indices for %d clip starts"
                             % (type(self).__name__, len(views), len(starts)))
        if any(not 0 <= v < self.views for v in views):
            raise ValueError("%s: view indices must be in 0..%d, got %r"
                             % (type(self).__name__, self.views - 1, views))
        clips, index, rows = [], {}, []
        for s, v in zip(starts, views):
            if s not in index:
                index[s] = len(clips)
                clips.append(s)
            rows.append((index[s], v))
        return clips, rows

    def _clip_args(self, vid, hdr, rows, span: int):
        """``yuv420_to_clip``'s (offsets, crop) for the output rows, clip ``c``
        staged at byte ``c * span``: one box for every row, or a box per row."""
        offsets = [c * span for c, _ in rows]
        boxes = self._boxes.get(vid)
        if boxes is None:
            return offsets, self._crop_box(hdr)
        if self.views == 1:
            return offsets, boxes[0]
        return offsets, [boxes[v] for _, v in rows]

    def _warm_crop(self, W: int, H: int):
        """(offsets, crop) of a warm-up launch: the kernel form a request runs."""
        if self.views == 1:
            return [0], None
        return [0] * self.views, [(0.0, 0.0, float(W), float(H))] * self.views

    # -- ring ---------------------------------------------------------------
    def _entry(self, nbytes: int) -> _UploadEntry:
        if nbytes > self._ring_bytes or not self._ring:
            for e in self._ring:
                e.acquire()                      # nothing in flight reads the old buffers
            self._ring_bytes = max(nbytes, self._ring_bytes)
            self._ring = [_UploadEntry(self._ring_bytes, self.device)
                          for _ in range(self.depth)]
            self._next = 0
        e = self._ring[self._next]
        self._next = (self._next + 1) % self.depth
        e.acquire()
        return e

    @contextlib.contextmanager
    def _staged(self, nbytes: int, cpu_nbytes: Optional[int] = None):
        """``(entry, host, buf)`` for a request: on a CUDA device a ring entry of
        ``nbytes`` (the ring's size for such requests), its pinned bytes and its
        device copy; on a CPU device ``None``, a fresh buffer of ``cpu_nbytes``
        (the request's own size; default ``nbytes``) and its tensor view. On exit
        the entry's event is recorded, also behind the uploads and kernels of a
        request that raised."""
        if self.device.type != "cuda":
            host = np.empty(nbytes if cpu_nbytes is None else cpu_nbytes, dtype=np.uint8)
            yield None, host, torch.from_numpy(host)
            return
        entry = self._entry(nbytes)
        try:
            yield entry, entry.host, entry.dev
        finally:
            entry.event.record(torch.cuda.current_stream(self.device))
            entry.in_flight = True

    def _out(self, n: int, out):
        if out is not None:
            return out
        return torch.empty((n, self.F, self.H, self.W, vops.clip_channels(self.dtype)),
                           dtype=self.dtype, device=self.device)


class Y4mDecoder(_StagedFileDecoder):
    """Raw YUV4MPEG2 (``.y4m``) videos at their source resolution.

    ``probe`` memory-maps the file and parses its header (``utils/y4m.py``):
    8-bit 4:2:0 (no ``C`` field or ``C420`` / ``C420jpeg`` / ``C420mpeg2`` /
    ``C420paldv``), 4:2:2 (``C422``) and 4:4:4 (``C444``); the header's sampling
    sizes the spans and goes down to the clip kernel, so one decoder serves
    files of all three. The 4:2:0 tags differ in chroma siting; all are
    sampled with the kernel's centred siting (chroma sample centres at 2x + 0.5
    luma pixels, exact for ``C420jpeg``; the co-sited variants are read half a
    luma pixel off horizontally, as NVVL's scaler does not distinguish them
    either). Everything else raises ``ValueError`` naming file and field.

    ``decode`` treats each clip's F consecutive frames as one contiguous span
    of the file: it copies the span into a pinned staging buffer, checks the
    ``FRAME`` marker of every frame, issues one asynchronous upload per clip
    and then one ``yuv420_to_clip`` launch (scale, BT.601, normalise) straight
    into ``out``. Staging and upload buffers form a ring of ``depth`` requests
    owned by the decoder, sized on first use for ``max(n, 15)`` clips and
    regrown for larger frames; an entry is reused once the event recorded
    behind its kernel has completed (waited for if not), so a warm decoder
    neither pins nor allocates. On a CPU device the spans go to the op's CPU
    mirror.

    ``crop``: ``"full"`` scales the whole frame to the output (what the
    synthetic NV12 path does), ``"center"`` the centred square of the short
    side, ``{"short_side": S, "views": V}`` one or three windows of the frame
    resized to short side ``S`` (``_StagedFileDecoder``); ``decode`` then
    returns ``V`` rows per clip, or with ``views=[...]`` (one view index per
    entry of ``starts``) exactly those rows, every distinct clip staged and
    uploaded once. ``filter``: ``"bilinear"`` (two taps per axis, the default) or
    ``"antialias"``, the triangle filter widened by the downscale factor that
    PIL's ``resize(BILINEAR)`` and torchvision's ``Resize(antialias=True)``
    apply (``yuv420_to_clip(filter=)``); both boxes lie inside the frame.

    With a ``step`` other than ``(1, 1)`` a clip is no contiguous span: its F
    selected frames (``clip_frames``) are copied one by one into the clip's
    staging slot, packed ``frame_stride`` apart, each one's marker checked; the
    upload per clip, its ``F * frame_stride`` bytes and the launch are the same."""

    _PLANES = {"420": vops.i420_planes, "422": vops.i422_planes, "444": vops.i444_planes}

    EMPTY_FIELD = "magic"

    def _parse(self, path, mm, data):
        return y4m.read_header(path, data=mm)

    def source_fps_of(self, vid):
        """The header's ``F`` field; the ``source_fps`` argument where the
        header has none (``F0:0`` or no ``F`` field)."""
        n, d = self._videos[vid][1].fps
        return (n, d) if n > 0 and d > 0 else self.source_fps

    def warmup(self, n: int) -> None:
        """Run the clip kernel on a zeroed upload buffer (no file needed)."""
        if self.device.type != "cuda":
            return
        W, H = self.WARMUP_W, self.WARMUP_H
        stride = len(y4m.FRAME_MARKER) + vops.nv12_frame_bytes(W, H)
        offsets, crop = self._warm_crop(W, H)
        for i in range(n):
            with self._staged(15 * self.F * stride) as (_, _, buf):
                buf[:self.F * stride].zero_()
                vops.yuv420_to_clip(buf, offsets, self.F, W, H, stride,
                                    vops.i420_planes(W, H, len(y4m.FRAME_MARKER)), self.W,
                                    self.H, crop=crop, dtype=self.dtype,
                                    out=self._out(len(offsets), None), filter=self.filter)

    # -- decode ---------------------------------------------------------------
    def decode(self, vid, starts, out=None, views=None, step=(1, 1)):
        if len(starts) == 0:
            return self.empty()
        got = self._videos.get(vid)
        if got is None:
            raise KeyError("video id %r was not probed" % (vid,))
        starts, rows = self._rows(starts, views)
        n = len(starts)
        stepped = tuple(step) != (1, 1)
        path, hdr = got
        _, data = self._map(vid, path)
        span = self.F * hdr.frame_stride
        marker = np.frombuffer(y4m.FRAME_MARKER, dtype=np.uint8)
        self._check_starts(path, starts, hdr.num_frames, step)
        planes = self._PLANES[hdr.sampling](hdr.width, hdr.height, len(y4m.FRAME_MARKER))
        offsets, crop = self._clip_args(vid, hdr, rows, span)
        with self._staged(max(n, 15) * span, n * span) as (entry, host, buf):
            for i, s in enumerate(starts):
                dst = host[i * span:(i + 1) * span]
                frames = dst.reshape(self.F, hdr.frame_stride)
                if stepped:
                    src = clip_frames(s, self.F, step)
                    for f, fr in enumerate(src):
                        a = hdr.frame_offset(fr)
                        np.copyto(frames[f], data[a:a + hdr.frame_stride])
                else:
                    a = hdr.frame_offset(s)
                    np.copyto(dst, data[a:a + span])
                heads = frames[:, :len(marker)]
                if not (heads == marker).all():
                    bad = int(np.nonzero((heads != marker).any(axis=1))[0][0])
                    raise ValueError("%s: frame %d does not start with a bare FRAME marker "
                                     "(field 'FRAME': %r); frame parameters are not supported"
                                     % (path, src[bad] if stepped else s + bad,
                                        bytes(heads[bad])))
                if entry is not None:     # this clip uploads while the next one is staged
                    buf[i * span:(i + 1) * span].copy_(
                        entry.pinned[i * span:(i + 1) * span], non_blocking=True)
            out = self._out(len(rows), out)
            vops.yuv420_to_clip(buf[:n * span], offsets, self.F, hdr.width, hdr.height,
                                hdr.frame_stride, planes, self.W, self.H,
                                crop=crop, dtype=self.dtype, out=out,
                                filter=self.filter, sampling=hdr.sampling)
        return out


class MjpegDecoder(_StagedFileDecoder):
    """Motion-JPEG streams (``.mjpeg`` / ``.mjpg``: JPEG frames back to back)
    at their source resolution, split the way a hardware decoder splits it:
    the serial entropy decode on the host, the per-sample arithmetic on the GPU.

    ``probe`` memory-maps the file and indexes it (``utils/mjpeg.py``,
    ``rnb_mjpeg_index_s``): baseline sequential Huffman JPEG, 8-bit, 4:2:0,
    4:2:2 or 4:4:4, one scan, all frames of one size and sampling; anything else
    raises ``ValueError`` naming file, frame and field. AVI / MOV containers,
    progressive JPEG, 4:4:0, 4:1:1 and grayscale are not read. The index's
    sampling sizes every buffer of a request and goes down to each kernel, so
    one decoder serves files of all three.

    ``decode`` entropy-decodes each clip's F frames (``librnb_jpeg.so``, on
    ``threads`` host threads with the GIL released) straight into a pinned
    staging entry as frame records of quantised coefficients, and uploads a
    clip while the next one decodes. One ``jpeg_idct`` launch turns the records
    into 8-bit I420 planes in a device surface the decoder owns, and one
    ``yuv420_to_clip(matrix="jfif")`` launch scales, converts (full-range JFIF
    YCbCr) and normalises them straight into ``out``; the frame's true size goes
    to that kernel, so the MCU padding is never sampled. The staging ring and
    its event discipline are ``Y4mDecoder``'s. On a CPU device the records go
    to the ops' CPU mirrors.

    ``crop`` and ``filter`` as for ``Y4mDecoder`` (with views, every frame is
    entropy-decoded and IDCT'd once per request); ``threads``: 1-16 entropy-decode
    threads.

    ``entropy="gpu"`` (opt-in; ``"host"`` is the path above) moves the Huffman
    decode to the GPU. ``decode`` then only *packs* each clip's scans on the
    host (``mjpeg.pack_scans``: header parse and restart markers, no Huffman
    work) into the pinned entry, which is sized from the frames' byte lengths,
    and uploads a clip while the next one packs: the entropy-coded bytes cross
    the bus, not the coefficients. One ``jpeg_huff`` launch (one workgroup per
    frame, one lane per restart interval, the host decoder's loop) writes the
    frame records into a device buffer the decoder owns, and ``jpeg_idct`` and
    ``yuv420_to_clip`` follow as above. What the packer refuses still raises
    from ``decode``. What only the Huffman decode can find (a bad code, a run
    past 63, an interval that does not end at its marker, ...) is *deferred*:
    the kernel's per-frame status words are copied back asynchronously into
    the entry's pinned memory and checked when that entry is next acquired
    (after its event) and in ``drain()``; either raises ``JpegError`` naming
    the file, the frame and the field of the request that failed. Until then
    the pixels of a corrupt frame (of its failing restart intervals) are grey:
    zero coefficients. On a CPU device the same decode loop runs on the host
    and such a frame raises from ``decode``.

    ``subseq_bytes`` (only with ``entropy="gpu"``; default ``SUBSEQ_BYTES``):
    above 0, a multiple of 16 in 16..4096, the launch is
    ``jpeg_huff_subseq_kernel``, which cuts the scan of a frame WITHOUT restart
    markers into subsequences of that many bytes and decodes them on the lanes
    of the frame's workgroup, synchronising their entry states
    (``csrc/jpeg_huff.h``); records, status words and deferred errors are the
    same. 0: one lane per restart interval, i.e. per frame of such a stream.

    ``reduce``: ``1`` (default), ``2``, ``4``, ``8`` or ``"auto"``: the
    reduced-size decode of libjpeg's ``scale_denom`` / PIL's ``draft``, in every
    entropy mode and on a CPU device. ``jpeg_idct(reduce=s)`` writes the frame
    at ``ceil(W / s) x ceil(H / s)``, each sample the ``s x s`` box mean of the
    unrounded full-size samples, into a surface ``s^2`` times smaller, and the
    clip launch gets that frame size, the reduced planes and every crop box
    divided by ``s`` (exact: a power of two), ``crop="full"`` as the explicit
    box ``(0, 0, W / s, H / s)`` so that the MCU padding in the last reduced
    column is not sampled. Records, Huffman decode and status handling are
    untouched. ``"auto"`` is decided per file at ``probe`` by geometry alone
    (``auto_reduce``): the largest ``s`` at which no crop box of the file,
    divided by ``s``, is smaller than the output, so the reduced frame is never
    upscaled (340x256 to 112x112: 2 in every crop mode; a 1280x720 centre
    crop: 4). ``reduce_of(vid)`` is the value a probed file decodes with.

    ``stats``: ``requests`` served and ``uploaded_bytes`` staged for upload
    (records, or scan records and their offset table)."""

    SUBSEQ_BYTES = 48          # entropy="gpu" without subseq_bytes: the measured best (profiles/NOTES.md)

    def __init__(self, device: torch.device, clip_length: int = 8, height: int = 112,
                 width: int = 112, dtype=torch.bfloat16, depth: int = 4, crop: str = "full",
                 threads: int = 4, entropy: str = "host", subseq_bytes: Optional[int] = None,
                 filter: str = "bilinear", reduce=1, source_fps=None):
        if isinstance(threads, bool) or not isinstance(threads, int) or not 1 <= threads <= 16:
            raise ValueError("MjpegDecoder: threads must be an integer in 1..16, got %r"
                             % (threads,))
        if isinstance(depth, bool) or not isinstance(depth, int):
            raise ValueError("MjpegDecoder: ring depth must be an integer, got %r" % (depth,))
        if entropy not in ("host", "gpu"):
            raise ValueError("MjpegDecoder: entropy must be 'host' or 'gpu', got %r" % (entropy,))
        if subseq_bytes is not None and entropy != "gpu":
            raise ValueError("MjpegDecoder: subseq_bytes goes with entropy='gpu', not %r"
                             % (entropy,))
        if subseq_bytes is None:
            subseq_bytes = self.SUBSEQ_BYTES if entropy == "gpu" else 0
        subseq_bytes = mjpeg.check_subseq_bytes(subseq_bytes, "MjpegDecoder")
        if reduce != "auto":
            vops.jpeg_reduce_points(reduce, "MjpegDecoder")
            reduce = int(reduce)
        super().__init__(device, clip_length, height, width, dtype, depth, crop, filter,
                         source_fps)
        self.threads = threads
        self.entropy = entropy
        self.subseq_bytes = subseq_bytes
        self.reduce = reduce
        self._reduce = {}          # video id -> the reduce its frames decode with
        self.stats = {"requests": 0, "uploaded_bytes": 0}
        self._surface = None       # device I420 planes of the request being decoded
        self._records = None       # entropy="gpu": device frame records of that request
        self._status = None        # ... and the kernel's per-frame status words
        self._rounds = None        # ... and, with subseq_bytes, its rounds per frame
        self._max_len = {}         # video id -> longest frame in bytes

    EMPTY_FIELD = "SOI"

    def _parse(self, path, mm, data):
        return mjpeg.read_index(path, data=data)

    def _planes(self, nframes: int, frame_bytes: int) -> torch.Tensor:
        # one surface, reused: its uses are ordered on the stream
        need = nframes * frame_bytes
        if self._surface is None or self._surface.numel() < need:
            self._surface = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._surface

    def auto_reduce(self, W: int, H: int, boxes=None) -> int:
        """The ``reduce`` of ``"auto"`` for ``W`` x ``H`` frames: the largest s in
        8, 4, 2, 1 with ``box_w / s >= out_w`` and ``box_h / s >= out_h`` for
        every crop box of such a file (``boxes``: its view boxes; without them
        the whole frame for ``crop="full"``, the square of the short side for
        ``"center"``, the windows of ``view_boxes`` for a short side)."""
        if boxes is None and self.short_side is not None:
            boxes = view_boxes(W, H, self.W, self.H, self.short_side, self.views)
        if boxes is None:
            side = min(W, H)
            boxes = [(0.0, 0.0, float(W), float(H)) if self.crop == "full"
                     else (0.0, 0.0, float(side), float(side))]
        for s in (8, 4, 2):
            if all(b[2] / s >= self.W and b[3] / s >= self.H for b in boxes):
                return s
        return 1

    def reduce_of(self, vid: int) -> int:
        """The reduce the frames of a probed file decode with."""
        return self._reduce[vid]

    def probe(self, path):
        vid, num_frames = super().probe(path)
        if vid not in self._reduce:
            hdr = self._videos[vid][1]
            self._reduce[vid] = self.reduce if self.reduce != "auto" else \
                self.auto_reduce(hdr.width, hdr.height, self._boxes[vid])
        return vid, num_frames

    def _clip_args(self, vid, hdr, rows, span: int, reduce: int = 1):
        """As ``_StagedFileDecoder._clip_args``, for frames decoded at 1 /
        ``reduce``: every box divided by it, the whole frame as the explicit
        box (0, 0, W / reduce, H / reduce)."""
        offsets, crop = super()._clip_args(vid, hdr, rows, span)
        if reduce == 1:
            return offsets, crop
        if crop is None:
            return offsets, (0.0, 0.0, hdr.width / reduce, hdr.height / reduce)
        if isinstance(crop, tuple):
            return offsets, tuple(c / reduce for c in crop)
        return offsets, [tuple(c / reduce for c in box) for box in crop]

    def _to_clips(self, records, n, W, H, mw, mh, clip_args, out, sampling="420", reduce=1):
        """``n`` clips of frame records -> one IDCT over all of them, then one clip
        launch over the output rows; ``clip_args(span)``: (offsets, crop) of the
        rows for clips ``span`` surface bytes apart, in the coordinates of the
        frame at 1 / ``reduce``."""
        fbytes = vops.jpeg_frame_bytes(mw, mh, sampling, reduce)[1]
        surf = vops.jpeg_idct(records, n * self.F, mw, mh,
                              out=self._planes(max(n, 15) * self.F, fbytes)
                              if self.device.type == "cuda" else None, sampling=sampling,
                              reduce=reduce)
        offsets, crop = clip_args(self.F * fbytes)
        return vops.yuv420_to_clip(surf, offsets, self.F, -(-W // reduce), -(-H // reduce),
                                   fbytes, vops.jpeg_surface_planes(mw, mh, sampling, reduce),
                                   self.W, self.H, crop=crop, dtype=self.dtype, out=out,
                                   matrix="jfif", filter=self.filter, sampling=sampling)

    def warmup(self, n: int) -> None:
        """Run both kernels on a zeroed record buffer (no file needed), at the
        reduce in use (``"auto"``: the one the warm-up frame size resolves to)."""
        if self.device.type != "cuda":
            return
        W, H = self.WARMUP_W, self.WARMUP_H
        mw, mh, rb = mjpeg.geometry(W, H)
        s = self.reduce if self.reduce != "auto" else self.auto_reduce(W, H)
        for i in range(n):
            with self._staged(15 * self.F * rb) as (_, _, buf):
                buf[:self.F * rb].zero_()
                self._to_clips(buf[:self.F * rb], 1, W, H, mw, mh,
                               lambda span: self._warm_crop(W / s, H / s),
                               self._out(max(1, self.views), None), reduce=s)

    def _clip_index(self, idx, s: int, step):
        """(offsets, lengths, source frames) of the clip at ``s``: slices of the
        index for consecutive frames, else gathered by ``clip_frames`` (a
        repeated frame is listed, and decoded, again)."""
        if tuple(step) == (1, 1):
            return idx.offsets[s:s + self.F], idx.lengths[s:s + self.F], None
        src = clip_frames(s, self.F, step)
        return (np.ascontiguousarray(idx.offsets[src]), np.ascontiguousarray(idx.lengths[src]),
                src)

    def decode(self, vid, starts, out=None, views=None, step=(1, 1)):
        if len(starts) == 0:
            return self.empty()
        got = self._videos.get(vid)
        if got is None:
            raise KeyError("video id %r was not probed" % (vid,))
        starts, rows = self._rows(starts, views)
        n = len(starts)
        path, idx = got
        _, data = self._map(vid, path)
        self._check_starts(path, starts, idx.num_frames, step)
        self.stats["requests"] += 1
        if self.entropy == "gpu":
            return self._decode_gpu_entropy(vid, path, idx, data, starts, out, rows, step)
        span = self.F * idx.record_bytes
        self.stats["uploaded_bytes"] += n * span
        with self._staged(max(n, 15) * span, n * span) as (entry, host, buf):
            for i, s in enumerate(starts):
                offsets, lengths, _ = self._clip_index(idx, s, step)
                mjpeg.entropy_decode(data, offsets, lengths,
                                     host[i * span:(i + 1) * span], idx.record_bytes,
                                     self.threads, name=path, sampling=idx.sampling)
                if entry is not None:     # this clip uploads while the next one decodes
                    buf[i * span:(i + 1) * span].copy_(
                        entry.pinned[i * span:(i + 1) * span], non_blocking=True)
            out = self._out(len(rows), out)
            red = self._reduce[vid]
            self._to_clips(buf[:n * span], n, idx.width, idx.height, idx.mw, idx.mh,
                           lambda sp: self._clip_args(vid, idx, rows, sp, red), out,
                           idx.sampling, red)
        return out

    # -- entropy="gpu" ----------------------------------------------------------
    def _check_entry(self, e: _UploadEntry) -> None:
        """Look at the status words of the entry's last request (its event has
        completed); raises for the first frame that failed."""
        pending, e.pending = e.pending, None
        if pending is not None:
            path, frames, at = pending
            status = e.host[at:at + 4 * len(frames)].view(np.int32)
            mjpeg.raise_for_status(status, path, frames)

    def _entry(self, nbytes: int) -> _UploadEntry:
        if self._ring and nbytes > self._ring_bytes:
            self.drain()                         # the ring is replaced: look at it first
        e = super()._entry(nbytes)
        self._check_entry(e)
        return e

    def drain(self) -> None:
        """Wait for every request in flight and raise ``JpegError`` for the
        oldest one whose Huffman decode failed on the GPU (``entropy="gpu"``),
        naming its file, frame and field. All deferred errors are cleared."""
        first = None
        for k in range(len(self._ring)):
            e = self._ring[(self._next + k) % len(self._ring)]      # oldest first
            e.acquire()
            try:
                self._check_entry(e)
            except mjpeg.JpegError as err:
                first = first or err
        if first is not None:
            raise first

    def _device_buffer(self, name: str, numel: int, dtype) -> torch.Tensor:
        # reused like _surface: its uses are ordered on the stream
        buf = getattr(self, name)
        if buf is None or buf.numel() < numel:
            buf = torch.empty(numel, dtype=dtype, device=self.device)
            setattr(self, name, buf)
        return buf

    def _decode_gpu_entropy(self, vid, path, idx, data, starts, out, rows, step=(1, 1)):
        n, F = len(starts), self.F
        nfr = n * F
        longest = self._max_len.get(vid)
        if longest is None:
            longest = self._max_len[vid] = int(idx.lengths.max())
        per = mjpeg.scan_record_bound(idx.mw, idx.mh, longest)
        cap = max(n, 15) * F                                  # frames the entry is sized for
        head = (8 * (cap + 1) + 15) & ~15                     # the offset table, then the records
        stat_at = head + cap * per                            # then the status words come back
        frames = [fr for s in starts for fr in clip_frames(s, F, step)]
        with self._staged(stat_at + 4 * cap, stat_at) as (entry, host, buf):
            offs = host[:8 * (nfr + 1)].view(np.int64)
            pos = head
            for i, s in enumerate(starts):
                offsets, lengths, src = self._clip_index(idx, s, step)
                got, rel = mjpeg.pack_scans(data, offsets, lengths,
                                            host[pos:stat_at], idx.width, idx.height,
                                            name=path, frame0=s, sampling=idx.sampling,
                                            frames=src)
                offs[i * F:(i + 1) * F] = rel[:F] + pos
                if entry is not None:     # this clip uploads while the next one packs
                    buf[pos:pos + got].copy_(entry.pinned[pos:pos + got], non_blocking=True)
                pos += got
            offs[nfr] = pos
            self.stats["uploaded_bytes"] += pos - head + 8 * (nfr + 1)
            rb = idx.record_bytes
            if entry is not None:
                buf[:8 * (nfr + 1)].copy_(entry.pinned[:8 * (nfr + 1)], non_blocking=True)
                records, status = vops.jpeg_huff(
                    buf[:pos], offs, nfr, idx.mw, idx.mh,
                    out=self._device_buffer("_records", cap * rb, torch.uint8),
                    status=self._device_buffer("_status", cap, torch.int32),
                    offs_dev=buf[:8 * (nfr + 1)].view(torch.int64),
                    subseq_bytes=self.subseq_bytes,
                    rounds=self._device_buffer("_rounds", cap, torch.int32)
                    if self.subseq_bytes else None, sampling=idx.sampling)
                entry.pinned[stat_at:stat_at + 4 * nfr].view(torch.int32).copy_(
                    status, non_blocking=True)
                entry.pending = (path, frames, stat_at)
            else:
                records, status = vops.jpeg_huff(buf[:pos], offs, nfr, idx.mw, idx.mh,
                                                 subseq_bytes=self.subseq_bytes,
                                                 sampling=idx.sampling)
                mjpeg.raise_for_status(status.numpy(), path, frames)
            out = self._out(len(rows), out)
            red = self._reduce[vid]
            self._to_clips(records, n, idx.width, idx.height, idx.mw, idx.mh,
                           lambda sp: self._clip_args(vid, idx, rows, sp, red), out,
                           idx.sampling, red)
        return out


def make_decoder(backend: str, device: torch.device, clip_length=8, height=112, width=112,
                 dtype=torch.bfloat16, decoder_args: Optional[dict] = None) -> Decoder:
    """``decoder_args``: backend-specific constructor arguments (``y4m``:
    ``depth``, ``crop``, ``filter``, ``source_fps``; ``mjpeg``: ``depth``,
    ``crop``, ``filter``, ``threads``, ``entropy``, ``subseq_bytes``,
    ``source_fps``, ``reduce``: 1, 2, 4, 8 or ``"auto"``, the reduced-size
    IDCT); the other backends take ``source_fps`` and ignore the rest.
    ``source_fps`` (a number or ``"n:d"``) is the frame rate of files that
    carry none, which a loader's ``fps`` needs (a Y4M header's ``F`` field
    comes first). ``crop`` is ``"full"``, ``"center"`` or
    ``{"short_side": S, "views": 1 or 3}``; with three views the decoder returns
    three rows per clip (``Decoder.views``; 1 for every other decoder)."""
    if backend == "y4m":
        return Y4mDecoder(device, clip_length, height, width, dtype, **(decoder_args or {}))
    if backend == "mjpeg":
        return MjpegDecoder(device, clip_length, height, width, dtype, **(decoder_args or {}))
    source_fps = (decoder_args or {}).get("source_fps")
    if backend in ("synthetic", "synthetic-nv12"):
        return SyntheticDecoder(device, clip_length, height, width, dtype, source="nv12",
                                source_fps=source_fps)
    if backend == "synthetic-rgb":
        return SyntheticDecoder(device, clip_length, height, width, dtype, source="rgb",
                                source_fps=source_fps)
    if backend == "npy":
        return NpyDecoder(device, clip_length, height, width, dtype, source_fps=source_fps)
    if backend in ("rocdecode", "nvvl"):
        raise RuntimeError("decoder backend %r is not available on this system "
                           "(no rocDecode/VCN library installed); use 'synthetic', "
                           "'y4m', 'mjpeg' or 'npy'" % backend)
    raise ValueError("unknown decoder backend %r" % backend)
