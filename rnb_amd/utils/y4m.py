"""YUV4MPEG2 (``.y4m``) raw video files: header parsing and a writer.

A stream is one text header line,

    YUV4MPEG2 W<w> H<h> F<n:d> [I?] [A?] [C<cs>] [X...]\\n

followed by frames of ``FRAME\\n`` + planar payload (Y, then U, then V), which
is what ``ffmpeg -pix_fmt yuv420p x.y4m`` writes (``W*H*3/2`` bytes; ``yuv422p``
gives ``C422`` frames of ``W*H*2`` bytes with ``W/2 x H`` chroma planes,
``yuv444p`` ``C444`` frames of ``W*H*3``). Only 8-bit 4:2:0, 4:2:2 and 4:4:4
are read here: every frame then has the same size, so frame
``i`` lies at ``data_offset + i * frame_stride`` and a clip of consecutive
frames is one contiguous span of the file (``Y4mDecoder`` uploads exactly
those spans).
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAGIC = b"YUV4MPEG2"
FRAME_MARKER = b"FRAME\n"
# 8-bit 4:2:0 variants; they differ only in where the chroma samples sit
COLOURSPACES_420 = ("420", "420jpeg", "420mpeg2", "420paldv")
# C field -> sampling ("420", "422", "444"); no C field means 4:2:0
COLOURSPACES = {**{c: "420" for c in COLOURSPACES_420}, "422": "422", "444": "444"}
SAMPLING_FACTORS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
MAX_HEADER = 4096


def payload_bytes(width: int, height: int, sampling: str = "420") -> int:
    """Bytes of one frame's planes: Y, then two chroma planes of
    (width / Hs) x (height / Vs)."""
    hs, vs = SAMPLING_FACTORS[sampling]
    return width * height + 2 * (width // hs) * (height // vs)


class Y4mHeader(NamedTuple):
    width: int
    height: int
    fps: Tuple[int, int]
    colourspace: str          # "" when the header has no C field (4:2:0)
    data_offset: int          # first byte after the header line
    frame_stride: int         # len(FRAME_MARKER) + frame_bytes
    num_frames: int
    sampling: str = "420"     # "420", "422" or "444", from the C field

    @property
    def frame_bytes(self) -> int:
        return payload_bytes(self.width, self.height, self.sampling)

    def frame_offset(self, i: int) -> int:
        """Byte offset of frame ``i``'s ``FRAME`` marker."""
        return self.data_offset + i * self.frame_stride


def parse_header(head: bytes, size: int, name: str = "<y4m>") -> Y4mHeader:
    """Parse the stream header from the file's first bytes ``head`` (at most
    ``MAX_HEADER`` are looked at) given the file ``size``. Raises ``ValueError``
    naming the file and the offending field for anything but 8-bit 4:2:0, 4:2:2
    or 4:4:4 with whole frames, parameterless frame markers and an even size
    along each axis whose chroma is subsampled."""
    head = bytes(head[:MAX_HEADER])
    if not head.startswith(MAGIC + b" "):
        raise ValueError("%s: not a YUV4MPEG2 stream (field 'magic')" % name)
    end = head.find(b"\n")
    if end < 0:
        raise ValueError("%s: unterminated stream header (field 'header')" % name)
    fields = {}
    for tok in head[len(MAGIC):end].decode("ascii", "replace").split():
        if tok[0] != "X":                       # comments / extensions may repeat
            fields[tok[0]] = tok[1:]
    cs = fields.get("C", "")
    if cs and cs not in COLOURSPACES:
        raise ValueError("%s: unsupported colourspace in field 'C' (C%s); only 8-bit 4:2:0, "
                         "4:2:2 and 4:4:4 (%s) are read"
                         % (name, cs, ", ".join("C" + c for c in COLOURSPACES)))
    sampling = COLOURSPACES[cs] if cs else "420"
    dims = {}
    for key, factor in zip(("W", "H"), SAMPLING_FACTORS[sampling]):
        val = fields.get(key, "")
        if not val.isdigit() or int(val) <= 0:
            raise ValueError("%s: missing or bad field '%s' (%r)" % (name, key, val))
        if factor == 2 and int(val) % 2:
            raise ValueError("%s: field '%s' is odd (%s); %s needs even sizes"
                             % (name, key, val, ":".join(sampling)))
        dims[key] = int(val)
    num, _, den = fields.get("F", "0:0").partition(":")
    if not (num.isdigit() and den.isdigit()):
        raise ValueError("%s: bad field 'F' (%r)" % (name, fields.get("F")))
    data = end + 1
    stride = len(FRAME_MARKER) + payload_bytes(dims["W"], dims["H"], sampling)
    payload = size - data
    if payload < 0 or payload % stride:
        # the usual cause besides truncation: a C field that does not describe the payload
        for other in SAMPLING_FACTORS:
            alt = len(FRAME_MARKER) + payload_bytes(dims["W"], dims["H"], other)
            if other != sampling and payload > 0 and payload % alt == 0:
                raise ValueError("%s: payload of %d bytes is not a whole number of %d-byte %s "
                                 "frames but of %d-byte %s ones (field 'C': %s does not describe "
                                 "the frames; field 'FRAME')"
                                 % (name, payload, stride, ":".join(sampling), alt,
                                    ":".join(other), "C" + cs if cs else "no C field, i.e. 4:2:0"))
        raise ValueError("%s: payload of %d bytes is not a whole number of %d-byte frames "
                         "(field 'FRAME': truncated file or frame parameters)"
                         % (name, payload, stride))
    if payload and head[data:data + len(FRAME_MARKER)] != FRAME_MARKER:
        raise ValueError("%s: first frame marker is not a bare FRAME (field 'FRAME': %r)"
                         % (name, head[data:data + 12]))
    return Y4mHeader(dims["W"], dims["H"], (int(num), int(den)), cs, data, stride,
                     payload // stride, sampling)


def read_header(path: str, data: Optional[bytes] = None) -> Y4mHeader:
    """Header of the file at ``path``; ``data`` may pass the file's contents
    (e.g. a memory map) to spare the read."""
    if data is not None:
        return parse_header(data[:MAX_HEADER], len(data), path)
    with open(path, "rb") as fp:
        head = fp.read(MAX_HEADER)
    return parse_header(head, os.path.getsize(path), path)


def write_y4m(path: str, frames_yuv420, fps: Sequence[int] = (25, 1),
              sampling: str = "420") -> None:
    """Write planar frames as a ``C420jpeg`` (``sampling="420"``), ``C422`` or
    ``C444`` stream. ``frames_yuv420`` is a sequence of ``(Y [H, W], U, V)``
    uint8 arrays with chroma planes of ``[H / Vs, W / Hs]``."""
    if sampling not in SAMPLING_FACTORS:
        raise ValueError("write_y4m: sampling must be one of %s, got %r"
                         % (tuple(SAMPLING_FACTORS), sampling))
    hs, vs = SAMPLING_FACTORS[sampling]
    frames = [tuple(np.ascontiguousarray(np.asarray(p), dtype=np.uint8) for p in f)
              for f in frames_yuv420]
    if not frames:
        raise ValueError("write_y4m: no frames")
    H, W = frames[0][0].shape
    if (hs == 2 and W % 2) or (vs == 2 and H % 2):
        raise ValueError("write_y4m: %s needs even sizes, got %dx%d"
                         % (":".join(sampling), W, H))
    tag = b"420jpeg" if sampling == "420" else sampling.encode()
    with open(path, "wb") as fp:
        fp.write(b"%s W%d H%d F%d:%d Ip A1:1 C%s\n" % (MAGIC, W, H, fps[0], fps[1], tag))
        for y, u, v in frames:
            if y.shape != (H, W) or u.shape != (H // vs, W // hs) or v.shape != u.shape:
                raise ValueError("write_y4m: frame planes %s %s %s do not fit %dx%d"
                                 % (y.shape, u.shape, v.shape, W, H))
            fp.write(FRAME_MARKER)
            fp.write(y.tobytes())
            fp.write(u.tobytes())
            fp.write(v.tobytes())
