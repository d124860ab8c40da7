"""Motion-JPEG (``.mjpeg`` / ``.mjpg``) streams: index, a small baseline
encoder, and a numpy reference decoder.

A stream is JPEG frames back to back (SOI ... EOI, SOI ... EOI, ...), what
``ffmpeg -c:v mjpeg -f mjpeg`` writes. Only what ``csrc/jpeg_entropy.cpp``
reads is accepted: baseline sequential Huffman (SOF0), 8-bit, three components
sampled 2x2 / 1x1 / 1x1 (4:2:0), 2x1 / 1x1 / 1x1 (4:2:2) or 1x1 / 1x1 / 1x1
(4:4:4), one interleaved scan, every frame of the first frame's size and
sampling. Containers (AVI / MOV), progressive JPEG, 4:4:0, 4:1:1 and grayscale
are not read.

The *sampling* (``"420"``, ``"422"``, ``"444"``; luma factors (Hs, Vs) = (2, 2),
(2, 1), (1, 1)) sets the MCU: ``8 Hs x 8 Vs`` luma pixels in ``B = Hs Vs + 2``
blocks, the Y blocks row-major, then Cb, then Cr; ``mw = ceil(W / (8 Hs))``,
``mh = ceil(H / (8 Vs))``. ``"420"`` is the default everywhere.

``read_index`` finds the frames (native ``rnb_mjpeg_index_s`` when
``librnb_jpeg.so`` is there, else the parser below); ``write_mjpeg`` encodes
planar frames with the Annex K Huffman tables and returns the quantised
coefficients it wrote; ``decode_reference`` is a slow, independent decoder of
one frame (the tests' oracle, and the fallback entropy decoder).

The *frame record* both decoders produce is the upload format of
``MjpegDecoder``: ``uint16 qt[3][64]`` (the quantisation table of each
component, natural order), then ``int16`` quantised coefficients, 64 per block
in natural order: the Y blocks row-major over the padded ``Vs mh x Hs mw`` grid,
then the ``mh x mw`` Cb blocks, then Cr: ``384 + 128 B mw mh`` bytes
(4:2:0: ``mw = ceil(W / 16)``, ``mh = ceil(H / 16)``, ``384 + 768 mw mh``).

``pack_scans`` / ``decode_scans_host`` serve ``MjpegDecoder(entropy="gpu")``:
the first packs frames' entropy-coded scans into *scan records* (tables, the
byte span of every restart interval, the scan verbatim; layout in
``csrc/jpeg_huff.h``), the second is the host mirror of ``jpeg_huff_kernel``,
which decodes them into frame records, one restart interval per lane, and
with ``subseq_bytes`` the emulation of ``jpeg_huff_subseq_kernel``, which
decodes a scan without restart markers by synchronised subsequences.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
                   12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                   58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K: example quantisation tables (natural order) ...
QT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                      24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                     + [99] * 32)
# ... and Huffman tables: (number of codes of each length 1..16, symbols)
HUFF_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bytes(range(12)))
HUFF_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], bytes(range(12)))
HUFF_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a"
    "25262728292a3435363738393a434445464748494a535455565758595a636465666768696a737475767778797a"
    "838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2"
    "d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
HUFF_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718"
    "191a262728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a"
    "82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9ca"
    "d2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))

# DCT basis: BASIS[u, x] = c(u) / 2 * cos((2x + 1) u pi / 16); samples = B^T F B
_u = np.arange(8, dtype=np.float64)
BASIS = 0.5 * np.cos((2.0 * _u[None, :] + 1.0) * _u[:, None] * np.pi / 16.0)
BASIS[0] *= np.sqrt(0.5)


class JpegError(ValueError):
    """A frame that is not read; ``field`` names what is wrong with it."""

    def __init__(self, field: str, text: str):
        ValueError.__init__(self, text)
        self.field = field


# what rnb_jpeg_error_name returns -> the message
_REASONS = {
    "argument": "bad arguments to the native decoder",
    "truncated": "the data ends inside a segment or inside the scan",
    "SOI": "no SOI marker at the start of the frame",
    "SOF": "progressive, extended or lossless frame; only baseline SOF0 is read",
    "arithmetic": "arithmetic coding; only Huffman coding is read",
    "precision": "sample precision is not 8 bits",
    "DQT precision": "16-bit quantisation table; only 8-bit tables are read",
    "components": "not three components (grayscale / CMYK are not read)",
    "sampling": "sampling factors are not 2x2 / 2x1 / 1x1 luma with 1x1 chroma "
                "(only 4:2:0, 4:2:2 and 4:4:4 are read)",
    "scans": "more than one scan, or a scan that does not hold all three components",
    "size": "the frame's size differs from the first frame's",
    "huffman": "a Huffman code that matches no table entry, or an invalid table",
    "run": "a zero run past coefficient 63",
    "RST": "missing or wrong restart marker",
    "marker": "malformed marker segment",
    "EOI": "no EOI marker behind the scan",
    "table": "the scan refers to a table the frame does not define",
    "record": "the record is too small for the frame",
    "dc_range": "DC value outside the 16-bit range",
    "dimensions": "zero width or height",
    "scan record": "malformed scan record (header, span table, extent or sampling word)",
    "sampling change": "the frame's sampling differs from the first frame's",
}

SAMPLINGS = ("420", "422", "444")        # index: the native sampling word
SAMPLING_FACTORS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
# SOF0 luma sampling byte -> sampling
_SOF_SAMPLING = {0x22: "420", 0x21: "422", 0x11: "444"}


def sampling_factors(sampling: str, who: str = "mjpeg") -> Tuple[int, int]:
    """Luma factors (Hs, Vs); ``ValueError`` naming the argument otherwise."""
    if sampling not in SAMPLING_FACTORS:
        raise ValueError("%s: sampling must be one of %s, got %r" % (who, SAMPLINGS, sampling))
    return SAMPLING_FACTORS[sampling]


def mcu_blocks(sampling: str = "420") -> int:
    """Blocks per MCU: 6, 4 or 3."""
    hs, vs = sampling_factors(sampling, "mcu_blocks")
    return hs * vs + 2


def geometry(width: int, height: int, sampling: str = "420") -> Tuple[int, int, int]:
    """(mw, mh, record bytes) of a ``width`` x ``height`` frame."""
    hs, vs = sampling_factors(sampling, "geometry")
    mw, mh = -(-width // (8 * hs)), -(-height // (8 * vs))
    return mw, mh, 384 + 128 * (hs * vs + 2) * mw * mh


def chroma_size(width: int, height: int, sampling: str = "420") -> Tuple[int, int]:
    """(cw, ch): ceil(width / Hs), ceil(height / Vs)."""
    hs, vs = sampling_factors(sampling, "chroma_size")
    return -(-width // hs), -(-height // vs)


class MjpegIndex(NamedTuple):
    width: int
    height: int
    mw: int                   # MCUs (8 Hs x 8 Vs luma samples) per row
    mh: int                   # MCU rows
    record_bytes: int         # 384 + 128 * B * mw * mh
    restart_interval: int     # of the first frame (informational)
    offsets: np.ndarray       # int64 [frames]: byte offset of each frame's SOI
    lengths: np.ndarray       # int64 [frames]: bytes up to and including its EOI
    sampling: str = "420"     # "420", "422" or "444": every frame's

    @property
    def num_frames(self) -> int:
        return int(self.offsets.shape[0])


def _native():
    from ..ops import native
    return native.jpeg() if native.available("librnb_jpeg.so") else None


def _as_u8(data) -> np.ndarray:
    return data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)


def read_index(path: str, data=None) -> MjpegIndex:
    """Frame table of the stream at ``path``; ``data`` may pass its contents
    (bytes, a memory map or a uint8 array). Every frame's header is parsed;
    raises ``ValueError`` naming file, frame and field for anything not read.
    The first frame is also decoded once: a header that announces another of
    the three samplings than its scan was written for is refused (field
    'sampling'; ``_check_announced_sampling``)."""
    if data is None:
        with open(path, "rb") as fp:
            data = fp.read()
    buf = _as_u8(data)
    if buf.size == 0:
        raise ValueError("%s: empty file (field 'SOI')" % path)
    lib = _native()
    if lib is not None:
        got = lib.index_s(buf)
        if isinstance(got, tuple) and len(got) == 2:          # (field, frame)
            raise ValueError("%s: frame %d is not read (field '%s': %s)"
                             % (path, got[1], got[0], _REASONS.get(got[0], got[0])))
        w, h, ri, offs, lens, sampling = got
        sampling = SAMPLINGS[sampling]
    else:
        offs, lens, pos, w, h, ri, sampling = [], [], 0, 0, 0, 0, "420"
        raw = buf.tobytes()
        while pos < len(raw):
            try:
                hdr = _parse_frame(raw[pos:])
                if offs and hdr["sampling"] != sampling:
                    raise JpegError("sampling change", _REASONS["sampling change"])
                if offs and (hdr["width"], hdr["height"]) != (w, h):
                    raise JpegError("size", _REASONS["size"])
            except JpegError as e:
                raise ValueError("%s: frame %d is not read (field '%s': %s)"
                                 % (path, len(offs), e.field, e))
            if not offs:
                w, h, ri, sampling = hdr["width"], hdr["height"], hdr["restart"], hdr["sampling"]
            offs.append(pos)
            lens.append(hdr["end"])
            pos += hdr["end"]
        offs, lens = np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)
    if len(offs):
        a0 = int(offs[0])
        _check_announced_sampling(path, buf[a0:a0 + int(lens[0])], w, h, sampling)
    mw, mh, rec = geometry(w, h, sampling)
    return MjpegIndex(w, h, mw, mh, rec, ri, offs, lens, sampling)


def _sof_offset(frame: np.ndarray) -> int:
    """Offset of the frame's SOF0 marker (walking the segments), or -1."""
    pos, n = 2, int(frame.size)
    while pos + 4 <= n and frame[pos] == 0xFF:
        m = int(frame[pos + 1])
        if m == 0xFF:
            pos += 1
            continue
        if m == 0xC0:
            return pos
        if m in (0xD9, 0xDA):
            break
        pos += 2 + (int(frame[pos + 2]) << 8 | int(frame[pos + 3]))
    return -1


def _frame_decodes(frame: np.ndarray, w: int, h: int, sampling: str) -> bool:
    lib = _native()
    if lib is not None:
        rec = np.empty(geometry(w, h, sampling)[2], dtype=np.uint8)
        return lib.decode_frames_rc(frame, [0], [frame.size], rec, rec.size, 1,
                                    SAMPLINGS.index(sampling)) == 0
    try:
        return decode_reference(frame.tobytes(), planes=False)["sampling"] == sampling
    except JpegError:
        return False


def _check_announced_sampling(path: str, frame: np.ndarray, w: int, h: int,
                              sampling: str) -> None:
    """The three samplings share every header byte but one, so a header can
    announce a layout its scan was not written for; the blocks then land in the
    wrong planes or the decode fails far from the cause. The stream's first frame
    is therefore decoded once: if it does not decode as announced but does with
    another luma sampling byte, the index refuses it, naming 'sampling'. A frame
    that decodes under none is left to ``decode``'s own refusals, as before."""
    frame = np.ascontiguousarray(frame)
    if _frame_decodes(frame, w, h, sampling):
        return
    sof = _sof_offset(frame)
    if sof < 0 or sof + 11 >= frame.size:
        return
    for byte, other in _SOF_SAMPLING.items():
        if other != sampling:
            trial = frame.copy()
            trial[sof + 11] = byte
            if _frame_decodes(trial, w, h, other):
                raise ValueError("%s: frame 0 is not read (field 'sampling': the header announces "
                                 "%s but the scan decodes only as %s)"
                                 % (path, ":".join(sampling), ":".join(other)))


def entropy_decode(data, offsets, lengths, out: np.ndarray, record_bytes: int,
                   threads: int = 1, name: str = "<mjpeg>", sampling: str = "420") -> None:
    """Entropy-decode the frames at ``offsets`` / ``lengths`` of ``data`` into
    records laid ``record_bytes`` apart in the uint8 array ``out`` (native
    decoder, or ``decode_reference`` when the library is absent). ``sampling``:
    the stream's (``MjpegIndex.sampling``); a frame of another is refused."""
    sampling_factors(sampling, "entropy_decode")
    buf = _as_u8(data)
    n = len(offsets)
    if out.dtype != np.uint8 or out.ndim != 1 or out.size < n * record_bytes:
        raise ValueError("entropy_decode: out must be a flat uint8 array of >= %d bytes"
                         % (n * record_bytes))
    lib = _native()
    if lib is not None:
        field = lib.decode_frames(buf, offsets, lengths, out, record_bytes, threads,
                                  SAMPLINGS.index(sampling))
        if field is not None:
            raise ValueError("%s: a sampled frame is not read (field '%s': %s)"
                             % (name, field, _REASONS.get(field, field)))
        return
    for i in range(n):
        try:
            ref = decode_reference(buf[int(offsets[i]):int(offsets[i] + lengths[i])].tobytes(),
                                   planes=False)
            if ref["sampling"] != sampling:
                raise JpegError("sampling change", _REASONS["sampling change"])
        except JpegError as e:
            raise ValueError("%s: a sampled frame is not read (field '%s': %s)"
                             % (name, e.field, e))
        rec = pack_record(ref["coefs"], ref["qt"])
        if rec.size > record_bytes:
            raise ValueError("%s: a sampled frame is not read (field 'record': %s)"
                             % (name, _REASONS["record"]))
        out[i * record_bytes:i * record_bytes + rec.size] = rec


# scan records (the upload format of ``MjpegDecoder(entropy="gpu")``; layout in
# csrc/jpeg_huff.h): 2032 fixed bytes (tables and header), 8 per restart
# interval, then the scan's bytes, padded to 16
SCAN_RECORD_FIXED = 2032


def scan_record_bound(mw: int, mh: int, frame_len: int) -> int:
    """An upper bound of the scan record of a ``frame_len``-byte frame."""
    return (SCAN_RECORD_FIXED + 8 * mw * mh + int(frame_len) + 15) & ~15


def _need_native(what: str):
    lib = _native()
    if lib is None:
        raise RuntimeError("%s needs librnb_jpeg.so (python -m rnb_amd.build)" % what)
    return lib


def pack_scans(data, offsets, lengths, out: np.ndarray, width: int = 0, height: int = 0,
               name: str = "<mjpeg>", frame0: int = 0,
               sampling: str = "420", frames=None) -> Tuple[int, np.ndarray]:
    """Pack the scans of the frames at ``offsets`` / ``lengths`` of ``data``
    into scan records in the flat, 16-byte aligned uint8 array ``out``
    (``rnb_jpeg_pack_scans``: header parse, restart markers located, counted and
    checked, no Huffman work). ``width`` / ``height``: the size every frame must
    have (0: the first frame's). Returns (bytes written, int64 offsets
    [n + 1] of the records in ``out``). A refusal raises ``JpegError`` naming
    ``name``, the frame (``frame0`` + its index, or ``frames[index]`` where the
    frames are not consecutive) and the field. ``sampling``:
    the stream's; it goes into the record's fourth header word, and a frame of
    another sampling is refused."""
    sampling_factors(sampling, "pack_scans")
    lib = _need_native("pack_scans")
    got, extra = lib.pack_scans(_as_u8(data), offsets, lengths, out, width, height,
                                SAMPLINGS.index(sampling))
    if got < 0:
        field = lib.error_name(got)
        raise JpegError(field, "%s: frame %d is not read (field '%s': %s)"
                        % (name, frame0 + extra if frames is None else int(frames[extra]),
                           field, _REASONS.get(field, field)))
    return got, extra


def check_subseq_bytes(subseq_bytes, what: str) -> int:
    """``subseq_bytes`` as the subsequence decoders take it: 0 (off) or a
    multiple of 16 in 16..4096; anything else raises ``ValueError``."""
    if isinstance(subseq_bytes, bool) or not isinstance(subseq_bytes, (int, np.integer)) \
            or (subseq_bytes != 0 and not (16 <= subseq_bytes <= 4096 and subseq_bytes % 16 == 0)):
        raise ValueError("%s: subseq_bytes must be 0 or a multiple of 16 in 16..4096, got %r"
                         % (what, subseq_bytes))
    return int(subseq_bytes)


def decode_scans_host(scans: np.ndarray, scan_offs, nframes: int, mw: int, mh: int,
                      out: Optional[np.ndarray] = None, record_bytes: Optional[int] = None,
                      status: Optional[np.ndarray] = None, subseq_bytes: int = 0,
                      return_rounds: bool = False, sampling: str = "420"):
    """The GPU interval decoder's host mirror (``rnb_jpeg_decode_scans_host``):
    ``nframes`` scan records -> (frame records ``record_bytes`` apart in a flat
    uint8 array, int32 status per frame: 0 or the code of the frame's
    lowest-numbered failing interval; see ``status_field``). A buffer, offset
    or alignment that is refused raises ``JpegError`` (field 'argument').

    ``subseq_bytes`` > 0 (a multiple of 16 in 16..4096, else ``ValueError``)
    runs the emulation of ``jpeg_huff_subseq_kernel`` instead
    (``rnb_jpeg_decode_scans_subseq_host``): frames without restart markers are
    decoded by synchronised subsequences of that many scan bytes, to the same
    records and status. ``return_rounds`` appends the int32 synchronisation
    rounds per frame (zeros at ``subseq_bytes=0``) to the result.

    ``sampling``: the geometry ``mw`` / ``mh`` count MCUs of; a scan record
    whose sampling word is another one gets the status 'scan record'."""
    check_subseq_bytes(subseq_bytes, "decode_scans_host")
    nb = mcu_blocks(sampling)
    lib = _need_native("decode_scans_host")
    rb = 384 + 128 * nb * mw * mh if record_bytes is None else int(record_bytes)
    if out is None:
        out = np.empty(nframes * rb, dtype=np.uint8)
    if status is None:
        status = np.zeros(nframes, dtype=np.int32)
    rounds = np.zeros(nframes, dtype=np.int32)
    rc = lib.decode_scans_host(scans, scan_offs, nframes, mw, mh, out, rb, status,
                               subseq_bytes, rounds, SAMPLINGS.index(sampling))
    if rc:
        field = lib.error_name(rc)
        raise JpegError(field, "decode_scans_host: %s (field '%s')"
                        % (_REASONS.get(field, field), field))
    return (out, status, rounds) if return_rounds else (out, status)


def status_field(code: int) -> str:
    """The field name of a per-frame status code of the interval decoders."""
    return _need_native("status_field").error_name(int(code))


def raise_for_status(status, name: str, frames) -> None:
    """Raise ``JpegError`` for the first non-zero code in ``status``;
    ``frames[i]`` is the frame number status ``i`` belongs to."""
    bad = np.nonzero(np.asarray(status))[0]
    if bad.size:
        i = int(bad[0])
        field = status_field(int(status[i]))
        raise JpegError(field, "%s: frame %d is not read (field '%s': %s)"
                        % (name, int(frames[i]), field, _REASONS.get(field, field)))


def pack_record(coefs: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """Frame record bytes from ``coefs`` int16 [B mw mh, 64] and ``qt`` [3, 64]."""
    return np.concatenate([np.ascontiguousarray(qt, dtype=np.uint16).reshape(-1).view(np.uint8),
                           np.ascontiguousarray(coefs, dtype=np.int16).reshape(-1).view(np.uint8)])


def unpack_record(rec: np.ndarray, mw: int, mh: int,
                  sampling: str = "420") -> Tuple[np.ndarray, np.ndarray]:
    """(coefs int16 [B mw mh, 64], qt uint16 [3, 64]) views of a record."""
    rec = np.ascontiguousarray(rec[:384 + 128 * mcu_blocks(sampling) * mw * mh])
    return rec[384:].view(np.int16).reshape(-1, 64), rec[:384].view(np.uint16).reshape(3, 64)


# ---------------------------------------------------------------------------
# fp64 reference IDCT
# ---------------------------------------------------------------------------
def idct_planes_f64(coefs: np.ndarray, qt: np.ndarray, mw: int, mh: int,
                    sampling: str = "420"):
    """Ideal IDCT of a frame's blocks: fp64 (Y [8 Vs mh, 8 Hs mw], Cb, Cr
    [8 mh, 8 mw]) sample values + 128, before rounding and clamping."""
    n = mw * mh
    hs, vs = sampling_factors(sampling, "idct_planes_f64")
    ny = hs * vs
    out = []
    for c, (lo, hi, rows, cols) in enumerate(((0, ny * n, vs * mh, hs * mw),
                                              (ny * n, (ny + 1) * n, mh, mw),
                                              ((ny + 1) * n, (ny + 2) * n, mh, mw))):
        f = (coefs[lo:hi].astype(np.float64) * qt[c].astype(np.float64)).reshape(-1, 8, 8)
        s = np.einsum("ux,buv,vy->bxy", BASIS, f, BASIS) + 128.0
        out.append(s.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))
    return tuple(out)


def round_planes(planes) -> Tuple[np.ndarray, ...]:
    return tuple(np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in planes)


# ---------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------
def _codes(bits, vals):
    """symbol -> (code, length) of a canonical Huffman table."""
    out, code, k = {}, 0, 0
    for length, count in enumerate(bits, 1):
        for _ in range(count):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quality_tables(quality: int) -> np.ndarray:
    """The Annex K tables scaled the way libjpeg scales them: uint16 [2, 64]."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (QT_LUMA, QT_CHROMA)]
                    ).astype(np.uint16)


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code: int, length: int) -> None:
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self) -> None:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)      # pad with ones


def _put_block(bw, zz, pred, dc, ac):
    diff = int(zz[0]) - pred
    s = abs(diff).bit_length()
    bw.put(*dc[s])
    if s:
        bw.put(diff if diff > 0 else diff + (1 << s) - 1, s)
    nz = np.nonzero(zz[1:])[0]
    last = 0
    for k in nz + 1:
        run = int(k) - last - 1
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        v = int(zz[k])
        s = abs(v).bit_length()
        bw.put(*ac[(run << 4) | s])
        bw.put(v if v > 0 else v + (1 << s) - 1, s)
        last = int(k)
    if last != 63:
        bw.put(*ac[0x00])
    return int(zz[0])


def _segment(marker: int, body: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def _pad_plane(p: np.ndarray, rows: int, cols: int) -> np.ndarray:
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _fdct_quant(plane: np.ndarray, q: np.ndarray, coef_max: int = 1023) -> np.ndarray:
    rows, cols = plane.shape[0] // 8, plane.shape[1] // 8
    b = (plane.astype(np.float64) - 128.0).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)
    f = np.einsum("ux,rcxy,vy->rcuv", BASIS, b, BASIS).reshape(rows * cols, 64)
    return np.clip(np.rint(f / q.astype(np.float64)), -coef_max, coef_max).astype(np.int16)


def encode_frame(y, u, v, qt: np.ndarray, restart_interval: int = 0,
                 coefs: Optional[np.ndarray] = None,
                 sampling: str = "420") -> Tuple[bytes, np.ndarray]:
    """One baseline JPEG frame of ``sampling`` from uint8 planes Y [H, W] and U, V
    [ceil(H/Vs), ceil(W/Hs)] with quantisation tables ``qt`` [2, 64] (luma,
    chroma; natural order). Returns (bytes, quantised coefficients int16
    [B mw mh, 64] in record order). ``coefs`` (same layout) replaces the
    transform of the planes, for hand-made blocks."""
    y = np.asarray(y)
    H, W = y.shape
    hs, vs = sampling_factors(sampling, "encode_frame")
    ny = hs * vs
    mw, mh, _ = geometry(W, H, sampling)
    qt = np.asarray(qt, dtype=np.uint16).reshape(2, 64)
    if coefs is None:
        cw, ch = chroma_size(W, H, sampling)
        if np.asarray(u).shape != (ch, cw) or np.asarray(v).shape != (ch, cw):
            raise ValueError("encode_frame: chroma planes must be %dx%d for a %dx%d frame"
                             % (cw, ch, W, H))
        coefs = np.concatenate([_fdct_quant(_pad_plane(y, 8 * vs * mh, 8 * hs * mw), qt[0]),
                                _fdct_quant(_pad_plane(np.asarray(u), 8 * mh, 8 * mw), qt[1]),
                                _fdct_quant(_pad_plane(np.asarray(v), 8 * mh, 8 * mw), qt[1])])
    coefs = np.ascontiguousarray(coefs, dtype=np.int16).reshape((ny + 2) * mw * mh, 64)
    head = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    head += _segment(0xDB, b"".join(bytes([i]) + bytes(qt[i][ZIGZAG].astype(np.uint8))
                                    for i in range(2)))
    head += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big")
                     + bytes([3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    tables = ((0x00, HUFF_DC_LUMA), (0x10, HUFF_AC_LUMA), (0x01, HUFF_DC_CHROMA),
              (0x11, HUFF_AC_CHROMA))
    head += _segment(0xC4, b"".join(bytes([i]) + bytes(t[0]) + t[1] for i, t in tables))
    if restart_interval:
        head += _segment(0xDD, int(restart_interval).to_bytes(2, "big"))
    head += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    dcl, acl = _codes(*HUFF_DC_LUMA), _codes(*HUFF_AC_LUMA)
    dcc, acc = _codes(*HUFF_DC_CHROMA), _codes(*HUFF_AC_CHROMA)
    zz = coefs[:, ZIGZAG]
    body = bytearray()
    bw = _BitWriter()
    pred = [0, 0, 0]
    n = mw * mh
    for m in range(n):
        if restart_interval and m and m % restart_interval == 0:
            bw.flush()
            body += bw.out + bytes([0xFF, 0xD0 + (m // restart_interval - 1) % 8])
            bw, pred = _BitWriter(), [0, 0, 0]
        my, mx = divmod(m, mw)
        for dy in range(vs):
            for dx in range(hs):
                pred[0] = _put_block(bw, zz[(vs * my + dy) * hs * mw + hs * mx + dx], pred[0],
                                     dcl, acl)
        pred[1] = _put_block(bw, zz[ny * n + m], pred[1], dcc, acc)
        pred[2] = _put_block(bw, zz[(ny + 1) * n + m], pred[2], dcc, acc)
    bw.flush()
    return head + bytes(body + bw.out) + b"\xff\xd9", coefs


def write_mjpeg(path: str, frames_yuv420, quality: int = 75, restart_interval: int = 0,
                qtables=None, sampling: str = "420") -> List[Tuple[np.ndarray, np.ndarray]]:
    """Write planar frames ``(Y [H, W], U, V [ceil(H/Vs), ceil(W/Hs)])`` of
    ``sampling`` (``"420"``, ``"422"``, ``"444"``) as
    a baseline MJPEG stream with the Annex K Huffman tables; ``restart_interval``
    in MCUs (0: none). ``qtables``: one ``[2, 64]`` (luma, chroma; natural order)
    array for all frames or a sequence of one per frame; default the Annex K
    tables at ``quality``. Returns, per frame, the quantised coefficients written
    (int16 [B mw mh, 64], record order) and the record's tables (uint16 [3, 64])."""
    sampling_factors(sampling, "write_mjpeg")
    frames = list(frames_yuv420)
    if not frames:
        raise ValueError("write_mjpeg: no frames")
    shape = np.asarray(frames[0][0]).shape
    if qtables is None:
        qtables = quality_tables(quality)
    per_frame = not (isinstance(qtables, np.ndarray) and qtables.ndim == 2)
    truth = []
    with open(path, "wb") as fp:
        for i, (y, u, v) in enumerate(frames):
            if np.asarray(y).shape != shape:
                raise ValueError("write_mjpeg: frame %d is %s, the first is %s"
                                 % (i, np.asarray(y).shape, shape))
            qt = np.asarray(qtables[i] if per_frame else qtables, dtype=np.uint16).reshape(2, 64)
            data, coefs = encode_frame(y, u, v, qt, restart_interval, sampling=sampling)
            fp.write(data)
            truth.append((coefs, qt[[0, 1, 1]].copy()))
    return truth


# ---------------------------------------------------------------------------
# reference decoder
# ---------------------------------------------------------------------------
def _parse_frame(buf: bytes) -> dict:
    """Header fields, tables and the scan's extent of the frame at buf[0]."""
    if buf[:2] != b"\xff\xd8":
        raise JpegError("SOI", _REASONS["SOI"])
    pos, qt, huff, hdr = 2, {}, {}, {"restart": 0}
    while True:
        if pos + 2 > len(buf) or (pos + 4 > len(buf) and buf[pos:pos + 2] != b"\xff\xd9"):
            field = "EOI" if "scan" in hdr else "truncated"
            raise JpegError(field, _REASONS[field])
        if buf[pos] != 0xFF:
            raise JpegError("marker", _REASONS["marker"])
        m = buf[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0xD9:
            if "scan" not in hdr:
                raise JpegError("marker", _REASONS["marker"])
            hdr.update(end=pos + 2, qt=qt, huff=huff)
            return hdr
        n = int.from_bytes(buf[pos + 2:pos + 4], "big")
        s = buf[pos + 4:pos + 2 + n]
        if n < 2 or len(s) != n - 2:
            raise JpegError("truncated", _REASONS["truncated"])
        if m == 0xC0:
            if s[0] != 8:
                raise JpegError("precision", _REASONS["precision"])
            if s[5] != 3:
                raise JpegError("components", _REASONS["components"])
            if s[7] not in _SOF_SAMPLING or [s[10], s[13]] != [0x11, 0x11]:
                raise JpegError("sampling", _REASONS["sampling"])
            hdr.update(sampling=_SOF_SAMPLING[s[7]], height=int.from_bytes(s[1:3], "big"),
                       width=int.from_bytes(s[3:5], "big"),
                       tq=[s[8], s[11], s[14]])
            if not hdr["width"] or not hdr["height"]:
                raise JpegError("dimensions", _REASONS["dimensions"])
        elif m in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise JpegError("arithmetic", _REASONS["arithmetic"])
        elif 0xC1 <= m <= 0xC7 and m != 0xC4:
            raise JpegError("SOF", _REASONS["SOF"])
        elif m == 0xDB:
            for o in range(0, len(s), 65):
                if s[o] >> 4:
                    raise JpegError("DQT precision", _REASONS["DQT precision"])
                t = np.zeros(64, dtype=np.uint16)
                t[ZIGZAG] = np.frombuffer(s[o + 1:o + 65], dtype=np.uint8)
                qt[s[o] & 15] = t
        elif m == 0xC4:
            o = 0
            while o < len(s):
                bits = list(s[o + 1:o + 17])
                vals = s[o + 17:o + 17 + sum(bits)]
                huff[s[o]] = {(ln, c): sym for sym, (c, ln) in _codes(bits, vals).items()}
                o += 17 + sum(bits)
        elif m == 0xDD:
            hdr["restart"] = int.from_bytes(s[:2], "big")
        elif m == 0xDA:
            if "scan" in hdr or s[0] != 3 or "width" not in hdr:
                raise JpegError("scans", _REASONS["scans"])
            hdr["tables"] = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(3)]
            q = pos + 2 + n
            while True:
                q = buf.find(b"\xff", q)
                if q < 0 or q + 1 >= len(buf):
                    raise JpegError("EOI", _REASONS["EOI"])
                if buf[q + 1] == 0 or 0xD0 <= buf[q + 1] <= 0xD7:
                    q += 2
                elif buf[q + 1] == 0xFF:
                    q += 1
                else:
                    break
            hdr["scan"] = (pos + 2 + n, q)
            pos = q
            continue
        pos += 2 + n


def decode_reference(frame_bytes: bytes, planes: bool = True) -> dict:
    """Decode one baseline 4:2:0 / 4:2:2 / 4:4:4 frame in numpy: ``coefs`` (int16
    [B mw mh, 64], record order), ``qt`` (uint16 [3, 64]), ``width``, ``height``,
    ``mw``, ``mh``, ``sampling`` and, with ``planes``, ``planes_f64`` (ideal IDCT + 128 at the padded size,
    before rounding) and ``planes_u8`` (rounded, clamped). Raises ``JpegError``."""
    buf = bytes(frame_bytes)
    hdr = _parse_frame(buf)
    W, H = hdr["width"], hdr["height"]
    sampling = hdr["sampling"]
    hs, vs = SAMPLING_FACTORS[sampling]
    ny = hs * vs
    mw, mh, _ = geometry(W, H, sampling)
    n = mw * mh
    try:
        qt = np.stack([hdr["qt"][t] for t in hdr["tq"]])
        tabs = [(hdr["huff"][d], hdr["huff"][0x10 | a]) for d, a in hdr["tables"]]
    except KeyError:
        raise JpegError("table", _REASONS["table"])
    coefs = np.zeros(((ny + 2) * n, 64), dtype=np.int16)
    a, b = hdr["scan"]
    chunks, start = [], a
    for q in range(a, b - 1):                      # split at RSTn
        if buf[q] == 0xFF and 0xD0 <= buf[q + 1] <= 0xD7:
            chunks.append((buf[start:q], buf[q + 1] - 0xD0))
            start = q + 2
    chunks.append((buf[start:b], None))
    ri = hdr["restart"] or n
    if len(chunks) != -(-n // ri) or any(r is not None and r != i % 8
                                         for i, (_, r) in enumerate(chunks)):
        raise JpegError("RST", _REASONS["RST"])
    for ci, (chunk, _) in enumerate(chunks):
        bits = np.unpackbits(np.frombuffer(chunk.replace(b"\xff\x00", b"\xff"), dtype=np.uint8))
        bits = np.concatenate([bits, np.zeros(64, dtype=np.uint8)]).tolist()
        real, pos, pred = len(bits) - 64, 0, [0, 0, 0]

        def symbol(table):
            nonlocal pos
            code = 0
            for ln in range(1, 17):
                code = (code << 1) | bits[pos + ln - 1]
                if (ln, code) in table:
                    pos += ln
                    return table[ln, code]
            raise JpegError("huffman", _REASONS["huffman"])

        def receive(s):
            nonlocal pos
            v = 0
            for bit in bits[pos:pos + s]:
                v = (v << 1) | bit
            pos += s
            return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

        for m in range(ci * ri, min(n, (ci + 1) * ri)):
            my, mx = divmod(m, mw)
            blocks = [(0, (vs * my + dy) * hs * mw + hs * mx + dx)
                      for dy in range(vs) for dx in range(hs)]
            for c, blk in blocks + [(1, ny * n + m), (2, (ny + 1) * n + m)]:
                dc, ac = tabs[c]
                s = symbol(dc)
                if s > 11:
                    raise JpegError("dc_range", _REASONS["dc_range"])
                pred[c] += receive(s) if s else 0
                if not -32768 <= pred[c] <= 32767:
                    raise JpegError("dc_range", _REASONS["dc_range"])
                coefs[blk, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = symbol(ac)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        if k + 15 > 63:
                            raise JpegError("run", _REASONS["run"])
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        raise JpegError("run", _REASONS["run"])
                    coefs[blk, ZIGZAG[k]] = receive(s)
                    k += 1
                if pos > real:
                    raise JpegError("truncated", _REASONS["truncated"])
    out = dict(coefs=coefs, qt=qt, width=W, height=H, mw=mw, mh=mh, sampling=sampling)
    if planes:
        out["planes_f64"] = idct_planes_f64(coefs, qt, mw, mh, sampling)
        out["planes_u8"] = round_planes(out["planes_f64"])
    return out
