"""Time the mjpeg decode path per 15-clip request at 340x256 (GPU required).

  * kernels: ``jpeg_idct_kernel`` on the request's 120 frame records, a device
    copy moving the same number of bytes as its ceiling, and the clip kernel
    (``yuv420_to_clip``: one ``rnb_yuv_to_clip_boxes`` launch, the only form) on
    the IDCT surface with the JFIF and with the BT.601 matrix; alternating,
    device events around ``--reps`` back-to-back launches per round;
  * host: ``MjpegDecoder.decode`` with 1, 4 and 16 entropy-decode threads on a
    stream written to a temporary directory (smooth synthetic frames with a
    little noise, quality 75; the entropy decode's cost grows with the bit
    rate) and read once before: time of the call itself, and of the call plus
    a device synchronise; and the host entropy decode alone; then the
    sustained rate of ``--sustained`` requests back to back with one final
    synchronise, which counts kernels that outlast the host call;
  * ``--entropy gpu`` adds, in the same session: ``jpeg_huff_kernel`` on the
    request's 120 packed scan records (back-to-back launches, device events),
    the scan packer alone, and the same host and sustained figures for
    ``MjpegDecoder(entropy="gpu")``, with the bytes each path uploads.
    ``--restart-interval N`` writes the stream with a restart marker every N
    MCUs (22: one MCU row at 340x256, 16 intervals, i.e. GPU lanes, per frame;
    0: none, one lane per frame). ``--subseq-bytes 0,64,256`` times
    ``jpeg_huff_subseq_kernel`` at each size above 0 in the same rounds as
    ``jpeg_huff_kernel`` (0, the baseline), after comparing its records with
    the host decoder's, prints the synchronisation rounds and subsequences
    per frame, and repeats the ``MjpegDecoder(entropy="gpu")`` rows per size.

    ``--sampling 422`` / ``444`` encodes, decodes and reports that chroma layout
    (default 420) on every row.

    ``--short-side S [--views V]`` reports the short-side resize + window
    protocol instead (``crop={"short_side": S, "views": V}``): the host and
    sustained rows of ``MjpegDecoder`` with ``threads=4`` and with
    ``entropy="gpu"``, both filters, for 1 view and for ``V``; the bytes
    uploaded per request do not depend on the views.

    ``--reduce 1,2,4,auto [--size 1280x720]`` reports the reduced-size decode
    instead (``MjpegDecoder(reduce=)``): per value the ``jpeg_idct`` launch, the
    clip launch on its surface (both filters, one view and three of short side
    128), the surface bytes, and the host and sustained rows of ``MjpegDecoder``
    with ``threads=4`` and with ``entropy="gpu", subseq_bytes=48`` on three
    antialiased views; the values alternate within every round.

    ``--frame-step N`` or ``--fps R`` reports ``MjpegDecoder.decode(step=)``
    instead: the request's clips at every N-th frame, or at ``R`` frames per
    second of a 30 fps stream, with ``threads=4`` and with ``entropy="gpu"``
    (host and sustained rows; ``--frame-step 1`` is consecutive frames).

    python scripts/mjpeg_decode_bench.py --out profiles/mjpeg_decode.txt
    python scripts/mjpeg_decode_bench.py --entropy gpu --restart-interval 22
    python scripts/mjpeg_decode_bench.py --entropy gpu --subseq-bytes 0,64,128,256,512
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_mjpeg_dataset import synthetic_frames  # noqa: E402
from rnb_amd.models.r2p1d.decoder import MjpegDecoder  # noqa: E402
from rnb_amd.ops import video as vops  # noqa: E402
from rnb_amd.utils import mjpeg  # noqa: E402

W, H, F, CLIPS = vops.SOURCE_W, vops.SOURCE_H, 8, 15
DISTINCT = 24          # frames encoded; the stream repeats them
SAMPLING = "420"       # --sampling: the chroma layout of everything below


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def encode(quality, restart=0):
    q = mjpeg.quality_tables(quality)
    return [mjpeg.encode_frame(*f, q, restart, sampling=SAMPLING)
            for f in synthetic_frames(3, DISTINCT, W, H, sampling=SAMPLING)]


def huff_kernel(dev, encoded, reps, rounds, lines, subseq=()):
    """jpeg_huff_kernel on one request's scan records, alternating with the
    IDCT kernel it feeds and with jpeg_huff_subseq_kernel at every size in
    ``subseq``."""
    mw, mh, rb = mjpeg.geometry(W, H, SAMPLING)
    n = CLIPS * F
    frames = [encoded[i % DISTINCT][0] for i in range(n)]
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    data = np.frombuffer(b"".join(frames), dtype=np.uint8)
    buf = np.zeros(sum(mjpeg.scan_record_bound(mw, mh, x) for x in lens), dtype=np.uint8)
    size, scan_offs = mjpeg.pack_scans(data, offs, lens, buf, sampling=SAMPLING)
    scans = torch.from_numpy(buf[:size]).to(dev)
    offs_dev = torch.from_numpy(scan_offs).to(dev)
    rec = torch.empty(n * rb, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    surf = torch.empty(n * vops.jpeg_frame_bytes(mw, mh, SAMPLING)[1], dtype=torch.uint8,
                       device=dev)

    def huff():
        vops.jpeg_huff(scans, scan_offs, n, mw, mh, out=rec, status=status, offs_dev=offs_dev,
                       sampling=SAMPLING)

    def idct():
        vops.jpeg_idct(rec, n, mw, mh, out=surf, sampling=SAMPLING)
    sync_rounds = torch.zeros(n, dtype=torch.int32, device=dev)

    def huff_subseq(size):
        def run():
            vops.jpeg_huff(scans, scan_offs, n, mw, mh, out=rec, status=status, offs_dev=offs_dev,
                           subseq_bytes=size, rounds=sync_rounds, sampling=SAMPLING)
        return run
    reps = max(10, reps // 10)                            # a millisecond-scale kernel
    fns = (("jpeg_huff_kernel", huff), ("jpeg_idct_kernel", idct)) + tuple(
        ("jpeg_huff_subseq S=%d" % sub, huff_subseq(sub)) for sub in subseq if sub)
    want = np.empty(n * rb, dtype=np.uint8)
    mjpeg.entropy_decode(data, offs, lens, want, rb, 4, sampling=SAMPLING)
    shape = {}
    for name, fn in fns:
        if fn is not idct:
            rec.fill_(0x5A)
        event_ms(fn, reps)
        assert int(status.abs().sum()) == 0, name
        assert (rec.cpu().numpy() == want).all(), name    # what is timed is the right answer
        if "subseq" in name:
            sub = int(name.split("=")[1])
            spans = [int(buf[o + 2036:o + 2040].view(np.uint32)[0])
                     - int(buf[o + 2032:o + 2036].view(np.uint32)[0]) for o in scan_offs[:-1]]
            shape[name] = (sync_rounds.float().mean().item(), int(sync_rounds.max()),
                           float(np.mean([-(-x // sub) for x in spans])))
    times = {name: [] for name, _ in fns}
    for _ in range(rounds):
        for name, fn in fns:
            times[name].append(event_ms(fn, reps))
    intervals = int(buf[2016:2020].view(np.uint32)[0])
    for name, _ in fns:
        t = times[name]
        lines.append("%-26s median %.1f us/launch (min %.1f, max %.1f over %d rounds of %d)"
                     % (name, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, rounds, reps))
    lines.append("jpeg_huff_kernel: %d workgroups of 64 lanes, %d intervals (busy lanes) per frame; "
                 "%d bytes of scan records in, %d bytes of frame records out"
                 % (n, intervals, size, n * rb))
    for name in shape:
        lines.append("%s: %d workgroups of 256 lanes; synchronisation rounds per frame mean %.1f, "
                     "max %d; %.0f subsequences per frame%s"
                     % ((name, n) + shape[name]
                        + ("" if intervals == 1 else " if it had one interval: it has %d, one "
                           "lane each, no rounds" % intervals,)))
    t = []
    for _ in range(20):
        t0 = time.perf_counter()
        mjpeg.pack_scans(data, offs, lens, buf, sampling=SAMPLING)
        t.append((time.perf_counter() - t0) * 1e3)
    lines.append("scan packer alone: median %.3f ms per %d frames (min %.3f), one thread"
                 % (statistics.median(t), n, min(t)))


def kernels(dev, dtype, encoded, reps, rounds, lines, filter="bilinear"):
    mw, mh, rb = mjpeg.geometry(W, H, SAMPLING)
    n = CLIPS * F
    qt = mjpeg.quality_tables(75)[[0, 1, 1]]
    rec = torch.from_numpy(np.concatenate(
        [mjpeg.pack_record(encoded[i % DISTINCT][1], qt) for i in range(n)])).to(dev)
    fb = vops.jpeg_frame_bytes(mw, mh, SAMPLING)[1]
    surf = torch.empty(n * fb, dtype=torch.uint8, device=dev)
    C = 4 if dtype == torch.float32 else 8
    out = torch.empty((CLIPS, F, 112, 112, C), dtype=dtype, device=dev)
    offs = [c * F * fb for c in range(CLIPS)]
    planes = vops.jpeg_surface_planes(mw, mh, SAMPLING)
    moved = rec.numel() + surf.numel()
    src, dst = (torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(2))

    def idct():
        vops.jpeg_idct(rec, n, mw, mh, out=surf, sampling=SAMPLING)

    def copy():
        dst.copy_(src)

    def jfif():
        vops.yuv420_to_clip(surf, offs, F, W, H, fb, planes, dtype=dtype, out=out, matrix="jfif",
                            sampling=SAMPLING)

    def bt601():
        vops.yuv420_to_clip(surf, offs, F, W, H, fb, planes, dtype=dtype, out=out,
                            sampling=SAMPLING)
    fns = (("jpeg_idct_kernel", idct, moved), ("device copy, same bytes", copy, moved),
           ("yuv420_clip_kernel jfif", jfif, n * fb + out.numel() * out.element_size()),
           ("yuv420_clip_kernel bt601", bt601, n * fb + out.numel() * out.element_size()))
    if filter == "antialias":
        def jfif_aa():
            vops.yuv420_to_clip(surf, offs, F, W, H, fb, planes, dtype=dtype, out=out,
                                matrix="jfif", filter="antialias", sampling=SAMPLING)
        fns += (("yuv420_clip_aa_kernel jfif", jfif_aa,
                 n * fb + out.numel() * out.element_size()),)
    for _, fn, _ in fns:
        event_ms(fn, reps)                                # warm
    times = {name: [] for name, _, _ in fns}
    for _ in range(rounds):
        for name, fn, _ in fns:
            times[name].append(event_ms(fn, reps))
    for name, _, nbytes in fns:
        t = times[name]
        med = statistics.median(t)
        lines.append("%-26s %s: median %.2f us/launch (min %.2f, max %.2f over %d rounds of %d); "
                     "%.0f GB/s of %d bytes read + written"
                     % (name, str(dtype).split(".")[1], med * 1e3, min(t) * 1e3, max(t) * 1e3,
                        rounds, reps, nbytes / med / 1e6, nbytes))
    lines.append("records uploaded per request: %d bytes (%d frames of %d); IDCT surface %d bytes; "
                 "raw 4:2:0 of the same frames %d bytes"
                 % (rec.numel(), n, rb, surf.numel(), n * W * H * 3 // 2))


def decoder_rows(dev, dtype, path, starts, out, reqs, sustained, lines, label, step=(1, 1),
                 **kw):
    """Host time of decode, and the sustained rate with one final synchronise."""
    dec = MjpegDecoder(dev, dtype=dtype, **kw)
    vid, _ = dec.probe(path)
    for _ in range(5):
        dec.decode(vid, starts, out=out, step=step)
    torch.cuda.synchronize()
    call, total = [], []
    for _ in range(reqs):
        t0 = time.perf_counter()
        dec.decode(vid, starts, out=out, step=step)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        call.append((t1 - t0) * 1e3)
        total.append((t2 - t0) * 1e3)
    med = statistics.median(call)
    lines.append("MjpegDecoder.decode %-16s %s: host call median %.3f ms (min %.3f, "
                 "max %.3f), call + sync median %.3f ms, %d requests of %d clips: "
                 "%.0f videos/s from one loader process"
                 % (label, str(dtype).split(".")[1], med, min(call), max(call),
                    statistics.median(total), reqs, CLIPS, 1e3 / med))
    rates = []
    for _ in range(3):
        before = dict(dec.stats)
        t0 = time.perf_counter()
        for _ in range(sustained):
            dec.decode(vid, starts, out=out, step=step)
        torch.cuda.synchronize()
        rates.append(sustained / (time.perf_counter() - t0))
    dec.drain()
    up = (dec.stats["uploaded_bytes"] - before["uploaded_bytes"]) // sustained
    lines.append("MjpegDecoder.decode %-16s sustained: %.0f requests/s (min %.0f, max %.0f over 3 "
                 "runs of %d back-to-back requests, one final synchronise); %d bytes uploaded "
                 "per request" % (label, statistics.median(rates), min(rates), max(rates),
                                  sustained, up))


def host(dev, dtype, encoded, reqs, lines, sustained=60, entropy="host", restart=0,
         subseq=(), filter="bilinear"):
    frames = 300
    starts = [20 * c for c in range(CLIPS)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.mjpeg")
        with open(path, "wb") as fp:
            for i in range(frames):
                fp.write(encoded[i % DISTINCT][0])
        size = os.path.getsize(path)
        lines.append("stream: %d frames, %.1f KB per frame (raw 4:2:0: %.1f KB), quality 75, "
                     "restart interval %d"
                     % (frames, size / frames / 1e3, W * H * 1.5 / 1e3, restart))
        data = np.fromfile(path, dtype=np.uint8)
        idx = mjpeg.read_index(path, data=data)
        sel = np.concatenate([np.arange(s, s + F) for s in starts])
        rec = np.empty(len(sel) * idx.record_bytes, dtype=np.uint8)
        C = 4 if dtype == torch.float32 else 8
        out = torch.empty((CLIPS, F, 112, 112, C), dtype=dtype, device=dev)
        for threads in (1, 4, 16):
            t = []
            for _ in range(max(3, reqs // 4)):
                t0 = time.perf_counter()
                mjpeg.entropy_decode(data, idx.offsets[sel], idx.lengths[sel], rec,
                                     idx.record_bytes, threads, sampling=idx.sampling)
                t.append((time.perf_counter() - t0) * 1e3)
            lines.append("entropy decode alone, %2d threads: median %.2f ms per %d frames "
                         "(min %.2f)" % (threads, statistics.median(t), len(sel), min(t)))
            decoder_rows(dev, dtype, path, starts, out, reqs, sustained, lines,
                         "threads=%d" % threads, threads=threads, filter=filter)
        if entropy == "gpu":
            for sub in subseq or (None,):
                decoder_rows(dev, dtype, path, starts, out, reqs, sustained, lines,
                             "entropy=gpu" if sub is None else "gpu S=%d" % sub,
                             entropy="gpu", subseq_bytes=sub, filter=filter)


def step_host(dev, dtype, encoded, reqs, lines, sustained, filt, frame_step, fps):
    """``--frame-step`` / ``--fps``: ``MjpegDecoder.decode(step=)`` on a 30 fps
    stream, host entropy decode on 4 threads and the GPU's."""
    from rnb_amd.models.r2p1d.sampler import clip_span, step_of
    step = step_of(frame_step or 1, fps, (30, 1))
    span = clip_span(F, step)
    starts = [max(20, span) * c for c in range(CLIPS)]
    frames = starts[-1] + span + 4
    C = 4 if dtype == torch.float32 else 8
    out = torch.empty((CLIPS, F, 112, 112, C), dtype=dtype, device=dev)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.mjpeg")
        with open(path, "wb") as fp:
            for i in range(frames):
                fp.write(encoded[i % DISTINCT][0])
        for label, kw in (("threads=4", dict(threads=4)), ("entropy=gpu", dict(entropy="gpu"))):
            decoder_rows(dev, dtype, path, starts, out, reqs, sustained, lines,
                         "%s step %d/%d" % (label, step[0], step[1]), step=step, filter=filt,
                         source_fps=30, **kw)


def views_host(dev, dtype, encoded, reqs, lines, sustained, short_side, nviews):
    frames = 300
    starts = [20 * c for c in range(CLIPS)]
    C = 4 if dtype == torch.float32 else 8
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.mjpeg")
        with open(path, "wb") as fp:
            for i in range(frames):
                fp.write(encoded[i % DISTINCT][0])
        for filt in vops.FILTERS:
            for v in sorted({1, nviews}):
                out = torch.empty((CLIPS * v, F, 112, 112, C), dtype=dtype, device=dev)
                crop = {"short_side": short_side, "views": v}
                for label, kw in (("threads=4", dict(threads=4)), ("entropy=gpu", dict(entropy="gpu"))):
                    decoder_rows(dev, dtype, path, starts, out, reqs, sustained, lines,
                                 "%s %s v=%d" % (label, filt[:4], v), filter=filt, crop=crop, **kw)


def reduce_report(dev, encoded, reduces, reps, rounds, reqs, sustained, lines):
    """``--reduce``: per value, the IDCT launch on the request's 120 records, the
    clip launch on its surface (both filters, one view and three, the windows of
    short side 128 divided by the reduce), the surface bytes, and
    ``MjpegDecoder(crop={"short_side": 128, "views": 3}, filter="antialias")``
    with ``threads=4`` and with ``entropy="gpu", subseq_bytes=48``. ``reduce=1``
    passes no ``reduce`` argument anywhere: the calls of a tree without it."""
    from rnb_amd.models.r2p1d.decoder import view_boxes
    dtype = torch.float32
    mw, mh, rb = mjpeg.geometry(W, H, SAMPLING)
    n = CLIPS * F
    qt = mjpeg.quality_tables(75)[[0, 1, 1]]
    rec = torch.from_numpy(np.concatenate(
        [mjpeg.pack_record(encoded[i % DISTINCT][1], qt) for i in range(n)])).to(dev)
    probe = MjpegDecoder(torch.device("cpu"), crop={"short_side": 128, "views": 3},
                         **({"reduce": "auto"} if "auto" in reduces else {}))
    cases = []
    for r in reduces:
        s = probe.auto_reduce(W, H) if r == "auto" else int(r)
        rk = {} if s == 1 else {"reduce": s}
        fb = vops.jpeg_frame_bytes(mw, mh, SAMPLING, **rk)[1]
        surf = torch.empty(n * fb, dtype=torch.uint8, device=dev)
        planes = vops.jpeg_surface_planes(mw, mh, SAMPLING, **rk)
        fns = [("jpeg_idct", lambda surf=surf, rk=rk: vops.jpeg_idct(
            rec, n, mw, mh, out=surf, sampling=SAMPLING, **rk))]
        for v in (1, 3):
            boxes = [tuple(c / s for c in b) for b in view_boxes(W, H, 112, 112, 128, v)]
            offs = [c * F * fb for c in range(CLIPS) for _ in range(v)]
            out = torch.empty((CLIPS * v, F, 112, 112, 4), dtype=dtype, device=dev)
            for filt in vops.FILTERS:
                fns.append(("clip %s %dv" % (filt[:4], v),
                            lambda surf=surf, offs=offs, fb=fb, planes=planes, out=out,
                            boxes=boxes * CLIPS, filt=filt, s=s: vops.yuv420_to_clip(
                                surf, offs, F, -(-W // s), -(-H // s), fb, planes, crop=boxes,
                                dtype=dtype, out=out, matrix="jfif", filter=filt,
                                sampling=SAMPLING)))
        cases.append((r, s, fb, fns))
    for _, _, _, fns in cases:
        for _, fn in fns:
            event_ms(fn, reps)                                # warm
    times = {}
    for _ in range(rounds):                                   # the reduces alternate per round
        for r, _, _, fns in cases:
            for name, fn in fns:
                times.setdefault((r, name), []).append(event_ms(fn, reps))
    for r, s, fb, fns in cases:
        lines.append("reduce %s (s = %d): frame %dx%d, surface %d bytes per request (%d per frame)"
                     % (r, s, -(-W // s), -(-H // s), n * fb, fb))
        for name, _ in fns:
            t = times[r, name]
            lines.append("  %-14s median %.2f us/launch (min %.2f, max %.2f over %d rounds of %d)"
                         % (name, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, rounds,
                            reps))
    frames = 300
    starts = [20 * c for c in range(CLIPS)]
    out = torch.empty((CLIPS * 3, F, 112, 112, 4), dtype=dtype, device=dev)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.mjpeg")
        with open(path, "wb") as fp:
            for i in range(frames):
                fp.write(encoded[i % DISTINCT][0])
        for label, kw in (("threads=4", dict(threads=4)),
                          ("gpu S=48", dict(entropy="gpu", subseq_bytes=48))):
            for r in reduces:
                rk = {} if r == 1 else {"reduce": r}
                decoder_rows(dev, dtype, path, starts, out, reqs, sustained, lines,
                             "%s r=%s" % (label, r), filter="antialias",
                             crop={"short_side": 128, "views": 3}, **dict(kw, **rk))


def main():
    global SAMPLING, W, H, DISTINCT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--requests", type=int, default=40)
    ap.add_argument("--sustained", type=int, default=60,
                    help="back-to-back requests per sustained-rate run")
    ap.add_argument("--entropy", choices=("host", "gpu"), default="host",
                    help="gpu: also measure jpeg_huff_kernel and MjpegDecoder(entropy='gpu')")
    ap.add_argument("--restart-interval", type=int, default=0, help="in MCUs; 0: none")
    ap.add_argument("--subseq-bytes", default="",
                    help="with --entropy gpu: comma-separated subsequence sizes for "
                         "jpeg_huff_subseq_kernel (0: jpeg_huff_kernel, always the baseline)")
    ap.add_argument("--filter", choices=vops.FILTERS, default="bilinear",
                    help="antialias: also time yuv420_clip_aa_kernel, and decode with "
                         "MjpegDecoder(filter='antialias')")
    ap.add_argument("--sampling", choices=mjpeg.SAMPLINGS, default="420")
    ap.add_argument("--short-side", type=float, default=None,
                    help="report MjpegDecoder with crop={'short_side': S, 'views': V} instead")
    ap.add_argument("--views", type=int, choices=(1, 3), default=1, help="with --short-side")
    ap.add_argument("--reduce", default="",
                    help="comma-separated reduces (1, 2, 4, 8, auto): report the reduced-size "
                         "decode instead (reduce_report)")
    ap.add_argument("--size", default=None, help="WxH of the synthetic frames (default 340x256)")
    ap.add_argument("--distinct", type=int, default=DISTINCT,
                    help="frames encoded; the stream repeats them")
    ap.add_argument("--frame-step", type=int, default=None,
                    help="report MjpegDecoder.decode(step=(N, 1)) instead (1: consecutive frames)")
    ap.add_argument("--fps", default=None,
                    help="report MjpegDecoder.decode at this rate of a 30 fps stream instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    SAMPLING = args.sampling
    DISTINCT = args.distinct
    if args.size:
        W, H = (int(x) for x in args.size.lower().split("x"))
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_decode_bench: needs a GPU")
    dev = torch.device("cuda:0")
    lines = ["mjpeg decode path, sampling %s, per 15-clip request at %dx%d -> 112x112%s (%s)"
             % (":".join(SAMPLING), W, H,
                ", filter antialias" if args.filter == "antialias" else "",
                torch.cuda.get_device_name(0))]
    subseq = tuple(mjpeg.check_subseq_bytes(int(x), "--subseq-bytes")
                   for x in args.subseq_bytes.split(",") if x.strip())
    encoded = encode(75, args.restart_interval)
    if args.reduce:
        reduces = [r if r == "auto" else int(r) for r in
                   (x.strip() for x in args.reduce.split(",")) if r]
        lines[0] = ("mjpeg reduced-size decode, sampling %s, per 15-clip request at %dx%d -> "
                    "112x112, short side 128 (%s)"
                    % (":".join(SAMPLING), W, H, torch.cuda.get_device_name(0)))
        reduce_report(dev, encoded, reduces, args.reps, args.rounds, args.requests,
                      args.sustained, lines)
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if args.out:
            with open(args.out, "w") as fp:
                fp.write(text)
        return
    if args.frame_step is not None or args.fps is not None:
        lines[0] = ("mjpeg decode path, sampling %s, frame step %s, fps %s, per 15-clip request "
                    "at %dx%d -> 112x112 (%s)"
                    % (":".join(SAMPLING), args.frame_step, args.fps, W, H,
                       torch.cuda.get_device_name(0)))
        step_host(dev, torch.float32, encoded, args.requests, lines, args.sustained, args.filter,
                  args.frame_step, args.fps)
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if args.out:
            with open(args.out, "w") as fp:
                fp.write(text)
        return
    if args.short_side is not None:
        lines[0] = ("mjpeg decode path, sampling %s, short side %g, %d view(s), per 15-clip "
                    "request at %dx%d -> 112x112 (%s)"
                    % (":".join(SAMPLING), args.short_side, args.views, W, H,
                       torch.cuda.get_device_name(0)))
        views_host(dev, torch.float32, encoded, args.requests, lines, args.sustained,
                   args.short_side, args.views)
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if args.out:
            with open(args.out, "w") as fp:
                fp.write(text)
        return
    for dtype in (torch.float32, torch.bfloat16):
        kernels(dev, dtype, encoded, args.reps, args.rounds, lines, args.filter)
    if args.entropy == "gpu":
        huff_kernel(dev, encoded, args.reps, args.rounds, lines, subseq)
    host(dev, torch.float32, encoded, args.requests, lines, args.sustained, args.entropy,
         args.restart_interval, subseq, args.filter)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
