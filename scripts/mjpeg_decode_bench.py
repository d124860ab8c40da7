"""Time the mjpeg decode path per 15-clip request at 340x256 (GPU required).

  * kernels: ``jpeg_idct_kernel`` on the request's 120 frame records, a device
    copy moving the same number of bytes as its ceiling, and the clip kernel on
    the IDCT surface with the JFIF and with the BT.601 matrix; alternating,
    device events around ``--reps`` back-to-back launches per round;
  * host: ``MjpegDecoder.decode`` with 1, 4 and 16 entropy-decode threads on a
    stream written to a temporary directory (smooth synthetic frames with a
    little noise, quality 75; the entropy decode's cost grows with the bit
    rate) and read once before: time of the call itself, and of the call plus
    a device synchronise; and the host entropy decode alone.

    python scripts/mjpeg_decode_bench.py --out profiles/mjpeg_decode.txt
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


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def encode(quality):
    q = mjpeg.quality_tables(quality)
    return [mjpeg.encode_frame(*f, q) for f in synthetic_frames(3, DISTINCT, W, H)]


def kernels(dev, dtype, encoded, reps, rounds, lines):
    mw, mh, rb = mjpeg.geometry(W, H)
    n = CLIPS * F
    qt = mjpeg.quality_tables(75)[[0, 1, 1]]
    rec = torch.from_numpy(np.concatenate(
        [mjpeg.pack_record(encoded[i % DISTINCT][1], qt) for i in range(n)])).to(dev)
    fb = 384 * mw * mh
    surf = torch.empty(n * fb, dtype=torch.uint8, device=dev)
    C = 4 if dtype == torch.float32 else 8
    out = torch.empty((CLIPS, F, 112, 112, C), dtype=dtype, device=dev)
    offs = [c * F * fb for c in range(CLIPS)]
    planes = vops.jpeg_surface_planes(mw, mh)
    moved = rec.numel() + surf.numel()
    src, dst = (torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(2))

    def idct():
        vops.jpeg_idct(rec, n, mw, mh, out=surf)

    def copy():
        dst.copy_(src)

    def jfif():
        vops.yuv420_to_clip(surf, offs, F, W, H, fb, planes, dtype=dtype, out=out, matrix="jfif")

    def bt601():
        vops.yuv420_to_clip(surf, offs, F, W, H, fb, planes, dtype=dtype, out=out)
    fns = (("jpeg_idct_kernel", idct, moved), ("device copy, same bytes", copy, moved),
           ("yuv420_clip_kernel jfif", jfif, n * fb + out.numel() * out.element_size()),
           ("yuv420_clip_kernel bt601", bt601, n * fb + out.numel() * out.element_size()))
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


def host(dev, dtype, encoded, reqs, lines):
    frames = 300
    starts = [20 * c for c in range(CLIPS)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.mjpeg")
        with open(path, "wb") as fp:
            for i in range(frames):
                fp.write(encoded[i % DISTINCT][0])
        size = os.path.getsize(path)
        lines.append("stream: %d frames, %.1f KB per frame (raw 4:2:0: %.1f KB), quality 75"
                     % (frames, size / frames / 1e3, W * H * 1.5 / 1e3))
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
                                     idx.record_bytes, threads)
                t.append((time.perf_counter() - t0) * 1e3)
            lines.append("entropy decode alone, %2d threads: median %.2f ms per %d frames "
                         "(min %.2f)" % (threads, statistics.median(t), len(sel), min(t)))
            dec = MjpegDecoder(dev, dtype=dtype, threads=threads)
            vid, _ = dec.probe(path)
            for _ in range(5):
                dec.decode(vid, starts, out=out)
            torch.cuda.synchronize()
            call, total = [], []
            for _ in range(reqs):
                t0 = time.perf_counter()
                dec.decode(vid, starts, out=out)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                call.append((t1 - t0) * 1e3)
                total.append((t2 - t0) * 1e3)
            med = statistics.median(call)
            lines.append("MjpegDecoder.decode threads=%-2d %s: host call median %.3f ms (min %.3f, "
                         "max %.3f), call + sync median %.3f ms, %d requests of %d clips: "
                         "%.0f videos/s from one loader process"
                         % (threads, str(dtype).split(".")[1], med, min(call), max(call),
                            statistics.median(total), reqs, CLIPS, 1e3 / med))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--requests", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_decode_bench: needs a GPU")
    dev = torch.device("cuda:0")
    lines = ["mjpeg decode path, per 15-clip request at %dx%d -> 112x112 (%s)"
             % (W, H, torch.cuda.get_device_name(0))]
    encoded = encode(75)
    for dtype in (torch.float32, torch.bfloat16):
        kernels(dev, dtype, encoded, args.reps, args.rounds, lines)
    host(dev, torch.float32, encoded, args.requests, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
