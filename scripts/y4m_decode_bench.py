"""Time the y4m decode path per 15-clip request at 340x256 (GPU required).

  * kernel: ``yuv420_clip_kernel`` on I420 frames behind FRAME markers next to
    ``nv12_clip_kernel`` on the same pixels as NV12, alternating, device events
    around ``--reps`` back-to-back launches per round;
  * host: ``Y4mDecoder.decode`` next to ``NpyDecoder.decode`` on files written
    to a temporary directory and read once before (warm page cache): time of
    the call itself, and of the call plus a device synchronise.

    python scripts/y4m_decode_bench.py --out profiles/y4m_decode.txt

``--filter antialias`` times ``yuv420_clip_aa_kernel`` next to the bilinear
``yuv420_clip_kernel`` on the same I420 buffer instead (alternating, one
process; the ratio is reported) and ``Y4mDecoder(filter="antialias")`` on the
host side. ``--size WxH`` and ``--clips N`` change that request, e.g.
``--size 1920x1080 --clips 1``. Without ``--filter antialias`` the script runs
and prints what it always did.

``--short-side S [--views V]`` times the short-side resize + window protocol
instead (``crop={"short_side": S, "views": V}``), for both filters: the clip
launch (``rnb_yuv_to_clip_boxes``, the only one) through ``yuv420_to_clip`` at
``--clips`` rows with one crop box ("one box": the op repeats it per row), at
the same rows with that box given as a per-row list ("boxed") and at
``clips * V`` rows with the views' boxes, then ``Y4mDecoder.decode`` (host call,
call + sync, sustained requests/s, uploaded bytes per request) for 1 view and
for ``V``.

``--frame-step N`` or ``--fps R`` times ``Y4mDecoder.decode(step=)`` instead:
the clips of the request at every N-th frame, or at ``R`` frames per second of
a 30 fps file (host call, call + sync, sustained requests/s), and next to it
the staging copies alone, one span per clip against F frames per clip. ``--size``,
``--clips`` and ``--filter`` apply; ``--frame-step 1`` is the contiguous path.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rnb_amd.models.r2p1d.decoder import NpyDecoder, Y4mDecoder  # noqa: E402
from rnb_amd.ops import video as vops  # noqa: E402
from rnb_amd.utils import y4m  # noqa: E402

W, H, F, CLIPS = vops.SOURCE_W, vops.SOURCE_H, 8, 15


SAMPLING = "420"       # --sampling: the chroma layout of the frames timed
PLANES = {"420": vops.i420_planes, "422": vops.i422_planes, "444": vops.i444_planes}


def chroma_shape(w, h):
    hs, vs = y4m.SAMPLING_FACTORS[SAMPLING]
    return h // vs, w // hs


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernels(dev, dtype, reps, rounds, lines):
    rng = np.random.default_rng(0)
    stride = 6 + vops.nv12_frame_bytes(W, H)
    i420 = torch.from_numpy(rng.integers(0, 256, (CLIPS * F, stride), dtype=np.uint8))
    y = i420[:, 6:6 + W * H].reshape(-1, H, W)
    u = i420[:, 6 + W * H:6 + W * H * 5 // 4].reshape(-1, H // 2, W // 2)
    v = i420[:, 6 + W * H * 5 // 4:].reshape(-1, H // 2, W // 2)
    nv = torch.cat([y, torch.stack([u, v], dim=-1).reshape(-1, H // 2, W)], dim=1).contiguous()
    buf, nvd = i420.reshape(-1).to(dev), nv.to(dev)
    offs = [c * F * stride for c in range(CLIPS)]
    C = 4 if dtype == torch.float32 else 8
    out = torch.empty((CLIPS, F, 112, 112, C), dtype=dtype, device=dev)
    planes = vops.i420_planes(W, H, 6)

    def new():
        vops.yuv420_to_clip(buf, offs, F, W, H, stride, planes, dtype=dtype, out=out)

    def old():
        vops.nv12_to_clip(nvd, W, H, dtype=dtype, out=out)
    new()
    a = out.clone()
    old()
    diff = (a.float() - out.float()).abs().max().item()
    for fn in (new, old):
        event_ms(fn, reps)                                # warm
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(event_ms(new, reps))
        t_old.append(event_ms(old, reps))
    src = CLIPS * F * stride
    dst = out.numel() * out.element_size()
    for name, t in (("yuv420_clip_kernel", t_new), ("nv12_clip_kernel  ", t_old)):
        med = statistics.median(t)
        lines.append("%s %s: median %.2f us/launch (min %.2f, max %.2f over %d rounds of %d); "
                     "%.0f GB/s of %d source + %d output bytes"
                     % (name, str(dtype).split(".")[1], med * 1e3, min(t) * 1e3, max(t) * 1e3,
                        rounds, reps, (src + dst) / med / 1e6, src, dst))
    lines.append("max |yuv420 - nv12| on the same pixels: %g" % diff)


def kernels_antialias(dev, dtype, reps, rounds, lines, w, h, clips):
    """``yuv420_clip_aa_kernel`` next to ``yuv420_clip_kernel`` on ``clips``
    clips of random ``w`` x ``h`` planar frames of ``SAMPLING`` behind FRAME markers."""
    rng = np.random.default_rng(0)
    stride = 6 + y4m.payload_bytes(w, h, SAMPLING)
    buf = torch.from_numpy(rng.integers(0, 256, clips * F * stride, dtype=np.uint8)).to(dev)
    offs = [c * F * stride for c in range(clips)]
    C = 4 if dtype == torch.float32 else 8
    out = torch.empty((clips, F, 112, 112, C), dtype=dtype, device=dev)
    planes = PLANES[SAMPLING](w, h, 6)

    def antialias():
        vops.yuv420_to_clip(buf, offs, F, w, h, stride, planes, dtype=dtype, out=out,
                            filter="antialias", sampling=SAMPLING)

    def bilinear():
        vops.yuv420_to_clip(buf, offs, F, w, h, stride, planes, dtype=dtype, out=out,
                            sampling=SAMPLING)
    for fn in (antialias, bilinear):
        event_ms(fn, reps)                                # warm
    t_aa, t_bil = [], []
    for _ in range(rounds):
        t_aa.append(event_ms(antialias, reps))
        t_bil.append(event_ms(bilinear, reps))
    src = clips * F * stride
    dst = out.numel() * out.element_size()
    name = str(dtype).split(".")[1]
    for kernel, t in (("yuv420_clip_aa_kernel", t_aa), ("yuv420_clip_kernel   ", t_bil)):
        med = statistics.median(t)
        lines.append("%s %s: median %.2f us/launch (min %.2f, max %.2f over %d rounds of %d); "
                     "%.0f GB/s of %d source + %d output bytes"
                     % (kernel, name, med * 1e3, min(t) * 1e3, max(t) * 1e3, rounds, reps,
                        (src + dst) / med / 1e6, src, dst))
    lines.append("antialias / bilinear kernel time %s: %.2f"
                 % (name, statistics.median(t_aa) / statistics.median(t_bil)))


def host_antialias(dev, dtype, reqs, lines, w, h, clips):
    """Host time of ``Y4mDecoder(filter="antialias").decode`` for ``clips`` clips
    20 frames apart in a ``w`` x ``h`` file (warm page cache)."""
    rng = np.random.default_rng(1)
    starts = [20 * c for c in range(clips)]
    frames = min(300, starts[-1] + F + 4)              # 1080p: do not write 300 frames
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.y4m")
        y4m.write_y4m(path, [(rng.integers(0, 256, (h, w), dtype=np.uint8),
                              rng.integers(0, 256, chroma_shape(w, h), dtype=np.uint8),
                              rng.integers(0, 256, chroma_shape(w, h), dtype=np.uint8))
                             for _ in range(frames)], sampling=SAMPLING)
        with open(path, "rb") as fp:                       # warm the page cache
            while fp.read(1 << 24):
                pass
        C = 4 if dtype == torch.float32 else 8
        out = torch.empty((clips, F, 112, 112, C), dtype=dtype, device=dev)
        dec = Y4mDecoder(dev, dtype=dtype, filter="antialias")
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
        lines.append("Y4mDecoder.decode (%dx%d y4m, antialias) %s: host call median %.3f ms "
                     "(min %.3f, max %.3f), call + sync median %.3f ms, %d requests of %d clips"
                     % (w, h, str(dtype).split(".")[1], statistics.median(call), min(call),
                        max(call), statistics.median(total), reqs, clips))


def views_kernels(dev, dtype, reps, rounds, lines, w, h, clips, short_side, nviews):
    """The clip launch at ``clips`` rows with one box, at ``clips`` rows with a
    per-row list of that box (the centre box repeated) and at ``clips * nviews``
    rows (each clip through every view's box, one uploaded span per clip), both
    filters, alternating."""
    from rnb_amd.models.r2p1d.decoder import view_boxes
    rng = np.random.default_rng(0)
    stride = 6 + y4m.payload_bytes(w, h, SAMPLING)
    buf = torch.from_numpy(rng.integers(0, 256, clips * F * stride, dtype=np.uint8)).to(dev)
    offs = [c * F * stride for c in range(clips)]
    C = 4 if dtype == torch.float32 else 8
    out = torch.empty((clips * nviews, F, 112, 112, C), dtype=dtype, device=dev)
    planes = PLANES[SAMPLING](w, h, 6)
    centre = view_boxes(w, h, 112, 112, short_side, 1)[0]
    vb = view_boxes(w, h, 112, 112, short_side, nviews)
    name = str(dtype).split(".")[1]
    for filt in vops.FILTERS:
        def run(offsets, crop):
            return lambda: vops.yuv420_to_clip(buf, offsets, F, w, h, stride, planes, dtype=dtype,
                                               out=out[:len(offsets)], crop=crop, filter=filt,
                                               sampling=SAMPLING)
        cases = [("one box, %d rows" % clips, run(offs, centre)),
                 ("boxed, %d rows, one box repeated" % clips, run(offs, [centre] * clips)),
                 ("boxed, %d rows, %d views" % (clips * nviews, nviews),
                  run([o for o in offs for _ in range(nviews)], vb * clips))]
        times = [[] for _ in cases]
        for _, fn in cases:
            event_ms(fn, reps)                            # warm
        for _ in range(rounds):
            for t, (_, fn) in zip(times, cases):
                t.append(event_ms(fn, reps))
        for (what, _), t in zip(cases, times):
            lines.append("clip kernel %s %s, %s: median %.2f us/launch (min %.2f, max %.2f over %d "
                         "rounds of %d)" % (filt, name, what, statistics.median(t) * 1e3,
                                            min(t) * 1e3, max(t) * 1e3, rounds, reps))


def views_host(dev, dtype, reqs, lines, w, h, clips, short_side, nviews):
    """``Y4mDecoder.decode`` with 1 view and with ``nviews``: host call, call +
    sync, sustained requests/s of one loader, staged bytes per request."""
    rng = np.random.default_rng(1)
    starts = [20 * c for c in range(clips)]
    frames = starts[-1] + F + 4
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.y4m")
        y4m.write_y4m(path, [(rng.integers(0, 256, (h, w), dtype=np.uint8),
                              rng.integers(0, 256, chroma_shape(w, h), dtype=np.uint8),
                              rng.integers(0, 256, chroma_shape(w, h), dtype=np.uint8))
                             for _ in range(frames)], sampling=SAMPLING)
        with open(path, "rb") as fp:                       # warm the page cache
            while fp.read(1 << 24):
                pass
        C = 4 if dtype == torch.float32 else 8
        for filt in vops.FILTERS:
            for v in sorted({1, nviews}):
                out = torch.empty((clips * v, F, 112, 112, C), dtype=dtype, device=dev)
                dec = Y4mDecoder(dev, dtype=dtype, filter=filt,
                                 crop={"short_side": short_side, "views": v})
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
                t0 = time.perf_counter()
                for _ in range(reqs):
                    dec.decode(vid, starts, out=out)
                torch.cuda.synchronize()
                rate = reqs / (time.perf_counter() - t0)
                hdr = dec._videos[vid][1]
                lines.append("Y4mDecoder.decode %s, %d view(s), %d rows %s: host call median %.3f ms "
                             "(min %.3f, max %.3f), call + sync median %.3f ms, sustained %.0f "
                             "requests/s, %d bytes uploaded per request"
                             % (filt, v, clips * v, str(dtype).split(".")[1],
                                statistics.median(call), min(call), max(call),
                                statistics.median(total), rate, clips * F * hdr.frame_stride))


def step_host(dev, dtype, reqs, lines, w, h, clips, filt, frame_step, fps):
    """``Y4mDecoder.decode(step=)`` on ``clips`` clips 20 * step frames apart in
    a 30 fps ``w`` x ``h`` file (warm page cache), and its staging copies alone."""
    from rnb_amd.models.r2p1d.sampler import clip_frames, clip_span, step_of
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "v.y4m")
        step = step_of(frame_step or 1, fps, (30, 1))
        span = clip_span(F, step)
        starts = [max(20, span) * c for c in range(clips)]
        frames = starts[-1] + span + 4
        y4m.write_y4m(path, [(rng.integers(0, 256, (h, w), dtype=np.uint8),
                              rng.integers(0, 256, chroma_shape(w, h), dtype=np.uint8),
                              rng.integers(0, 256, chroma_shape(w, h), dtype=np.uint8))
                             for _ in range(frames)], fps=(30, 1), sampling=SAMPLING)
        with open(path, "rb") as fp:                       # warm the page cache
            while fp.read(1 << 24):
                pass
        C = 4 if dtype == torch.float32 else 8
        out = torch.empty((clips, F, 112, 112, C), dtype=dtype, device=dev)
        dec = Y4mDecoder(dev, dtype=dtype, filter=filt)
        vid, _ = dec.probe(path)
        assert dec.source_fps_of(vid) == (30, 1)
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
        t0 = time.perf_counter()
        for _ in range(reqs):
            dec.decode(vid, starts, out=out, step=step)
        torch.cuda.synchronize()
        rate = reqs / (time.perf_counter() - t0)
        hdr = dec._videos[vid][1]
        lines.append("Y4mDecoder.decode %s, step %d/%d (span %d) %s: host call median %.3f ms "
                     "(min %.3f, max %.3f), call + sync median %.3f ms, sustained %.0f requests/s, "
                     "%d requests of %d clips, %d bytes uploaded per request"
                     % (filt, step[0], step[1], span, str(dtype).split(".")[1],
                        statistics.median(call), min(call), max(call), statistics.median(total),
                        rate, reqs, clips, clips * F * hdr.frame_stride))
        # the staging copies alone (no upload, no launch): where a step's host time goes
        _, data = dec._map(vid, path)
        fs = hdr.frame_stride
        pinned = torch.empty(clips * F * fs, dtype=torch.uint8, pin_memory=True).numpy()

        def one_span():
            for i, s in enumerate(starts):
                a = hdr.frame_offset(s)
                np.copyto(pinned[i * F * fs:(i + 1) * F * fs], data[a:a + F * fs])

        def per_frame():
            for i, s in enumerate(starts):
                dst = pinned[i * F * fs:(i + 1) * F * fs].reshape(F, fs)
                for f, fr in enumerate(clip_frames(s, F, step)):
                    a = hdr.frame_offset(fr)
                    np.copyto(dst[f], data[a:a + fs])
        for what, fn in (("one span per clip", one_span), ("F frames per clip", per_frame)):
            t = []
            for _ in range(reqs + 5):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            lines.append("staging copies alone, %s: median %.3f ms (min %.3f) per request of %d "
                         "bytes" % (what, statistics.median(t[5:]), min(t[5:]), clips * F * fs))


def host(dev, dtype, reqs, lines):
    rng = np.random.default_rng(1)
    frames = 300
    starts = [20 * c for c in range(CLIPS)]
    with tempfile.TemporaryDirectory() as d:
        py, pn = os.path.join(d, "v.y4m"), os.path.join(d, "v.npy")
        y4m.write_y4m(py, [(rng.integers(0, 256, (H, W), dtype=np.uint8),
                            rng.integers(0, 256, chroma_shape(W, H), dtype=np.uint8),
                            rng.integers(0, 256, chroma_shape(W, H), dtype=np.uint8))
                           for _ in range(frames)], sampling=SAMPLING)
        np.save(pn, rng.integers(0, 256, (frames, 112, 112, 3), dtype=np.uint8))
        for p in (py, pn):
            with open(p, "rb") as fp:                      # warm the page cache
                while fp.read(1 << 24):
                    pass
        C = 4 if dtype == torch.float32 else 8
        out = torch.empty((CLIPS, F, 112, 112, C), dtype=dtype, device=dev)
        for name, dec, path in (("Y4mDecoder.decode (340x256 y4m)", Y4mDecoder(dev, dtype=dtype), py),
                                ("NpyDecoder.decode (112x112 npy)", NpyDecoder(dev, dtype=dtype), pn)):
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
            lines.append("%s %s: host call median %.3f ms (min %.3f, max %.3f), call + sync "
                         "median %.3f ms, %d requests of %d clips"
                         % (name, str(dtype).split(".")[1], statistics.median(call), min(call),
                            max(call), statistics.median(total), reqs, CLIPS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--requests", type=int, default=40)
    ap.add_argument("--filter", choices=vops.FILTERS, default="bilinear")
    ap.add_argument("--size", default="%dx%d" % (W, H),
                    help="with --filter antialias: source WxH (even)")
    ap.add_argument("--clips", type=int, default=CLIPS, help="with --filter antialias")
    ap.add_argument("--sampling", choices=tuple(PLANES), default="420",
                    help="422 / 444: the clip kernels (both filters) and Y4mDecoder on C422 / "
                         "C444 frames")
    ap.add_argument("--short-side", type=float, default=None,
                    help="time crop={'short_side': S, 'views': V} (both filters) instead")
    ap.add_argument("--views", type=int, choices=(1, 3), default=1, help="with --short-side")
    ap.add_argument("--frame-step", type=int, default=None,
                    help="time Y4mDecoder.decode(step=(N, 1)) instead (1: the contiguous path)")
    ap.add_argument("--fps", default=None,
                    help="time Y4mDecoder.decode at this rate of a 30 fps file instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    global SAMPLING
    SAMPLING = args.sampling
    if not torch.cuda.is_available():
        raise SystemExit("y4m_decode_bench: needs a GPU")
    dev = torch.device("cuda:0")
    if args.frame_step is not None or args.fps is not None:
        w, h = (int(x) for x in args.size.lower().split("x"))
        lines = ["y4m decode path, sampling %s, frame step %s, fps %s, per %d-clip request at "
                 "%dx%d -> 112x112 (%s)" % (":".join(SAMPLING), args.frame_step, args.fps,
                                            args.clips, w, h, torch.cuda.get_device_name(0))]
        step_host(dev, torch.float32, args.requests, lines, w, h, args.clips, args.filter,
                  args.frame_step, args.fps)
    elif args.short_side is not None:
        w, h = (int(x) for x in args.size.lower().split("x"))
        lines = ["y4m decode path, sampling %s, short side %g, %d view(s), per %d-clip request at "
                 "%dx%d -> 112x112 (%s)" % (":".join(SAMPLING), args.short_side, args.views,
                                            args.clips, w, h, torch.cuda.get_device_name(0))]
        for dtype in (torch.float32, torch.bfloat16):
            views_kernels(dev, dtype, args.reps, args.rounds, lines, w, h, args.clips,
                          args.short_side, args.views)
        views_host(dev, torch.float32, args.requests, lines, w, h, args.clips, args.short_side,
                   args.views)
    elif args.filter == "antialias":
        w, h = (int(x) for x in args.size.lower().split("x"))
        lines = ["y4m decode path, sampling %s, filter antialias, per %d-clip request at %dx%d -> "
                 "112x112 (%s)" % (":".join(SAMPLING), args.clips, w, h,
                                   torch.cuda.get_device_name(0))]
        for dtype in (torch.float32, torch.bfloat16):
            kernels_antialias(dev, dtype, args.reps, args.rounds, lines, w, h, args.clips)
        host_antialias(dev, torch.float32, args.requests, lines, w, h, args.clips)
    else:
        lines = ["y4m decode path, sampling %s, per 15-clip request at %dx%d -> 112x112 (%s)"
                 % (":".join(SAMPLING), W, H, torch.cuda.get_device_name(0))]
        for dtype in (torch.float32, torch.bfloat16):
            if SAMPLING == "420":
                kernels(dev, dtype, args.reps, args.rounds, lines)
            else:                       # no NV12 twin to compare with: both filters' kernels
                kernels_antialias(dev, dtype, args.reps, args.rounds, lines, W, H, CLIPS)
        host(dev, torch.float32, args.requests, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
