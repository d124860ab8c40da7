"""Write a ``root/label/video.mjpeg`` tree of synthetic videos for the mjpeg decoder.

The frames are smooth moving gradients with a little deterministic noise
(random pixels, as ``make_y4m_dataset.py`` writes them, do not compress),
encoded with ``utils/mjpeg.write_mjpeg`` (baseline, Annex K tables; 4:2:0, or
4:2:2 / 4:4:4 with ``--sampling``), so

    python scripts/make_mjpeg_dataset.py /tmp/mjpeg --videos 8 --frames 120
    RNB_VIDEO_ROOT=/tmp/mjpeg python benchmark.py -c configs/r2p1d-whole-mjpeg.json -v 100

runs the compressed-file loader without any outside data or imaging library.
The encoder is plain numpy: about 0.1 s per 340x256 frame.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from rnb_amd.ops import video as vops  # noqa: E402
from rnb_amd.utils.mjpeg import SAMPLINGS, chroma_size, write_mjpeg  # noqa: E402


def synthetic_frames(vid: int, frames: int, W: int, H: int, noise: int = 6,
                     sampling: str = "420"):
    """``frames`` frames (Y, U, V uint8 arrays) of synthetic video ``vid``; the
    chroma planes have the size of ``sampling``."""
    rng = np.random.default_rng(vid)
    cw, ch = chroma_size(W, H, sampling)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = np.mgrid[0:ch, 0:cw].astype(np.float64)
    fx, fy, ph = rng.uniform(0.01, 0.06, 3)
    out = []
    for f in range(frames):
        t = 0.15 * f + vid
        y = 128 + 90 * np.sin(fx * xx + t) * np.cos(fy * yy - 0.5 * t) \
            + rng.integers(-noise, noise + 1, (H, W))
        u = 128 + 60 * np.sin(2 * fy * cx + ph + 0.3 * t) + 0 * cy
        v = 128 + 60 * np.cos(2 * fx * cy - ph - 0.2 * t) + 0 * cx
        out.append(tuple(np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in (y, u, v)))
    return out


def make_dataset(root: str, videos: int, frames: int, W: int, H: int, labels: int = 2,
                 quality: int = 75, restart_interval: int = 0, sampling: str = "420"):
    """Returns the paths written: ``root/label<k>/video<i>.mjpeg``."""
    paths = []
    for i in range(videos):
        ldir = os.path.join(root, "label%d" % (i % max(1, labels)))
        os.makedirs(ldir, exist_ok=True)
        path = os.path.join(ldir, "video%04d.mjpeg" % i)
        write_mjpeg(path, synthetic_frames(i, frames, W, H, sampling=sampling), quality=quality,
                    restart_interval=restart_interval, sampling=sampling)
        paths.append(path)
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("root")
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--width", type=int, default=vops.SOURCE_W)
    ap.add_argument("--height", type=int, default=vops.SOURCE_H)
    ap.add_argument("--labels", type=int, default=2)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--restart-interval", type=int, default=0, help="in MCUs; 0: none")
    ap.add_argument("--sampling", choices=SAMPLINGS, default="420")
    args = ap.parse_args()
    paths = make_dataset(args.root, args.videos, args.frames, args.width, args.height,
                         args.labels, args.quality, args.restart_interval, args.sampling)
    size = sum(os.path.getsize(p) for p in paths)
    raw = len(paths) * args.frames * args.width * args.height * 3 // 2
    print("wrote %d videos (%dx%d, %s, %d frames each, %.1f MB, %.1fx smaller than raw 4:2:0) "
          "under %s" % (len(paths), args.width, args.height, ":".join(args.sampling), args.frames,
                        size / 1e6, raw / max(size, 1), args.root))


if __name__ == "__main__":
    main()
