"""Write a ``root/label/video.y4m`` tree of synthetic videos for the y4m decoder.

The frames are ``vops.nv12gen``'s deterministic pixels (its CPU mirror),
de-interleaved from NV12 to the planar I420 a ``.y4m`` file holds, so

    python scripts/make_y4m_dataset.py /tmp/y4m --videos 8 --frames 120
    RNB_VIDEO_ROOT=/tmp/y4m python benchmark.py -c configs/r2p1d-whole-y4m.json -v 100

runs the file-reading loader without any outside data.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rnb_amd.ops import video as vops  # noqa: E402
from rnb_amd.utils.y4m import SAMPLING_FACTORS, write_y4m  # noqa: E402


def synthetic_frames(vid: int, frames: int, W: int, H: int, sampling: str = "420"):
    """``frames`` planar frames (Y, U, V uint8 arrays) of synthetic video ``vid``:
    the synthetic NV12 generator's 4:2:0 frames, their chroma samples repeated
    along each axis that ``sampling`` does not subsample."""
    hs, vs = SAMPLING_FACTORS[sampling]
    out = []
    for s in range(0, frames, 8):                 # a few frames at a time: bounded memory
        k = min(8, frames - s)
        nv = vops.nv12gen(vid, [s], k, H, W, torch.device("cpu")).numpy()
        uv = nv[:, H:].reshape(k, H // 2, W // 2, 2)
        uv = uv.repeat(2 // vs, axis=1).repeat(2 // hs, axis=2)
        out.extend((nv[i, :H], uv[i, :, :, 0], uv[i, :, :, 1]) for i in range(k))
    return out


def make_dataset(root: str, videos: int, frames: int, W: int, H: int, labels: int = 2,
                 fps=(25, 1), sampling: str = "420"):
    """Returns the paths written: ``root/label<k>/video<i>.y4m``."""
    paths = []
    for i in range(videos):
        ldir = os.path.join(root, "label%d" % (i % max(1, labels)))
        os.makedirs(ldir, exist_ok=True)
        path = os.path.join(ldir, "video%04d.y4m" % i)
        write_y4m(path, synthetic_frames(i, frames, W, H, sampling), fps, sampling=sampling)
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
    ap.add_argument("--sampling", choices=tuple(SAMPLING_FACTORS), default="420")
    args = ap.parse_args()
    paths = make_dataset(args.root, args.videos, args.frames, args.width, args.height,
                         args.labels, sampling=args.sampling)
    size = sum(os.path.getsize(p) for p in paths)
    print("wrote %d videos (%dx%d, %s, %d frames each, %.1f MB) under %s"
          % (len(paths), args.width, args.height, ":".join(args.sampling), args.frames,
             size / 1e6, args.root))


if __name__ == "__main__":
    main()
