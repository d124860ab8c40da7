#!/usr/bin/env python
"""Time the video_scores kernel against the same result built from torch ops.

Per shape (videos x rows per video x classes), on one stream, alternating the
two sides round by round: microseconds per call from device events around
``--calls`` back-to-back calls, after a warm-up of both. The torch side is what
the tree offered before the kernel: ``torch.softmax``, a per-video mean and a
stable descending sort cut at k (three or more launches, and ``torch.sort``
where a fixed tie rule is wanted). Writes the table to ``--out`` (default
profiles/video_scores.txt) and prints it. Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rnb_amd.ops import video as vops  # noqa: E402

SHAPES = ((64, 45, 400), (1, 30, 400))


def torch_scores(logits, nvid, rows, k):
    mean = torch.softmax(logits, dim=1).view(nvid, rows, -1).mean(dim=1)
    val, idx = torch.sort(mean, dim=1, descending=True, stable=True)
    return mean, val[:, :k], idx[:, :k]


def time_calls(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_scores.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("video_scores_bench: no GPU visible; a CPU run gives no timing")
    dev = torch.device("cuda:0")
    k = args.top_k
    lines = ["video_scores kernel vs torch.softmax + per-video mean + stable sort, top-%d" % k,
             "us per call, device events around %d calls, %d alternating rounds: min / median"
             % (args.calls, args.rounds),
             "%-22s %-20s %-20s %s" % ("videos x rows x cls", "kernel", "torch ops", "faster")]
    for nvid, rows, ncls in SHAPES:
        gen = torch.Generator().manual_seed(nvid * rows)
        logits = (torch.randn(nvid * rows, ncls, generator=gen) * 3).to(dev)
        off = torch.arange(0, nvid * rows + 1, rows, dtype=torch.int32, device=dev)
        out = (torch.empty((nvid, ncls), device=dev), torch.empty((nvid, k), device=dev),
               torch.empty((nvid, k), dtype=torch.int32, device=dev))
        sides = {"kernel": lambda: vops.video_scores(logits, off, top_k=k, out=out),
                 "torch": lambda: torch_scores(logits, nvid, rows, k)}
        # same answer first (ties aside: random logits have none at this size)
        sc, _, ti = sides["kernel"]()
        mean, _, idx = sides["torch"]()
        assert torch.equal(ti.long(), idx), "kernel and torch ops disagree on the top-k"
        assert (sc - mean).abs().max().item() < 1e-6
        for fn in sides.values():
            time_calls(fn, 200)
        took = {name: [] for name in sides}
        for _ in range(args.rounds):
            for name, fn in sides.items():
                took[name].append(time_calls(fn, args.calls))
        stat = {n: (min(t), sorted(t)[len(t) // 2]) for n, t in took.items()}
        lines.append("%-22s %-20s %-20s %s" % (
            "%d x %d x %d" % (nvid, rows, ncls),
            "%.1f / %.1f" % stat["kernel"], "%.1f / %.1f" % stat["torch"],
            "kernel" if stat["kernel"][1] < stat["torch"][1] else "torch ops"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
