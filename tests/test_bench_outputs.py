"""bench.py ``--full`` / ``--dump-outputs`` and repeatable inputs (CPU)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_plain_run_drops_everything_but_the_headline():
    """Without --full: no latency phases, numerics check or extra runs, even
    when their own options ask for them; --full keeps the defaults."""
    plain = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1",
                              "--latency-seconds", "5"])
    assert plain.steps == 3 and plain.warmup == 1 and not plain.full
    assert plain.latency_seconds == 0
    assert not (plain.check or plain.literal or plain.cross_gpu_extras)
    full = bench.parse_args(["--full"])
    assert full.full and full.latency_seconds == 3.0
    assert full.check and full.literal and full.cross_gpu_extras
    assert bench.parse_args(["--full", "--no-check"]).check is False
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"


def test_loader_config_carries_the_sample_seed():
    for pipe in ("aggressive", "global", "whole", "rnb", "segment"):
        cfg = bench.pipeline_config(bench.parse_args(["--pipeline", pipe, "--seed", "77"]), 1)
        assert cfg["pipeline"][0]["model"] == bench.LOADER == "bench.SeededLoader"
        assert cfg["pipeline"][0]["sample_seed"] == 77
        assert cfg["pipeline"][1]["model"] != bench.DUMP_RUNNER
    cfg = bench.pipeline_config(bench.parse_args(["--dump-outputs", "d"]), 1)
    assert cfg["pipeline"][1]["model"] == bench.DUMP_RUNNER


def test_plugins_load_by_their_config_paths():
    """The loader / runner processes resolve bench.<plugin> like any model."""
    from rnb_amd.models.r2p1d.model import R2P1DLoader, R2P1DRunner
    from rnb_amd.utils.class_utils import load_class
    assert issubclass(load_class(bench.LOADER), R2P1DLoader)
    assert issubclass(load_class(bench.DUMP_RUNNER), R2P1DRunner)


def test_work_root_falls_back_when_the_checkout_is_not_writable(tmp_path):
    """A run writes under logs/ of the checkout only when it can create and
    replace files there (files another user left, a read-only tree)."""
    import stat
    root = tmp_path / "co"
    root.mkdir()
    assert bench.work_root(str(root)) == str(root / "logs")
    left = root / "logs" / "bench" / "old.json"
    left.write_text("{}")
    left.chmod(stat.S_IRUSR)
    if os.access(left, os.W_OK):                 # root may write anything
        return
    other = bench.work_root(str(root))
    assert not other.startswith(str(root)) and os.path.isdir(os.path.join(other, "bench"))


def test_sample_seed_makes_a_videos_clips_independent_of_the_loader():
    """Two loaders with one sample_seed sample every video alike whatever
    they sampled before; the clip-count mix stays the sampler's (1 w.p. 10/11,
    15 w.p. 1/11)."""
    import torch
    cpu = torch.device("cpu")
    a = bench.SeededLoader(cpu, dtype="fp32", warmup=0, sample_seed=1234)
    b = bench.SeededLoader(cpu, seed=5, dtype="fp32", warmup=0, sample_seed=1234)
    c = bench.SeededLoader(cpu, dtype="fp32", warmup=0, sample_seed=1235)
    paths = ["synthetic://%d?frames=%d" % (i, 250 + i % 51) for i in range(4400)]
    sa = [a._sample(p)[1] for p in paths]
    sb = [b._sample(p)[1] for p in reversed(paths)][::-1]
    assert sa == sb
    assert [c._sample(p)[1] for p in paths] != sa
    assert {len(s) for s in sa} == {1, 15}
    large = sum(len(s) == 15 for s in sa)
    # 4400 / 11 = 400 expected, standard deviation 19: within 4 of them
    assert abs(large - 400) <= 76, large


def test_write_outputs_is_float32_and_capped(tmp_path, monkeypatch):
    rng = np.random.default_rng(0)
    arrays = {"a": rng.standard_normal((100, 8)), "b": rng.standard_normal((10, 4))}
    info = bench.write_outputs(str(tmp_path / "o"), arrays, seed=1)
    a = np.load(tmp_path / "o" / "a.npy")
    assert a.dtype == np.float32 and a.shape == (100, 8)
    assert np.array_equal(a, arrays["a"].astype(np.float32))
    assert info["a"] == {"shape": [100, 8], "rows_of": 100}
    # over the cap: the same seeded sample of rows every time, in order
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 40 * 8 * 4)
    bench.write_outputs(str(tmp_path / "p"), arrays, seed=1)
    bench.write_outputs(str(tmp_path / "q"), arrays, seed=1)
    p, q = np.load(tmp_path / "p" / "a.npy"), np.load(tmp_path / "q" / "a.npy")
    assert p.shape == (40, 8) and np.array_equal(p, q)
    rows = [int(np.flatnonzero((a == r).all(axis=1))[0]) for r in p]
    assert rows == sorted(set(rows))
    assert np.load(tmp_path / "p" / "b.npy").shape == (10, 4)
    total = sum(os.path.getsize(tmp_path / "p" / f) for f in os.listdir(tmp_path / "p"))
    assert total <= bench.DUMP_MAX_BYTES + 2 * 128          # .npy headers


def test_two_pipeline_runs_dump_the_same_last_step(tmp_path):
    """The launcher path bench.py drives (client, 2 loader and 2 runner
    processes, CPU): with a sample_seed two runs serve the same clips, and
    the runners' dumps of requests 9..12 join to the same logits."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = "rnb_amd.models.r2p1d.model."
    cfg = {"video_path_iterator": m + "R2P1DVideoPathIterator",
           "defaults": {"depth": 10, "num_clips_population": [1, 3],
                        "num_clips_weights": [2, 1], "warmup": 0},
           "pipeline": [
               {"model": bench.LOADER, "sample_seed": 5, "num_shared_tensors": 6,
                "queue_groups": [{"gpus": [-1, -1], "out_queues": [0]}]},
               {"model": bench.DUMP_RUNNER, "max_clips": 6, "max_batch_videos": 2,
                "queue_groups": [{"gpus": [-1, -1], "in_queue": 0}]}]}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    outs = []
    for run in ("a", "b"):
        parts = tmp_path / run / "parts"
        parts.mkdir(parents=True)
        env = dict(os.environ, RNB_NO_TQDM="1", RNB_CPU_THREADS="1", PYTHONPATH=root,
                   RNB_DUMP_DIR=str(parts), RNB_DUMP_IDS="9,12")
        proc = subprocess.run(
            [sys.executable, os.path.join(root, "benchmark.py"), "-c",
             str(tmp_path / "cfg.json"), "--log-root", str(tmp_path / run / "logs"),
             "--barrier-timeout", "200", "-mi", "0", "-v", "8", "--warmup-videos", "4"],
            capture_output=True, text=True, timeout=240, env=env)
        assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
        info = bench.merge_dump(argparse.Namespace(dump_outputs=str(tmp_path / run), seed=0),
                                str(parts))
        assert info["videos"] == 4, info
        outs.append((np.load(tmp_path / run / "logits.npy"),
                     np.load(tmp_path / run / "video_logits.npy")))
    (la, va), (lb, vb) = outs
    assert la.shape == lb.shape and va.shape == vb.shape == (4, 400)
    # same clips, same weights; only the batching of a call may differ (fp32
    # summation order: 1e-4 of the largest logit is far above it)
    assert np.abs(la - lb).max() <= 1e-4 * np.abs(la).max()
    assert np.abs(va - vb).max() <= 1e-4 * np.abs(va).max()


def test_runner_dump_and_merge(tmp_path, monkeypatch):
    """RNB_DUMP_DIR / RNB_DUMP_IDS: a final-layer DumpingRunner keeps the logits of
    the named requests only and writes them when it ends; bench.merge_dump
    joins the parts in request order."""
    import torch
    from rnb_amd.timecard import TimeCard, TimeCardList
    parts = tmp_path / "out" / "parts"
    parts.mkdir(parents=True)
    monkeypatch.setenv("RNB_DUMP_DIR", str(parts))
    monkeypatch.setenv("RNB_DUMP_IDS", "4,6")
    cpu = torch.device("cpu")
    loader = bench.SeededLoader(cpu, dtype="fp32", warmup=0, sample_seed=2)
    runner = bench.DumpingRunner(cpu, depth=10, bn_mode="batch", dtype="fp32", warmup=0,
                         max_clips=48, use_graphs=False, autotune=False)
    want = {}
    for call in ([6, 3, 4], [5, 2]):             # ids 2 and 3 are not dumped
        cards, frames = [], []
        for rid in call:
            (f,), _, tc = loader(None, "synthetic://%d?frames=270" % rid, TimeCard(rid))
            cards.append(tc)
            frames.append(f)
        rows = [f.shape[0] for f in frames]
        (y,), _, _ = runner((torch.cat(frames),), None, TimeCardList(cards, rows))
        off = 0
        for rid, n in zip(call, rows):
            want[rid] = y[off:off + n].detach().numpy().copy()
            off += n
    runner.runtime_stats()                        # runner.py calls it after its loop
    assert len(list(parts.glob("part_p*.npz"))) == 1
    args = argparse.Namespace(dump_outputs=str(tmp_path / "out"), seed=0)
    info = bench.merge_dump(args, str(parts))
    assert info["videos"] == 3 and not parts.exists()
    logits = np.load(tmp_path / "out" / "logits.npy")
    videos = np.load(tmp_path / "out" / "video_logits.npy")
    assert logits.dtype == np.float32 and videos.dtype == np.float32
    assert np.array_equal(logits, np.concatenate([want[4], want[5], want[6]]))
    assert videos.shape == (3, logits.shape[1])
    for i, rid in enumerate((4, 5, 6)):
        assert np.allclose(videos[i], want[rid].sum(axis=0), rtol=1e-6, atol=1e-6)
    assert "error" in bench.merge_dump(args, str(parts))      # nothing kept
