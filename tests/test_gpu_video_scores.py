"""The video_scores HIP kernel (csrc/score_ops.hip) against video_reduce, its
own scores, the fp64 oracle (tests/score_oracle.py) and the torch mirror; then
through the aggregator on the GPU and the fused engine's bucket graph.

Measured on an MI355X (max |scores - fp64| over ACCURACY_CASES; the bound is
4x the mirror's distance, at least 16 * 2^-24 = 9.5e-07): see
profiles/video_scores.txt, which quotes this test's printed figures."""
import functools

import numpy as np
import pytest
import torch

import score_oracle as orc
from rnb_amd.ops import video as vops
from test_video_scores_cpu import aggregator_cases, run_arrival_forms

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL_FLOOR = 16 * 2.0 ** -24         # a few ulps of 1.0, the scale of a probability
# no one-row video here: its peak row alone is a one-hot, the other scores ~e^-30
ACC_ROWS = (0, 45, 3, 0, 130, 65, 0)
# fp64 top-5 gaps of these exceed the tolerance at this seed (asserted below)
ACCURACY_CASES = ((400, ACC_ROWS, 5), (1000, orc.ROWS_7B, 5), (65, ACC_ROWS, 5),
                  (4096, (130,), 5), (257, (64,), 5))
ACCURACY_SEED = 11


def _gpu(x, rows, kind, k):
    off = torch.tensor(orc.offsets_of(rows), dtype=torch.int32, device=DEV)
    return vops.video_scores(torch.tensor(x, device=DEV), off, scores=kind, top_k=k)


@functools.lru_cache(maxsize=None)
def _integer_case(ncls, rows, dup):
    """Small-integer logits (fp32 sums are exact), whole columns duplicated."""
    rng = np.random.RandomState(ncls * 7 + len(rows))
    x = rng.randint(-8, 9, size=(sum(rows), ncls)).astype(np.float32)
    if dup and ncls >= 3:
        x[:, ncls - 1] = x[:, 0]
        x[:, ncls // 2] = x[:, 0]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _accuracy_ref(ncls, rows, k, kind):
    """(input, fp64 scores, fp64 top_idx, the mirror's distance from fp64)."""
    x = orc.peaked_logits(rows, ncls, ACCURACY_SEED)
    x.setflags(write=False)
    want, _, wi = orc.video_scores(x, orc.offsets_of(rows), kind, k)
    mirror = vops.video_scores(torch.tensor(x), torch.tensor(orc.offsets_of(rows)),
                               scores=kind, top_k=k)[0].numpy().astype(np.float64)
    return x, want, wi, float(np.abs(mirror - want).max())


def test_logit_sum_is_exact_and_equals_video_reduce_bit_for_bit():
    for ncls, rows, k in orc.grid_cases():
        x = _integer_case(ncls, rows, True)
        sc, tv, ti = _gpu(x, rows, "logit_sum", k)
        off = orc.offsets_of(rows)
        want, wv, wi = orc.video_scores(x, off, "logit_sum", k)
        assert np.array_equal(sc.cpu().numpy().astype(np.float64), want), (ncls, rows)
        # ties (duplicated columns, and many equal small sums): lower index first
        assert np.array_equal(ti.cpu().numpy(), wi), (ncls, rows, k)
        assert np.array_equal(tv.cpu().numpy().astype(np.float64), wv)
        sums, arg = vops.video_reduce(torch.tensor(x, device=DEV),
                                      torch.tensor(off, dtype=torch.int32, device=DEV))
        assert torch.equal(sc.view(torch.int32), sums.view(torch.int32))
        assert torch.equal(ti[:, 0], arg)


def test_logit_sum_of_real_logits_equals_video_reduce_bit_for_bit():
    """Inexact sums: equal bits need the same row order in one accumulator."""
    for ncls, rows in ((400, orc.ROWS_7), (4096, (130,)), (1000, orc.ROWS_7B)):
        x = orc.peaked_logits(rows, ncls, 5)
        sc, _, ti = _gpu(x, rows, "logit_sum", 1)
        sums, arg = vops.video_reduce(
            torch.from_numpy(x).to(DEV),
            torch.tensor(orc.offsets_of(rows), dtype=torch.int32, device=DEV))
        assert torch.equal(sc.view(torch.int32), sums.view(torch.int32))
        assert torch.equal(ti[:, 0], arg)


@pytest.mark.parametrize("kind", orc.KINDS)
def test_top_k_is_consistent_with_the_kernels_own_scores(kind):
    for ncls, rows, k in orc.grid_cases():
        x = orc.peaked_logits(rows, ncls, seed=ncls + k)
        sc, tv, ti = _gpu(x, rows, kind, k)
        sc, tv, ti = sc.cpu(), tv.cpu(), ti.cpu()
        assert torch.isfinite(sc).all()
        for v, n in enumerate(rows):
            if n == 0:
                assert ti[v].tolist() == [-1] * k and tv[v].tolist() == [0.0] * k
                assert not sc[v].any()
                continue
            order = torch.sort(sc[v], descending=True, stable=True)[1][:k]
            assert ti[v].tolist() == order.tolist(), (ncls, rows, k, v)
            assert torch.equal(tv[v].view(torch.int32), sc[v][order].view(torch.int32))


@pytest.mark.parametrize("kind", ["softmax_sum", "softmax_mean", "logit_mean"])
def test_scores_are_as_close_to_fp64_as_the_mirror(kind):
    for ncls, rows, k in ACCURACY_CASES:
        x, want, wi, mirror_err = _accuracy_ref(ncls, rows, k, kind)
        tol = max(4 * mirror_err, TOL_FLOOR)
        sc, _, ti = _gpu(x, rows, kind, k)
        err = float(np.abs(sc.cpu().numpy().astype(np.float64) - want).max())
        print("video_scores %-12s ncls %4d rows %-28s kernel %.3e mirror %.3e tol %.3e"
              % (kind, ncls, rows, err, mirror_err, tol))
        assert err <= tol, (kind, ncls, rows, err, mirror_err)
        nonempty = [v for v, n in enumerate(rows) if n]
        assert orc.top_gap(want[nonempty], k) > 2 * tol, "seed: fp64 top-k too close to call"
        assert np.array_equal(ti.cpu().numpy(), wi), (kind, ncls, rows)


def test_extreme_rows_give_finite_scores_summing_to_one():
    ncls = 400
    rng = np.random.RandomState(2)
    spread = rng.rand(3, ncls).astype(np.float32) * 1e4      # spread 1e4: a one-hot each
    spread[0] -= 1e4
    equal = np.repeat(np.array([[0.0], [1e4], [-1e4], [7.5]], dtype=np.float32), ncls, axis=1)
    mixed = np.concatenate([spread[:2], equal[:3]])
    x = np.concatenate([spread, equal, mixed])
    rows = (3, 4, 5)
    sc, tv, ti = _gpu(x, rows, "softmax_mean", 5)
    got = sc.cpu().numpy().astype(np.float64)
    want = orc.video_scores(x, orc.offsets_of(rows), "softmax_mean", 5)[0]
    mirror = vops.video_scores(torch.from_numpy(x), torch.tensor(orc.offsets_of(rows)))[0]
    tol = max(4 * float(np.abs(mirror.numpy().astype(np.float64) - want).max()), TOL_FLOOR)
    assert np.isfinite(got).all() and torch.isfinite(tv).all()
    assert np.abs(got - want).max() <= tol
    assert np.abs(got.sum(axis=1) - 1.0).max() <= tol
    assert ti[1].tolist() == [0, 1, 2, 3, 4]                 # all equal: index order


def test_two_launches_give_equal_bits():
    x = orc.peaked_logits(orc.ROWS_7, 1000, 4)
    a = _gpu(x, orc.ROWS_7, "softmax_mean", 16)
    b = _gpu(x, orc.ROWS_7, "softmax_mean", 16)
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))


def test_graph_capture_replays_on_new_logits_and_offsets():
    ncls, k, nvid = 400, 5, 7
    x0 = orc.peaked_logits(orc.ROWS_7, ncls, 1)
    nrows = sum(orc.ROWS_7)
    logits = torch.from_numpy(x0).to(DEV)
    off = torch.tensor(orc.offsets_of(orc.ROWS_7), dtype=torch.int32, device=DEV)
    out = (torch.empty((nvid, ncls), device=DEV), torch.empty((nvid, k), device=DEV),
           torch.empty((nvid, k), dtype=torch.int32, device=DEV))
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        vops.video_scores(logits, off, top_k=k, out=out)        # warm-up outside capture
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            vops.video_scores(logits, off, top_k=k, out=out)
        stream.synchronize()
    # other rows, other ranges (same row total or fewer), in place
    rows2 = (40, 0, 0, 101, 7, 1, 60)
    assert sum(rows2) <= nrows
    x1 = orc.peaked_logits((nrows,), ncls, 9)
    logits.copy_(torch.from_numpy(x1))
    off.copy_(torch.tensor(orc.offsets_of(rows2), dtype=torch.int32))
    for t in out:
        t.zero_()
    torch.cuda.synchronize(DEV)
    graph.replay()
    torch.cuda.synchronize(DEV)
    eager = vops.video_scores(logits, off, top_k=k)
    for p, q in zip(out, eager):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    assert eager[2][1].tolist() == [-1] * k


def test_errors_name_the_argument_and_launch_nothing():
    off = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="ncls"):
        vops.video_scores(torch.zeros(2, 4097, device=DEV), off, top_k=1)
    with pytest.raises(ValueError, match=r"\bk\b"):
        vops.video_scores(torch.zeros(2, 400, device=DEV), off, top_k=17)
    with pytest.raises(ValueError, match=r"\bk\b"):
        vops.video_scores(torch.zeros(2, 3, device=DEV), off, top_k=5)
    # the kernel entry's own codes (the op checks k first only for its range)
    from rnb_amd.ops.native import kernels
    z = torch.zeros(2, 4, device=DEV)
    ti = torch.full((1, 4), 7, dtype=torch.int32, device=DEV)
    args = (z.data_ptr(), off.data_ptr(), 0, z.data_ptr(), ti.data_ptr(), 1)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    with pytest.raises(ValueError, match="ncls = 0"):
        kernels().video_scores(*args, 0, 1, 1, 1, stream)
    with pytest.raises(ValueError, match="k = 5"):
        kernels().video_scores(*args, 4, 5, 1, 1, stream)
    torch.cuda.synchronize(DEV)
    assert ti.tolist() == [[7] * 4]


def test_aggregator_on_the_gpu_equals_the_cpu_aggregator():
    rows, x, off = aggregator_cases()
    want = orc.video_scores(x, off, "softmax_mean", 5)[0]
    mirror = vops.video_scores(torch.from_numpy(x), torch.tensor(off))[0]
    tol = max(4 * float(np.abs(mirror.numpy().astype(np.float64) - want).max()), TOL_FLOOR)
    cpu = run_arrival_forms(torch.device("cpu"))
    gpu = run_arrival_forms(DEV)
    assert sorted(gpu) == ["batch", "segments", "single"]
    for name in gpu:
        for (gc, gs), (cc, cs) in zip(gpu[name], cpu[name]):
            assert gc == cc, name
            assert np.abs(np.array(gs) - np.array(cs)).max() <= tol, name
    assert gpu["batch"][1] == ((-1,) * 5, (0.0,) * 5)


def test_fused_engine_ends_in_video_scores():
    from rnb_amd.models.r2p1d.fused import FusedR2P1D
    f = FusedR2P1D(DEV, depth=18, replicas=1, max_clips=4, max_videos=3, buckets=(4,),
                   autotune=False, scores="softmax_mean", top_k=5)
    rep = f.replicas[0]
    videos = [(5, [0, 50]), (9, [3])]
    ev, top_idx, nvid = rep.submit(videos)
    ev.synchronize()
    assert nvid == 2 and tuple(top_idx.shape) == (2, 5) and top_idx.dtype == torch.int32
    bg = rep.graphs[4]
    assert bg.logits.dtype == torch.float32
    sc, tv, ti = vops.video_scores(bg.logits, bg.offsets, scores="softmax_mean", top_k=5)
    assert torch.equal(top_idx, ti[:2].cpu())
    assert torch.equal(rep.last_top_val.view(torch.int32), tv[:2].cpu().view(torch.int32))
    assert torch.equal(bg.sums.view(torch.int32), sc.view(torch.int32))
    assert ti[2].tolist() == [-1] * 5                  # the unused third video: empty
