"""Per-video scores on the CPU: the torch mirror of ``video_scores`` against the
fp64 oracle (tests/score_oracle.py), the aggregator's score modes, accuracy
counters and JSONL results, directory labels, and the two -eval configs."""
import json
import os

import numpy as np
import pytest
import torch

import score_oracle as orc
from rnb_amd.config import load_pipeline
from rnb_amd.models.r2p1d.model import R2P1DAggregator, R2P1DLoader
from rnb_amd.ops import video as vops
from rnb_amd.timecard import TimeCard, TimeCardList
from rnb_amd.video_path_provider import DirectoryLabels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
# fp32 mirror vs fp64: a score is a sum of <= 130 terms, each within a few ulps
# (softmax: exp and the row normalisation) of its fp64 value, so within
# 130 * 8 * 2^-24 of the score's scale, the largest |score| of the case
MIRROR_RTOL = 130 * 8 * 2.0 ** -24


def _mirror(x, rows, kind, k):
    return vops.video_scores(torch.from_numpy(x), torch.tensor(orc.offsets_of(rows)),
                             scores=kind, top_k=k)


@pytest.mark.parametrize("kind", orc.KINDS)
def test_mirror_matches_oracle_on_grid(kind):
    for ncls, rows, k in orc.grid_cases():
        x = orc.peaked_logits(rows, ncls, seed=ncls + k)
        sc, tv, ti = _mirror(x, rows, kind, k)
        want, _, _ = orc.video_scores(x, orc.offsets_of(rows), kind, k)
        assert sc.dtype == torch.float32 and ti.dtype == torch.int32
        assert tuple(sc.shape) == (len(rows), ncls) and tuple(ti.shape) == (len(rows), k)
        err = np.abs(sc.numpy().astype(np.float64) - want).max()
        assert err <= MIRROR_RTOL * max(1.0, np.abs(want).max()), (ncls, rows, k, err)
        # ranks are judged on the mirror's own fp32 scores: no near-tie against fp64
        for v, n in enumerate(rows):
            if n == 0:
                assert ti[v].tolist() == [-1] * k and tv[v].tolist() == [0.0] * k
                assert not sc[v].any()
            else:
                assert ti[v].tolist() == orc.top_order(sc[v].numpy(), k).tolist()
                assert torch.equal(tv[v], sc[v][ti[v].long()])


def test_mirror_ties_go_to_the_lower_index_and_integers_are_exact():
    rng = np.random.RandomState(0)
    x = rng.randint(-8, 9, size=(9, 12)).astype(np.float32)
    x[:, 7] = x[:, 2]
    x[:, 11] = x[:, 2]
    rows = (4, 0, 5)
    sc, tv, ti = _mirror(x, rows, "logit_sum", 12)
    want, wv, wi = orc.video_scores(x, orc.offsets_of(rows), "logit_sum", 12)
    assert np.array_equal(sc.numpy().astype(np.float64), want)
    assert np.array_equal(ti.numpy(), wi) and np.array_equal(tv.numpy().astype(np.float64), wv)
    for v in (0, 2):
        order = ti[v].tolist()
        assert order.index(2) < order.index(7) < order.index(11)


def test_ranking_differs_by_kind():
    """One confident clip against four lukewarm ones: the logit sum follows the
    confident clip, the mean of softmax scores follows the majority."""
    x = np.array([[8, 0, 0]] + [[0, 1, 0]] * 4, dtype=np.float32)
    off = torch.tensor([0, 5])
    _, _, by_sum = vops.video_scores(torch.from_numpy(x), off, scores="logit_sum", top_k=3)
    sc, tv, by_soft = vops.video_scores(torch.from_numpy(x), off, scores="softmax_mean", top_k=3)
    assert by_sum[0].tolist() == [0, 1, 2]
    assert by_soft[0].tolist() == [1, 0, 2]
    assert orc.video_scores(x, [0, 5], "logit_sum", 3)[2][0].tolist() == [0, 1, 2]
    assert orc.video_scores(x, [0, 5], "softmax_mean", 3)[2][0].tolist() == [1, 0, 2]
    assert abs(float(sc.sum()) - 1.0) < 1e-6
    # the aggregator follows its ``scores`` kind
    assert R2P1DAggregator(CPU)((torch.from_numpy(x),), None, TimeCard(1))[1] == 0
    agg = R2P1DAggregator(CPU, scores="softmax_mean", top_k=3)
    classes, scores = agg((torch.from_numpy(x),), None, TimeCard(1))[1]
    assert classes == (1, 0, 2) and scores == tuple(tv[0].tolist())


def test_argument_errors_name_the_argument():
    x, off = torch.zeros(2, 8), torch.tensor([0, 2])
    with pytest.raises(ValueError, match="k = 17"):
        vops.video_scores(torch.zeros(2, 32), off, top_k=17)
    with pytest.raises(ValueError, match="k = 9"):
        vops.video_scores(x, off, top_k=9)
    with pytest.raises(ValueError, match="k = 0"):
        vops.video_scores(x, off, top_k=0)
    with pytest.raises(ValueError, match="ncls = 4097"):
        vops.video_scores(torch.zeros(2, 4097), off, top_k=1)
    with pytest.raises(ValueError, match="scores"):
        vops.video_scores(x, off, scores="mean")
    with pytest.raises(ValueError, match="scores"):
        R2P1DAggregator(CPU, scores="softmax")
    with pytest.raises(ValueError, match="k = 17"):
        R2P1DAggregator(CPU, top_k=17)


# ------------------------------------------------------------------ aggregator
def test_aggregator_defaults_are_unchanged():
    """The returns of the default aggregator on the inputs of tests/test_stages.py
    (ints, -1 for an empty video of a batch, 0 for an empty single card), with
    and without the new keywords spelled out."""
    for kw in ({}, {"scores": "logit_sum", "top_k": 1, "results_path": None}):
        agg = R2P1DAggregator(CPU, aggregate=3, **kw)
        tc = TimeCard(9)
        tc.record("enqueue_filename")
        kids = [tc.fork(i) for i in range(3)]
        logits = torch.zeros(6, 400)
        logits[4, 123] = 10.0
        res = []
        for i, kid in enumerate(kids):
            kid.record("inference1_finish")
            res.append(agg((logits[2 * i:2 * i + 2],), None, kid))
        assert res[0] == (None, None, None) and res[1] == (None, None, None)
        assert res[2][1] == 123 and type(res[2][1]) is int and res[2][2].id == 9
        agg = R2P1DAggregator(CPU, aggregate=1, **kw)
        _, pred, card = agg((torch.zeros(0, 400),), None, TimeCard(1))
        assert pred == 0 and type(pred) is int and card.id == 1
        agg = R2P1DAggregator(CPU, **kw)
        a, b, c = TimeCard(1), TimeCard(2), TimeCard(3)
        a.num_clips, b.num_clips, c.num_clips = 1, 2, 0
        logits = torch.zeros(3, 400)
        logits[0, 5] = logits[1, 7] = logits[2, 7] = 1
        _, preds, cards = agg((logits,), None, TimeCardList([a, b, c]))
        assert preds == [5, 7, -1] and [t.id for t in cards.time_cards] == [1, 2, 3]
        assert agg.runtime_stats() == {}


def aggregator_cases(seed=3, ncls=400):
    """Three videos (the middle one empty) of peaked logits and their one-shot
    fp64 top-5: what every arrival form below must reproduce."""
    rows = (6, 0, 9)
    x = orc.peaked_logits(rows, ncls, seed)
    return rows, x, orc.offsets_of(rows)


def run_arrival_forms(device, kind="softmax_mean", k=5, results_path=None):
    """The aggregator's three arrival forms on ``device`` -> {form: [(classes,
    scores) per video]}: single cards, one TimeCardList batch with an empty
    video in it, and aggregate=3 with the segments of the videos interleaved
    over different calls and out of order."""
    rows, x, off = aggregator_cases()
    t = torch.from_numpy(x).to(device)
    out = {}
    agg = R2P1DAggregator(device, scores=kind, top_k=k, results_path=results_path)
    out["single"] = [agg((t[off[v]:off[v + 1]],), None, TimeCard(v))[1] for v in range(3)]
    cards = [TimeCard(v) for v in range(3)]
    for tc, n in zip(cards, rows):
        tc.num_clips = n
    _, res, done = agg((t,), None, TimeCardList(cards))
    assert [c.id for c in done.time_cards] == [0, 1, 2]
    out["batch"] = res
    # aggregate=3: video v's rows split 3 ways; the nine segments arrive as a
    # single card, a batch of five (with "rows" set, as a gathering runner
    # does) and a batch of three, sub_ids out of order
    agg3 = R2P1DAggregator(device, aggregate=3, scores=kind, top_k=k)
    segs = {}
    for v in range(3):
        parent = TimeCard(v)
        parent.record("enqueue_filename")
        cuts = [off[v] + (rows[v] * s) // 3 for s in range(4)]
        for s in range(3):
            kid = parent.fork(s)
            kid.record("inference1_finish")
            kid.extra["rows"] = cuts[s + 1] - cuts[s]
            segs[(v, s)] = (kid, t[cuts[s]:cuts[s + 1]])
    got = {}

    def send(keys):
        if len(keys) == 1:
            kid, part = segs[keys[0]]
            _, res, done = agg3((part,), None, kid)
            res, done = ([], []) if done is None else ([res], [done])
        else:
            block = torch.cat([segs[key][1] for key in keys])
            _, res, done = agg3((block,), None, TimeCardList([segs[key][0] for key in keys]))
            res, done = ([], []) if done is None else (res, done.time_cards)
        for r, tc in zip(res, done):
            got[tc.id] = r
    send([(2, 2)])
    assert not got
    send([(0, 1), (2, 0), (1, 2), (0, 0), (1, 0)])
    assert not got
    send([(1, 1), (0, 2), (2, 1)])
    assert sorted(got) == [0, 1, 2] and not agg3.results
    out["segments"] = [got[v] for v in range(3)]
    return out


def check_forms(forms, k, tol, classes_from=None):
    """Every form equals the one-shot fp64 result of the same rows: the classes
    (their fp64 gaps exceed ``tol``, asserted) and the scores within ``tol``."""
    rows, x, off = aggregator_cases()
    _, wv, wi = orc.video_scores(x, off, "softmax_mean", k)
    assert orc.top_gap(orc.video_scores(x, off, "softmax_mean", k)[0][[0, 2]], k) > 2 * tol
    for name, res in forms.items():
        assert len(res) == 3, name
        for v in range(3):
            classes, scores = res[v]
            assert isinstance(classes, tuple) and isinstance(scores, tuple)
            assert len(classes) == k and len(scores) == k
            assert all(type(c) is int for c in classes) and all(type(s) is float for s in scores)
            assert list(classes) == wi[v].tolist(), (name, v)
            assert np.abs(np.array(scores) - wv[v]).max() <= tol, (name, v)


def test_aggregator_modes_equal_the_one_shot_result():
    # softmax_mean scores are <= 1: the mirror's bound at that scale
    check_forms(run_arrival_forms(CPU), 5, MIRROR_RTOL)
    # an empty video: no class, zero scores
    assert run_arrival_forms(CPU)["batch"][1] == ((-1,) * 5, (0.0,) * 5)


def _scripted():
    """Logits of one row whose descending class order is 3, 9, 1, 7, 5, ..."""
    x = torch.zeros(1, 12)
    for rank, c in enumerate((3, 9, 1, 7, 5)):
        x[0, c] = 10.0 - rank
    return x


def test_accuracy_counters():
    agg = R2P1DAggregator(CPU, scores="softmax_mean", top_k=5)
    dflt = R2P1DAggregator(CPU)
    x = _scripted()
    for i, label in enumerate([3, 7, 11, None]):   # rank 1, rank 4, miss, unlabelled
        for a in (agg, dflt):
            tc = TimeCard(i)
            if label is not None:
                tc.extra["label"] = label
            a((x,), None, tc)
    assert agg.runtime_stats() == {"eval_videos": 3, "eval_top1": 1, "eval_top5": 2}
    # the default mode counts too: top-1 only
    assert dflt.runtime_stats() == {"eval_videos": 3, "eval_top1": 1}
    # the label of a re-joined video is read from its first segment's card
    agg3 = R2P1DAggregator(CPU, aggregate=2, scores="logit_mean", top_k=2)
    parent = TimeCard(5)
    parent.extra["label"] = 9
    parent.record("enqueue_filename")
    for s in (1, 0):
        kid = parent.fork(s)
        kid.record("inference1_finish")
        res = agg3((x,), None, kid)
    assert res[1][0] == (3, 9)
    assert agg3.runtime_stats() == {"eval_videos": 1, "eval_top1": 0, "eval_top2": 1}


def test_results_jsonl(tmp_path):
    base = str(tmp_path / "res")
    forms = run_arrival_forms(CPU, results_path=base)
    path = "%s.%d.jsonl" % (base, os.getpid())
    lines = [json.loads(line) for line in open(path)]
    want = forms["single"] + forms["batch"]
    assert [ln["id"] for ln in lines] == [0, 1, 2, 0, 1, 2]
    for ln, (classes, scores) in zip(lines, want):
        assert ln["label"] is None
        assert tuple(ln["classes"]) == classes and tuple(ln["scores"]) == scores
    # default mode: the argmax and its summed logit, with the label
    agg = R2P1DAggregator(CPU, results_path=str(tmp_path / "dflt"))
    tc = TimeCard(4)
    tc.extra["label"] = 1
    x = torch.tensor([[0.0, 2.0, 1.0], [0.0, 2.5, 1.0]])
    assert agg((x,), None, tc)[1] == 1
    (ln,) = [json.loads(line) for line in open("%s.%d.jsonl" % (tmp_path / "dflt", os.getpid()))]
    assert ln == {"id": 4, "label": 1, "classes": [1], "scores": [4.5]}


# ---------------------------------------------------------------------- labels
def _tree(tmp_path):
    root = tmp_path / "videos"
    for name in ("walking", "archery", "zumba"):
        (root / name).mkdir(parents=True)
        (root / name / "a.y4m").write_bytes(b"")
    (root / "README").write_text("not a class")
    return root


def test_directory_labels(tmp_path):
    root = _tree(tmp_path)
    lab = DirectoryLabels()
    assert [lab.label(str(root / n / "a.y4m")) for n in ("archery", "walking", "zumba")] \
        == [0, 1, 2]
    assert lab.label("synthetic://5?frames=300") is None
    (root / "aaa").mkdir()                          # listed once per root
    assert lab.label(str(root / "zumba" / "a.y4m")) == 2
    names = tmp_path / "classes.txt"
    names.write_text("abseiling\nzumba\nwalking\narchery\n")
    lab = DirectoryLabels(str(names))
    assert [lab.label(str(root / n / "a.y4m")) for n in ("archery", "walking", "zumba")] \
        == [3, 2, 1]
    names.write_text("abseiling\nzumba\n")
    lab = DirectoryLabels(str(names))
    with pytest.raises(ValueError) as err:
        lab.label(str(root / "archery" / "a.y4m"))
    assert "class_names" in str(err.value) and str(root / "archery" / "a.y4m") in str(err.value)
    assert "archery" in str(err.value) and str(names) in str(err.value)


def test_loader_sets_the_label_and_fork_keeps_it(tmp_path):
    from rnb_amd.utils import y4m
    root = tmp_path / "tree"
    rng = np.random.RandomState(0)
    frames = [(rng.randint(0, 256, (112, 128), dtype=np.uint8),
               rng.randint(0, 256, (56, 64), dtype=np.uint8),
               rng.randint(0, 256, (56, 64), dtype=np.uint8)) for _ in range(20)]
    paths = []
    for name in ("label0", "label1"):
        (root / name).mkdir(parents=True)
        paths.append(str(root / name / "video.y4m"))
        y4m.write_y4m(paths[-1], frames)
    loader = R2P1DLoader(CPU, num_clips_population=[2], num_clips_weights=[1], seed=0,
                         warmup=0, decoder="y4m", labels="dir")
    for want, path in enumerate(paths):
        (frames,), _, tc = loader(None, path, TimeCard(want))
        assert frames.shape[0] == 2 and tc.extra["label"] == want
        assert tc.fork(1).extra["label"] == want
        into = TimeCard(10 + want)
        out = (torch.empty(R2P1DLoader.output_shape_for(max_clips=15)[0]),)
        loader.call_into(None, path, into, out)
        assert into.extra["label"] == want
        seg = TimeCard(20 + want)
        rows, _, _ = loader.call_into_segments(None, path, seg, [out, (torch.empty_like(out[0]),)])
        assert sum(rows) == 2 and seg.extra["label"] == want
    # no labels asked for, or a synthetic path: no label
    plain = R2P1DLoader(CPU, num_clips_population=[2], num_clips_weights=[1], seed=0,
                        warmup=0, decoder="y4m")
    assert "label" not in plain(None, paths[1], TimeCard(1))[2].extra
    synth = R2P1DLoader(CPU, num_clips_population=[2], num_clips_weights=[1], seed=0,
                        warmup=0, labels="dir")
    assert "label" not in synth(None, "synthetic://5?frames=300", TimeCard(1))[2].extra
    with pytest.raises(ValueError, match="labels"):
        R2P1DLoader(CPU, warmup=0, labels="file")
    with pytest.raises(ValueError, match="class_names"):
        R2P1DLoader(CPU, warmup=0, class_names="x.txt")


# --------------------------------------------------------------------- configs
@pytest.mark.parametrize("decoder", ["y4m", "mjpeg"])
def test_eval_configs_load(decoder):
    spec = load_pipeline(os.path.join(ROOT, "configs", "r2p1d-whole-%s-3crop-eval.json" % decoder))
    base = load_pipeline(os.path.join(ROOT, "configs", "r2p1d-whole-%s-3crop.json" % decoder))
    assert len(spec.steps) == 3 and len(base.steps) == 2
    loader, runner, agg = (s.groups[0].kwargs for s in spec.steps)
    assert loader["decoder"] == decoder and loader["labels"] == "dir"
    assert loader["num_clips_population"] == [10] and loader["num_clips_weights"] == [1]
    assert loader["max_clips"] == 30 and runner["max_clips"] == 30
    assert agg["scores"] == "softmax_mean" and agg["top_k"] == 5 and agg["aggregate"] == 1
    assert spec.steps[2].groups[0].gpus == spec.steps[1].groups[0].gpus
    for key in ("crop", "filter", "depth"):
        assert loader[key] == base.steps[0].groups[0].kwargs[key]
