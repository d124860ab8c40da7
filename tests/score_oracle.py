"""fp64 numpy oracle of ``rnb_amd.ops.video.video_scores``, written apart from
its torch mirror: a plain loop over the videos, numpy's own exp and sums, and
``np.lexsort`` for the tie rule (descending score, then ascending class)."""
import numpy as np

KINDS = ("logit_sum", "logit_mean", "softmax_sum", "softmax_mean")


def video_scores(logits, offsets, kind, k):
    """-> (scores [nvid][ncls] f64, top_val [nvid][k] f64, top_idx [nvid][k] int64)."""
    assert kind in KINDS
    x = np.asarray(logits, dtype=np.float64)
    off = [int(o) for o in offsets]
    nvid, ncls = len(off) - 1, x.shape[1]
    scores = np.zeros((nvid, ncls))
    top_val = np.zeros((nvid, k))
    top_idx = np.full((nvid, k), -1, dtype=np.int64)
    for v in range(nvid):
        rows = x[off[v]:off[v + 1]]
        if rows.shape[0] == 0:
            continue
        if kind.startswith("softmax"):
            e = np.exp(rows - rows.max(axis=1, keepdims=True))
            rows = e / e.sum(axis=1, keepdims=True)
        s = rows.sum(axis=0)
        if kind.endswith("mean"):
            s = s / rows.shape[0]
        scores[v] = s
        top_idx[v] = top_order(s, k)
        top_val[v] = s[top_idx[v]]
    return scores, top_val, top_idx


def top_order(s, k):
    """The k largest of ``s``, descending, ties to the lower index."""
    s = np.asarray(s)
    return np.lexsort((np.arange(s.shape[0]), -s))[:k]


def top_gap(scores64, k):
    """Smallest distance between consecutive fp64 scores among the k + 1 largest
    of any non-empty row: the top-k order is decided by more than this."""
    gap = np.inf
    for s in np.asarray(scores64):
        d = np.sort(s)[::-1][:k + 1]
        if d.size > 1:
            gap = min(gap, float(np.min(d[:-1] - d[1:])))
    return gap


# ---------------------------------------------------------------- shared cases
NCLS_GRID = (1, 5, 63, 64, 65, 255, 256, 257, 400, 1000, 4096)
ROWS_7 = (0, 45, 1, 0, 130, 65, 0)      # empty video first, in the middle and last
ROWS_7B = (0, 3, 4, 0, 5, 63, 0)        # with ROWS_7 and (64,): every row count of the grid
K_GRID = (1, 5, 16)


def offsets_of(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    return off


def grid_cases():
    """(ncls, rows per video, k) over the shape grid: 7 videos with empty ones
    first / middle / last and 1 video; the row counts {0, 1, 3, 4, 5, 45, 63,
    64, 65, 130} all occur; k capped at ncls."""
    cases = []
    for i, ncls in enumerate(NCLS_GRID):
        for k in sorted({min(k, ncls) for k in K_GRID}):
            cases.append((ncls, ROWS_7 if (i + k) % 2 else ROWS_7B, k))
        cases.append((ncls, (64,) if i % 2 else (130,), min(5, ncls)))
    return cases


def peaked_logits(rows, ncls, seed):
    """Logits ~ N(0, 3^2) plus, per video, one row with a 30-unit peak."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(sum(rows), ncls) * 3.0).astype(np.float32)
    off = offsets_of(rows)
    for v, n in enumerate(rows):
        if n:
            x[off[v] + rng.randint(n), rng.randint(ncls)] += np.float32(30.0)
    return x
