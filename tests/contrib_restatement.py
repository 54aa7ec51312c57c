"""rl_model_cover / rl_model_predict_contribs restated in plain Python from the definitions of include/rlhip.h -- TEST
INFRASTRUCTURE ONLY.  Every chain is scalar f64 arithmetic in the stated order (Python floats and numpy.float64 scalars: one rounding per
operation, nothing fused); nothing is summed by a library routine.  Trees are the dicts of tests/tree_models.py.

    covers(trees, rows)                 per tree, uint64 [nodes]: the rows whose walk visits the node (covers_np: the same, vectorised)
    node_values(trees, covers)          per tree, float64 [nodes], children first
    contribs(trees, weights, values, rows, columns)      float64 [rows][C + 2]: the requested columns, rest, bias
    leaf_sums(trees, weights, rows)     float64 [rows]: the f64 sum of weight * leaf output, and what local accuracy is measured with
"""
import numpy as np

import tree_models as TM


def walk(tree, row):
    """the nodes of the row's path, the root first, the leaf last.  Split.eval: a column at or beyond the row's width reads 0;
    `value <= threshold` goes left, so a NaN goes right."""
    feat, thr, left, right = tree["feature"], tree["threshold"], tree["left"], tree["right"]
    j, path = 0, [0]
    while feat[j] != -1:
        f = int(feat[j])
        v = row[f] if f < len(row) else np.float32(0)
        j = int(left[j]) if v <= thr[j] else int(right[j])
        path.append(j)
    return path


def paths(trees, rows):
    rows = np.asarray(rows, np.float32)
    return [[walk(t, r) for t in trees] for r in rows]


def covers(trees, rows, paths_=None):
    out = [np.zeros(len(t["feature"]), np.uint64) for t in trees]
    for per_tree in (paths(trees, rows) if paths_ is None else paths_):
        for c, p in zip(out, per_tree):
            for j in p:
                c[j] += np.uint64(1)
    return out


def covers_np(trees, rows):
    """covers() for large backgrounds: the same walk, all rows at a time; every node a walk visits is counted where it is visited"""
    rows = np.asarray(rows, np.float32)
    n, width = rows.shape
    ar = np.arange(n)
    out = []
    with np.errstate(invalid="ignore"):
        for t in trees:
            c = np.zeros(len(t["feature"]), np.uint64)
            nd = np.zeros(n, np.int64)
            c[0] += np.uint64(n)
            while True:
                f = t["feature"][nd]
                act = f != -1
                if not act.any():
                    break
                v = np.where(f < width, rows[ar, np.clip(f, 0, width - 1)], np.float32(0))
                nd = np.where(act, np.where(v <= t["threshold"][nd], t["left"][nd], t["right"][nd]), nd)
                c += np.bincount(nd[act], minlength=len(c)).astype(np.uint64)
            out.append(c)
    return out


def node_values(trees, covers_):
    out = []
    for t, c in zip(trees, covers_):
        val = [0.0] * len(t["feature"])
        for j in range(len(val) - 1, -1, -1):              # pre-order: the children come after their parent
            if t["feature"][j] == -1:
                val[j] = float(np.float64(t["output"][j]))
                continue
            l, r = int(t["left"][j]), int(t["right"][j])
            a, b = int(c[l]), int(c[r])
            if a + b == 0:
                a = b = 1
            with np.errstate(all="ignore"):
                val[j] = float((np.float64(a) * np.float64(val[l]) + np.float64(b) * np.float64(val[r])) / np.float64(a + b))
        out.append(np.array(val, np.float64))
    return out


def contribs(trees, weights, values, rows, columns, paths_=None, terms=None):
    """terms: a list that receives, per row, every d and every bias term (for the local-accuracy bound)"""
    rows = np.asarray(rows, np.float32)
    columns = [int(c) for c in columns]
    C = len(columns)
    slot_of = {f: s for s, f in enumerate(columns)}
    out = np.zeros((len(rows), C + 2), np.float64)
    all_paths = paths(trees, rows) if paths_ is None else paths_
    with np.errstate(all="ignore"):
        for i, per_tree in enumerate(all_paths):
            acc = [np.float64(0.0)] * (C + 2)
            mine = []
            for t, w, val, p in zip(trees, weights, values, per_tree):
                W = np.float64(np.float32(w))
                b = W * val[0]
                acc[C + 1] = acc[C + 1] + b
                mine.append(float(b))
                for j, n in zip(p[:-1], p[1:]):
                    d = W * (val[n] - val[j])
                    s = slot_of.get(int(t["feature"][j]), C)
                    acc[s] = acc[s] + d
                    mine.append(float(d))
            out[i] = acc
            if terms is not None:
                terms.append(mine)
    return out


def leaf_sums(trees, weights, rows, paths_=None, terms=None):
    rows = np.asarray(rows, np.float32)
    out = np.zeros(len(rows), np.float64)
    with np.errstate(all="ignore"):
        for i, per_tree in enumerate(paths(trees, rows) if paths_ is None else paths_):
            s, mine = np.float64(0.0), []
            for t, w, p in zip(trees, weights, per_tree):
                x = np.float64(np.float32(w)) * np.float64(t["output"][p[-1]])
                s = s + x
                mine.append(float(x))
            out[i] = s
            if terms is not None:
                terms.append(mine)
    return out


def model_features(trees):
    """rl_model_features' order: the feature ids the model splits on, ascending"""
    return sorted({int(f) for t in trees for f in t["feature"] if f != -1})


def same_f64(got, want):
    """None, or what differs.  Outside NaN results bit for bit; where the reference is NaN the other is NaN (as TM.same_scores)"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if got.shape != want.shape:
        return "shape %r != %r" % (got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.argwhere(np.where(nan, ~np.isnan(got), got.view(np.uint64) != want.view(np.uint64)))
    if bad.size == 0:
        return None
    i = tuple(bad[0])
    return "%d of %d values differ, first at %r: %r (%#018x) != %r (%#018x)" % (len(bad), want.size, i, got[i], got.view(np.uint64)[i], want[i],
                                                                               want.view(np.uint64)[i])


# ---- k_model_contribs' LDS plan (rl_contrib_host.h) -----------------------------------------------------------------------------------
LDS_BUDGET, TREE_TILE, NODE_BYTES = 160 * 1024, 8, 32


def tree_tile(maxn):
    """contrib_tree_tile: at most TREE_TILE trees, fewer while the tile would pass a fifth of the budget"""
    return max(1, min(TREE_TILE, (LDS_BUDGET // 5) // (NODE_BYTES * maxn)))


def slot_limit(maxn, docs=64):
    """contrib_slot_limit: the f64 accumulators [slots][docs + 1] a block holds beside its tree tile"""
    return max(0, LDS_BUDGET - tree_tile(maxn) * maxn * NODE_BYTES) // ((docs + 1) * 8)


# ---- the models the tests share -------------------------------------------------------------------------------------------------------
def hand_stump():
    """one stump on feature 1, threshold 0.0, outputs (-1, 3), weight 0.5; a background of three rows going left and one going right"""
    trees = [TM.flatten(TM.S(1, 0.0, TM.L(-1.0), TM.L(3.0)))]
    bg = np.array([[0, -1.0], [0, 0.0], [0, -2.0], [0, 0.5]], np.float32)
    return trees, np.array([0.5], np.float32), bg


def chain_model(side, depth=30, seed=5):
    rng = np.random.default_rng(seed)
    g = TM.Gen(rng)
    return [TM.chain(g, depth, side)], np.array([0.7], np.float32)


def grid_rows(rng, n, width=13, special=0.06):
    """rows from TM.GRID, so they hit thresholds exactly, with NaN and +-Infinity cells among them; column 0 is 0"""
    rows = TM.GRID[rng.integers(0, len(TM.GRID), (n, width))]
    sp = rng.random((n, width)) < special
    rows[sp] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, int(sp.sum()))]
    rows[:, 0] = 0.0
    return np.ascontiguousarray(rows, np.float32)
