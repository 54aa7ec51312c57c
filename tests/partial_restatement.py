"""rl_model_predict_partial restated with what the tests already have -- TEST INFRASTRUCTURE ONLY.

Cell j of a call, grid_off[c] <= j < grid_off[c + 1], is column columns[c] set to grid[j] in every document.  Two restatements of its
scores:

  materialised   the substituted matrix is built -- widened with zeros where the column lies at or beyond the rows' width -- and
                 tree_models.eval_ensemble_np scores it.  This is the definition.
  path rule      what the kernel is allowed to skip: a document walks a tree on its own row until a node on that path
                 tests the cell's column; from that node on the walk goes on with the grid value standing in at EVERY node that tests
                 the column.  A tree that never tests the column returns the base leaf.

and the two sums of a cell in their fixed order as a plain Python loop: partial p the serial chain over the documents
[256 p, 256 p + 256), the total the serial chain over the partials, both from +0.0.  plan() restates rl_partial_host.h's bookkeeping:
chunks of cells, batches that never straddle a column, uses per column.  tests/test_partial_cpu.py holds all of them against each
other and against tables derived by hand; the GPU tests compare the kernels with them."""
import functools

import numpy as np

import permuted_restatement as PR
import tree_models as TM

SUM_BLOCK = 256
bits32, bits64 = PR.bits32, PR.bits64


def materialise(rows, column, value):
    rows = np.asarray(rows, np.float32)
    out = np.zeros((rows.shape[0], max(rows.shape[1], column + 1)), np.float32)
    out[:, :rows.shape[1]] = rows
    out[:, column] = np.float32(value)
    return out


def partial_scores(trees, weights, rows, columns, grids):
    """(f32 base [n], f32 [cells][n]) by the materialised definition"""
    rows = np.asarray(rows, np.float32)
    base = TM.eval_ensemble_np(trees, weights, rows)
    out = [TM.eval_ensemble_np(trees, weights, materialise(rows, int(c), v)) for c, g in zip(columns, grids) for v in np.asarray(g, np.float32)]
    return base, np.stack(out)


def partial_scores_path_rule(trees, weights, rows, columns, grids):
    """the same by the path rule"""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    base = TM.eval_ensemble_np(trees, weights, rows)
    zero = np.zeros(n, np.int64)
    out = []
    with np.errstate(all="ignore"):
        for c, g in zip(columns, grids):
            c = int(c)
            for v in np.asarray(g, np.float32):
                dv = np.full(n, v, np.float32)
                s = np.zeros(n, np.float32)
                for t, w in zip(trees, weights):
                    if not (t["feature"] == c).any():               # the tree never tests the column: the base leaf
                        leaf, _ = PR._walk_from(t, zero, rows, -2, dv, False)
                    else:
                        at, hit = PR._walk_from(t, zero, rows, c, dv, True)           # the base walk, up to the first node that tests c
                        sub, _ = PR._walk_from(t, at, rows, c, dv, False)             # from there on: the grid value at every node that tests c
                        own, _ = PR._walk_from(t, at, rows, -2, dv, False)            # the base walk's own end
                        leaf = np.where(hit, sub, own)
                    s = (s.astype(np.float64) + t["output"][leaf].astype(np.float64) * np.float64(np.float32(w))).astype(np.float32)
                out.append(s)
    return base, np.stack(out)


def fixed_sums(ice, base, block=SUM_BLOCK):
    """(S1, S2) of one cell, the definition's order as a plain loop.  `block` is there for the order probe only."""
    x = np.asarray(ice, np.float32).astype(np.float64)          # (numpy scalars below: inf - inf is NaN, not an exception)
    b = np.asarray(base, np.float32).astype(np.float64)
    s1 = s2 = np.float64(0.0)
    with np.errstate(all="ignore"):
        for p0 in range(0, len(x), block):
            p1 = p2 = np.float64(0.0)
            for i in range(p0, min(len(x), p0 + block)):
                d = x[i] - b[i]
                p1 = p1 + x[i]
                p2 = p2 + d * d
            s1 = s1 + p1
            s2 = s2 + p2
    return float(s1), float(s2)


def reduce_cells(base, sc):
    """(f64 mean [cells], f64 shift2 [cells]) of scores [cells][n]"""
    n = np.float64(len(base))
    sums = [fixed_sums(s, base) for s in sc]
    with np.errstate(all="ignore"):
        return np.array([np.float64(a) / n for a, _ in sums], np.float64), np.array([np.float64(b) / n for _, b in sums], np.float64)


def thresholds_grid(trees, column):
    """the model's distinct thresholds of the column, ascending, -0.0 folded into 0.0, plus nextafter(last, +inf) where that is finite and
    greater; None where no tree tests the column"""
    v = np.array([th for t in trees for f, th in zip(t["feature"], t["threshold"]) if f == column], np.float32)
    v = np.unique(v[~np.isnan(v)] + np.float32(0))
    if not v.size:
        return None
    with np.errstate(over="ignore"):
        nxt = np.nextafter(v[-1], np.float32(np.inf), dtype=np.float32)
    return np.concatenate([v, [nxt]]).astype(np.float32) if np.isfinite(nxt) and nxt > v[-1] else v


def plan(trees, columns, grids, chunk, B):
    """rl_partial_host.h's partial_plan: a list of chunks, each a list of batches (column, place in columns, first cell in the chunk,
    cells, the B values with the last repeated, uses as a string of 0 / 1 per tree); the base is the first batch of the first chunk"""
    off = np.concatenate([[0], np.cumsum([len(g) for g in grids])])
    flat = np.concatenate([np.asarray(g, np.float32) for g in grids])
    col_of = np.repeat(np.arange(len(columns)), [len(g) for g in grids])
    uses = lambda c: "".join("1" if (t["feature"] == c).any() else "0" for t in trees)      # noqa: E731
    chunks, j, total = [], 0, int(off[-1])
    while j < total:                                            # a chunk ends where the next batch would not fit whole, unless no chunk could hold it
        bs, used = ([(-1, -1, 0, 1, [np.float32(0)] * B, "0" * len(trees))] if j == 0 else []), 0
        while j < total:
            c = int(col_of[j])
            want, left = min(B, int(off[c + 1]) - j), chunk - used
            if left == 0 or (want > left and used > 0 and want <= chunk):
                break
            cnt = min(want, left)
            vals = [flat[j + min(u, cnt - 1)] for u in range(B)]
            bs.append((int(columns[c]), c, used, cnt, vals, uses(int(columns[c]))))
            j, used = j + cnt, used + cnt
        chunks.append(bs)
    return chunks


# ---- the main data of the tests: permuted_restatement's model and rows under the thresholds grids -----------------------------------------
TWO = np.array([-0.5, 0.5], np.float32)                         # the grid of a column without thresholds (0: untested; 13: at the row stride)


@functools.lru_cache(maxsize=None)
def main_grids():
    trees = PR.main_data()[0]
    out = []
    for c in PR.COLUMNS:
        g = thresholds_grid(trees, c)
        out.append(TWO if g is None else g)
    for g in out:
        g.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def main_partial():
    """(base, scores [cells][n], mean, shift2) of the main data by the materialised restatement, made once"""
    trees, w, rows = PR.main_data()[:3]
    base, sc = partial_scores(trees, w, rows, PR.COLUMNS, main_grids())
    mean, shift2 = reduce_cells(base, sc)
    for a in (base, sc, mean, shift2):
        a.setflags(write=False)
    return base, sc, mean, shift2
