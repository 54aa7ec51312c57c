"""rl_model_predict_partial2 restated with what the tests already have -- TEST INFRASTRUCTURE ONLY.

Cell (p, u, v) of a call is column a = pairs[p][0] set to grids[p][0][u] AND column b = pairs[p][1] set to grids[p][1][v] in every
document; a pair's cells are row-major.  Two restatements of its scores:

  materialised       the substituted matrix is built -- widened with zeros where a column lies at or beyond the rows' width -- and
                     tree_models.eval_ensemble_np scores it.  This is the definition.
  rectangle descent  what the kernel does, as a plain Python loop per document, tree and tile: the document descends
                     the tree once with the index rectangle of the tile's cells that reach the node; a node on a splits the a range at the
                     number of the tile's values of a that are <= the threshold, a node on b the b range, any other node takes the row's
                     own value; where both sides hold cells the right one waits on a stack, whose greatest depth is returned.

plan() restates rl_partial2_host.h's bookkeeping.  The sums are partial_restatement's.  tests/test_partial2_cpu.py holds all of them
against each other and against a table written out by hand; the GPU tests compare the kernel with them."""
import functools

import numpy as np

import partial_restatement as PD
import permuted_restatement as PR
import tree_models as TM

bits32, bits64 = PD.bits32, PD.bits64


def materialise2(rows, a, va, b, vb):
    return PD.materialise(PD.materialise(rows, a, va), b, vb)


def partial2_scores(trees, weights, rows, pairs, grids):
    """(f32 base [n], f32 [cells][n]) by the materialised definition"""
    rows = np.asarray(rows, np.float32)
    base = TM.eval_ensemble_np(trees, weights, rows)
    out = [TM.eval_ensemble_np(trees, weights, materialise2(rows, int(a), va, int(b), vb))
           for (a, b), (ga, gb) in zip(pairs, grids) for va in np.asarray(ga, np.float32) for vb in np.asarray(gb, np.float32)]
    return base, np.stack(out)


def descend(t, row, a, ga, b, gb, give):
    """one document's rectangle descent of tree t over the tile ga x gb: give(u0, u1, v0, v1, leaf) per leaf reached; returns the greatest
    number of pending siblings"""
    feat, thr, left, right = t["feature"], t["threshold"], t["left"], t["right"]
    stack, deepest = [], 0
    nd, u0, u1, v0, v1 = 0, 0, len(ga), 0, len(gb)
    while True:
        f = int(feat[nd])
        if f == -1:
            give(u0, u1, v0, v1, nd)
            if not stack:
                return deepest
            nd, u0, u1, v0, v1 = stack.pop()
            continue
        th = thr[nd]
        if f == a or f == b:
            with np.errstate(invalid="ignore"):
                p = int((ga <= th).sum()) if f == a else int((gb <= th).sum())
            lo, hi = (u0, u1) if f == a else (v0, v1)
            m = min(max(p, lo), hi)
            if m == lo:
                nd = int(right[nd])
            elif m == hi:
                nd = int(left[nd])
            else:
                stack.append((int(right[nd]), m, u1, v0, v1) if f == a else (int(right[nd]), u0, u1, m, v1))
                deepest = max(deepest, len(stack))
                nd = int(left[nd])
                if f == a:
                    u1 = m
                else:
                    v1 = m
        else:
            v = row[f] if f < len(row) else np.float32(0)
            with np.errstate(invalid="ignore"):
                nd = int(left[nd]) if v <= th else int(right[nd])


def partial2_scores_descent(trees, weights, rows, pairs, grids, TA, TB):
    """(f32 [cells][n], the greatest number of pending siblings) by the rectangle descent over tiles of TA x TB cells"""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    out, deepest = [], 0
    for (a, b), (ga, gb) in zip(pairs, grids):
        ga, gb = np.asarray(ga, np.float32), np.asarray(gb, np.float32)
        sc = np.zeros((len(ga), len(gb), n), np.float32)
        for x0 in range(0, len(ga), TA):
            for y0 in range(0, len(gb), TB):
                ta, tb = ga[x0:x0 + TA], gb[y0:y0 + TB]
                for i in range(n):
                    s = np.zeros((len(ta), len(tb)), np.float32)
                    for t, w in zip(trees, weights):
                        cover = np.zeros(s.shape, np.int64)

                        def give(u0, u1, v0, v1, leaf):
                            ow = np.float64(t["output"][leaf]) * np.float64(np.float32(w))
                            with np.errstate(all="ignore"):
                                s[u0:u1, v0:v1] = (s[u0:u1, v0:v1].astype(np.float64) + ow).astype(np.float32)
                            cover[u0:u1, v0:v1] += 1
                        deepest = max(deepest, descend(t, rows[i], int(a), ta, int(b), tb, give))
                        assert (cover == 1).all()               # the rectangles that reach leaves partition the tile
                    sc[x0:x0 + TA, y0:y0 + TB, i] = s
        out.append(sc.reshape(-1, n))
    return np.concatenate(out), deepest


def uses(trees, a, b):
    return "".join("1" if ((t["feature"] == a) | (t["feature"] == b)).any() else "0" for t in trees)


def plan(trees, pairs, grids, chunk, TA, TB):
    """rl_partial2_host.h's partial2_plan: (the base tile, a list of chunks, each a list of tiles); a tile is (a, b, pair, first slot in the
    chunk, values of a, values of b, first cell of the call, gb, the TA + TB values with the last of either axis repeated, uses)"""
    base = (-1, -1, -1, 0, 1, 1, -1, 1, [np.float32(0)] * (TA + TB), "0" * len(trees))
    sb = min(TB, chunk)
    sa = max(1, min(TA, chunk // sb))                        # cut only where a whole chunk is smaller than a tile
    chunks, used, cell0 = [], chunk, 0
    for q, ((a, b), (ga, gb)) in enumerate(zip(pairs, grids)):
        ga, gb = np.asarray(ga, np.float32), np.asarray(gb, np.float32)
        for u0 in range(0, len(ga), sa):
            for v0 in range(0, len(gb), sb):
                ca, cb = min(sa, len(ga) - u0), min(sb, len(gb) - v0)
                if used + ca * cb > chunk:
                    chunks.append([])
                    used = 0
                vals = [ga[u0 + min(u, ca - 1)] for u in range(TA)] + [gb[v0 + min(v, cb - 1)] for v in range(TB)]
                chunks[-1].append((int(a), int(b), q, used, ca, cb, cell0 + u0 * len(gb) + v0, len(gb), vals, uses(trees, int(a), int(b))))
                used += ca * cb
        cell0 += len(ga) * len(gb)
    return base, chunks


# ---- the main data of the tests: permuted_restatement's model and rows, pairs that trees test together on a path ---------------------------
def together(trees):
    """{(a, b), a < b: the trees with a node on a above or below a node on b}"""
    out = {}
    for k, t in enumerate(trees):
        def rec(nd, above):
            f = int(t["feature"][nd])
            if f == -1:
                return
            for g in above - {f}:
                out.setdefault((min(f, g), max(f, g)), set()).add(k)
            rec(int(t["left"][nd]), above | {f})
            rec(int(t["right"][nd]), above | {f})
        rec(0, set())
    return out


@functools.lru_cache(maxsize=None)
def main_pairs():
    """the three pairs of the main model that the most trees test together on a path, the second one turned round"""
    both = together(PR.main_data()[0])
    top = sorted(both, key=lambda pr: (-len(both[pr]), pr))[:3]
    return (top[0], top[1][::-1], top[2])


def pair_grids(pairs, na=None, nb=None):
    """the thresholds grids of the main data for both axes of every pair, cut to na and nb values spread over the grid"""
    pick = lambda g, k: g if k is None or k >= len(g) else g[np.unique(np.arange(k) * (len(g) - 1) // max(1, k - 1))]      # noqa: E731
    return [(pick(PD.main_grids()[a], na), pick(PD.main_grids()[b], nb)) for a, b in pairs]


@functools.lru_cache(maxsize=None)
def main_partial2():
    """(pairs, grids, base, scores [cells][n], mean, shift2) of the main data by the materialised restatement, made once: 9 x 10 cells a pair"""
    trees, w, rows = PR.main_data()[:3]
    pairs = main_pairs()
    grids = pair_grids(pairs, 9, 10)
    base, sc = partial2_scores(trees, w, rows, pairs, grids)
    mean, shift2 = PD.reduce_cells(base, sc)
    for a in (base, sc, mean, shift2):
        a.setflags(write=False)
    return pairs, grids, base, sc, mean, shift2
