"""rl_model_predict_permuted / rl_model_eval_permuted restated with what the tests already have -- TEST INFRASTRUCTURE ONLY.

Cell (c, r) of a call is column columns[c] under repeat r: document i reads that column from row donor[r][i].  Two restatements:

  materialised   the permuted matrix is built, tree_models.eval_ensemble_np scores it, eval_lists_restatement.eval_lists ranks it.  This
                 is the definition.
  path rule      what the kernel is allowed to skip: a document walks a tree on its own row until a node on that path
                 tests the cell's column; from that node on the walk goes on with the donated value standing in at EVERY node that tests
                 the column.  A tree whose base path never tests the column returns the base leaf, and a column at or beyond the row
                 width reads 0 on both sides.

tests/test_permuted_cpu.py holds the two against each other and against a table derived by hand; the GPU tests compare the kernels
with them.  A (cell, list) whose scores hold a NaN returns the flag and 0.0, as stages_restatement has it for a (stage, list)."""
import functools

import numpy as np

import stages_restatement as SR
import tree_models as TM


def donors_2d(donor, n):
    d = np.asarray(donor, np.int64)
    d = d[None, :] if d.ndim == 1 else d
    assert d.shape[1] == n and (d >= 0).all() and (d < max(n, 1)).all()
    return d


def materialise(rows, column, donor_r):
    out = np.array(rows, np.float32, copy=True)
    if column < out.shape[1]:
        out[:, column] = rows[donor_r, column]
    return out


def permuted_scores(trees, weights, rows, columns, donor):
    """(f32 base [n], f32 [C][R][n]) by the materialised definition"""
    rows = np.asarray(rows, np.float32)
    d = donors_2d(donor, len(rows))
    base = TM.eval_ensemble_np(trees, weights, rows)
    out = np.stack([np.stack([TM.eval_ensemble_np(trees, weights, materialise(rows, int(c), d[r])) for r in range(len(d))]) for c in columns])
    return base, out


def _walk_from(t, nd, rows, column, dv, stop_at_column):
    """every document's walk of tree t from node nd[i] on its own row; with stop_at_column the walk stops AT the first node that tests
    `column` (returned with hit = True), otherwise `dv` stands in wherever the column is tested and the walk ends in a leaf"""
    n, width = rows.shape
    ar = np.arange(n)
    nd = nd.copy()
    hit = np.zeros(n, bool)
    while True:
        f = t["feature"][nd]
        if stop_at_column:
            hit |= (f == column)
        act = (f != -1) & ~hit
        if not act.any():
            return nd, hit
        own = np.where(f < width, rows[ar, np.clip(f, 0, width - 1)], np.float32(0))
        v = own if stop_at_column else np.where(f == column, dv, own)
        with np.errstate(invalid="ignore"):
            nxt = np.where(v <= t["threshold"][nd], t["left"][nd], t["right"][nd])
        nd = np.where(act, nxt, nd)


def permuted_scores_path_rule(trees, weights, rows, columns, donor):
    """the same by the path rule"""
    rows = np.asarray(rows, np.float32)
    n, width = rows.shape
    d = donors_2d(donor, n)
    base = TM.eval_ensemble_np(trees, weights, rows)
    out = np.zeros((len(columns), len(d), n), np.float32)
    zero = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for ci, c in enumerate(columns):
            c = int(c)
            for r in range(len(d)):
                if c >= width:                                  # reads 0 on both sides
                    out[ci, r] = base
                    continue
                dv = rows[d[r], c]
                s = np.zeros(n, np.float32)
                for t, w in zip(trees, weights):
                    if not (t["feature"] == c).any():           # the tree tests none of the cell's columns: the base leaf
                        leaf, _ = _walk_from(t, zero, rows, -2, dv, False)
                    else:
                        at, hit = _walk_from(t, zero, rows, c, dv, True)          # the base walk, up to the first node that tests c
                        sub, _ = _walk_from(t, at, rows, c, dv, False)            # from there on: substituted at every node that tests c
                        own, _ = _walk_from(t, at, rows, -2, dv, False)           # the base walk's own end
                        leaf = np.where(hit, sub, own)
                    s = (s.astype(np.float64) + t["output"][leaf].astype(np.float64) * np.float64(np.float32(w))).astype(np.float32)
                out[ci, r] = s
    return base, out


def eval_permuted(trees, weights, rows, labels, qoff, metric, k, columns, donor, err_max=16.0, qkey=None, ideal_dcg=None,
                  rel_doc_count=None, scores=None):
    """(f64 base [Q], uint8 base NaN flags [Q], f64 values [C][R][Q], uint8 flags [C][R][Q], f64 ideal [Q]) with the arguments of
    _native.Model.eval_permuted behind the model.  scores: permuted_scores(...) of an earlier call on the same model and file."""
    base, sc = permuted_scores(trees, weights, rows, columns, donor) if scores is None else scores
    C, R, n = sc.shape
    flat = np.concatenate([sc.reshape(C * R, n), base[None, :]])                 # the base: one more cell
    st = list(range(1, C * R + 2))
    v, nan, ideal = SR.eval_stages(None, None, None, labels, qoff, metric, k, st, err_max=err_max, qkey=qkey, ideal_dcg=ideal_dcg,
                                   rel_doc_count=rel_doc_count, scores=flat)
    nl = v.shape[1]
    return v[-1], nan[-1], v[:-1].reshape(C, R, nl), nan[:-1].reshape(C, R, nl), ideal


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the main data of the tests -------------------------------------------------------------------------------------------------------
LENS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600]       # both sides of kEvTiny and kEvWave
NT = 37
COLUMNS = list(range(14))                                       # 0: no tree tests it; 1 .. 12: used; 13: at the row stride


@functools.lru_cache(maxsize=None)
def main_data():
    """tests/test_gpu_stages.py's main data, built by the same steps from the same seed: 37 random trees of 2 - 8 leaves with weight 0.1
    over 13-column rows from the 65-value grid, labels 0 - 4, lists of LENS documents.  donor[r] = RandomState(1 + r).permutation(n),
    r < 3; the materialised restatement's scores of all 14 columns, made once."""
    rng = np.random.default_rng(5)
    g = TM.Gen(rng)
    trees = [TM.random_tree(g, int(rng.integers(2, 9))) for _ in range(NT)]
    w = np.full(NT, 0.1, np.float32)
    qoff = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    rows = rng.choice(TM.GRID, (int(qoff[-1]), 13)).astype(np.float32)
    rows[:, 0] = 0.0
    lab = rng.integers(0, 5, int(qoff[-1])).astype(np.float32)
    donor = np.stack([np.random.RandomState(1 + r).permutation(len(rows)) for r in range(3)]).astype(np.int32)
    base, sc = permuted_scores(trees, w, rows, COLUMNS, donor)
    for a in (w, qoff, rows, lab, donor, base, sc):
        a.setflags(write=False)
    return trees, w, rows, lab, qoff, donor, base, sc


# ---- trees built to catch a wrong path rule -------------------------------------------------------------------------------------------
def trap_trees():
    """on column 3 (and 5): a chain that tests one column at every level; a tree that tests the column at the root and again below both
    children; single leaves; a tree that uses the column next to one that does not; thresholds that donated values hit exactly"""
    L, S = TM.L, TM.S
    rng = np.random.default_rng(24)
    g3 = TM.Gen(rng, features=[3])
    trees = [TM.chain(g3, 6, "left"), TM.chain(g3, 5, "right"),
             TM.flatten(S(3, 0.0, S(3, -1.0, L(1.0), S(3, -0.5, L(2.0), L(3.0))), S(3, 1.0, S(5, 0.25, L(4.0), S(3, 0.5, L(5.0), L(6.0))), L(7.0)))),
             TM.single_leaf(TM.Gen(rng)), TM.single_leaf(TM.Gen(rng)),
             TM.flatten(S(3, 0.25, L(-1.0), L(1.5))), TM.flatten(S(7, 0.25, L(-2.0), L(0.5))),
             TM.flatten(S(5, -0.0, S(3, np.inf, L(0.125), L(9.0)), S(3, -np.inf, L(-9.0), L(0.75)))),
             TM.flatten(S(2, 0.0, S(3, 0.0, L(1.0), L(-1.0)), S(5, 0.0, L(2.0), S(3, -0.0, L(-3.0), L(3.0)))))]
    w = np.array([0.1, 1.0, 0.5, -0.25, 3.0, 0.7, 1e-3, -1.0, 0.1], np.float32)
    return trees, w


def trap_rows(rng, n):
    """grid rows whose columns 3 and 5 also hold the values the thresholds above are made of, NaN, +-Infinity and -0.0"""
    rows = rng.choice(TM.GRID, (n, 13)).astype(np.float32)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.25, 0.5, -0.5, 1.0, -1.0], np.float32)
    for c in (3, 5):
        at = rng.random(n) < 0.4
        rows[at, c] = sp[rng.integers(0, len(sp), int(at.sum()))]
    rows[:, 0] = 0.0
    return rows
