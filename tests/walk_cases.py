"""The adversarial models of the scoring tests, with rows fit for attribution, and their references -- TEST INFRASTRUCTURE ONLY.

tests/test_gpu_model_eval.py holds the scoring kernels against tests/tree_models.py's hand-built models at the edges of
`value <= threshold`.  The other eight walks of a model's trees (rl_model_cover, rl_model_predict_contribs, _leaf_sums, _shap,
_interactions, _stages, _partial, _permuted) each have a loop of their own; tests/test_gpu_model_walks.py holds them against their
restatements on the models named here, and tests/test_model_walks_cpu.py holds the restatements against something independent first.

The cases' OWN rows are not used: tree_models.probe_rows overwrites its first len(pool) + 12 rows with rows that hold one value in every
column, which with the cases' 200 rows is 200 of 200 on count_37 and 180 of 200 on feature_0 -- and attribution over rows whose features
are all equal exercises almost nothing.  Here a row set is that constant prefix, at least 128 rows of probe_rows' mixed part, the whole
shuffled with a fixed seed, so that constant and mixed rows both fall into every block of 64.  Everything is made once (lru_cache) and
handed out read-only.
"""
import functools

import numpy as np

import contrib_restatement as CR
import interact_restatement as IR
import partial_restatement as PD
import shap_restatement as SR
import tree_models as TM

L, S = TM.L, TM.S
WIDTHS = (20, 13, 12, 5, 2, 1)                   # the width family: one model scored at every one of them
MODELS = ("thresholds", "feature_0", "col0_garbage", "feat_254", "feat_255", "width", "big_ids", "dup_path", "thresholds_deep")
CASES = tuple(n for n in MODELS if n != "width") + tuple("width_%d" % w for w in WIDTHS)
EDGE_MODELS = ("thresholds", "thresholds_deep", "dup_path")       # the models every wrong rule below must show on
MIXED = 128                                      # mixed rows of a set at least
MIN_ROWS = 258                                   # a set holds at least this many: both sides of a block of 256, and a background of 257 is not all
ROW_COUNTS = (1, 63, 64, 65, None)               # rows per call: both sides of a block of 64; None: all
BG_COUNTS = (0, 257, None)                       # background rows: none, 257, all
BIG = 2147483647


def model_of(case):
    return "width" if case.startswith("width_") else case


# ---- the models -----------------------------------------------------------------------------------------------------------------------
def _big_ids():
    """stumps and depth-2 trees on the feature ids 1, 65535, 65536 and 2^31 - 1; rows are 3 columns wide, so the large ids read 0 and
    their thresholds lie on both sides of it: +-0.0, +-Float.MIN_VALUE"""
    rng = np.random.default_rng(71)
    o = lambda: np.float32(rng.standard_normal())                       # noqa: E731
    T = TM
    trees = [S(1, 0.25, L(o()), L(o())), S(65535, 0.0, L(o()), L(o())), S(65536, -T.F32_MIN, L(o()), L(o())), S(BIG, -0.0, L(o()), L(o())),
             S(BIG, T.F32_MIN, L(o()), L(o())), S(65535, -1.0, L(o()), L(o())),
             S(1, 0.0, S(65536, 0.0, L(o()), L(o())), S(BIG, -T.F32_MIN, L(o()), L(o()))),
             S(BIG, 0.5, S(65535, T.F32_MIN, L(o()), L(o())), S(1, -0.5, L(o()), L(o()))),
             S(65536, np.nan, L(o()), S(1, 1.0 / 3.0, L(o()), L(o()))),
             S(2, 0.1, S(BIG, 0.0, L(o()), S(65535, 0.0, L(o()), L(o()))), S(BIG, -1.0, L(o()), L(o())))]
    return [TM.flatten(t) for t in trees], TM.WEIGHTS[rng.integers(0, len(TM.WEIGHTS), len(trees))], 3


# dup_path's leaves that no row reaches: (tree, node), under every background their cover is 0
DUP_UNREACHED = ((2, 3), (3, 3), (4, 3), (4, 5), (5, 3), (7, 1))


def _dup_path():
    """trees whose paths test one feature two and three times, thresholds from TM.THRESHOLDS.  Trees 0, 1, 6, 8, 9: consistent repeats.
    Trees 2 and 3: contradictory ones (x <= 0.1 and then x > 1/3; x > 1/3 and then x <= 0.1).  Tree 4: the same threshold again below
    both children.  Tree 5: 0.0 and then -0.0, which are one value.  Tree 7: a NaN threshold, which sends every row right."""
    rng = np.random.default_rng(72)
    o = lambda: np.float32(rng.standard_normal())                       # noqa: E731
    T, third = TM, np.float32(1.0 / 3.0)
    trees = [S(1, third, S(1, 0.1, L(o()), L(o())), S(1, 1e7, L(o()), L(o()))),
             S(2, 0.30000001, S(2, 1e-3, S(2, 9.999999e-4, L(o()), L(o())), L(o())), L(o())),
             S(3, 0.1, S(3, third, L(o()), L(o())), L(o())),
             S(3, third, L(o()), S(3, 0.1, L(o()), L(o()))),
             S(4, 1e-40, S(4, 1e-40, L(o()), L(o())), S(4, 1e-40, L(o()), L(o()))),
             S(1, 0.0, S(1, -0.0, L(o()), L(o())), S(2, T.F32_MIN, L(o()), L(o()))),
             S(2, 16777216.0, S(3, 123456.79, S(2, 9999999.0, L(o()), L(o())), L(o())), S(2, np.inf, L(o()), L(o()))),
             S(4, np.nan, L(o()), S(4, -2.7182817, L(o()), L(o()))),
             S(3, T.F32_MIN_NORMAL, S(3, T.F32_MIN, S(3, -T.F32_MIN, L(o()), L(o())), L(o())), S(3, T.F32_MAX, L(o()), L(o()))),
             S(1, -T.F32_MAX, S(1, -np.inf, L(o()), L(o())), S(4, 0.1, L(o()), S(1, 1e-3, L(o()), L(o()))))]
    trees = [TM.flatten(t) for t in trees]
    known = set(TM.THRESHOLDS[~np.isnan(TM.THRESHOLDS)].view(np.uint32).tolist())
    for t in trees:
        th = t["threshold"][t["feature"] != -1]
        assert all(np.isnan(v) or int(v.view(np.uint32)) in known for v in th)
    return trees, TM.WEIGHTS[rng.integers(0, len(TM.WEIGHTS), len(trees))], 5


def _thresholds_deep():
    """TM.THRESHOLDS as random trees of depth 3, where the `thresholds` case has stumps: a path holds several edge thresholds on different
    features, which is what SHAP's per-path conditions need"""
    rng = np.random.default_rng(73)
    g = TM.Gen(rng, thresholds=TM.THRESHOLDS)
    trees = []
    while len(trees) < 24:
        t = TM.random_tree(g, int(rng.integers(4, 9)))
        if TM.depth_of(t) == 3:
            trees.append(t)
    return trees, TM.WEIGHTS[rng.integers(0, len(TM.WEIGHTS), len(trees))], 13


@functools.lru_cache(maxsize=None)
def model(name):
    """(trees, weights, the width of its rows) of a name of MODELS"""
    if name == "big_ids":
        return _big_ids()
    if name == "dup_path":
        return _dup_path()
    if name == "thresholds_deep":
        return _thresholds_deep()
    if name == "width":
        trees, weights, _ = TM._width_parts()
        return trees, weights, 20
    c = TM.CASES[name]()                         # the same generator calls as the scoring tests' case
    return c.trees, c.weights, c.rows.shape[1]


# ---- the five wrong rules: CR.walk with another comparison ------------------------------------------------------------------------------
def _flush(x):
    return np.float32(0) if abs(x) < TM.F32_MIN_NORMAL else x


def _six_digits(t):
    return t if not np.isfinite(t) else np.float32(float("%.6g" % float(t)))


def _zero_ordered(v, t):
    if v == 0 and t == 0:
        return bool(np.signbit(v)) or not np.signbit(t)           # -0.0 < +0.0
    return v <= t


RULES = {"lt": lambda v, t: v < t,
         "nan_left": lambda v, t: not (v > t),
         "flush_subnormals": lambda v, t: _flush(v) <= _flush(t),
         "zero_ordered": _zero_ordered,
         "six_digits": lambda v, t: v <= _six_digits(t)}


def leaf_under(tree, row, goes_left):
    """the leaf of CR.walk with `goes_left(value, threshold)` in place of `value <= threshold`"""
    feat, thr, left, right = tree["feature"], tree["threshold"], tree["left"], tree["right"]
    j = 0
    with np.errstate(invalid="ignore"):
        while feat[j] != -1:
            f = int(feat[j])
            v = row[f] if f < len(row) else np.float32(0)
            j = int(left[j]) if goes_left(v, thr[j]) else int(right[j])
    return j


def rows_changed(trees, rows, rule):
    """bool [rows]: the rule changes the leaf of the row in some tree"""
    right = lambda v, t: v <= t                                         # noqa: E731
    return np.array([any(leaf_under(t, r, RULES[rule]) != leaf_under(t, r, right) for t in trees) for r in rows], bool)


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
def _draw(name, seed):
    trees, _, width = model(name)
    k = len(TM.probe_pool(trees)) + len(TM.SPECIAL_VALUES)
    rng = np.random.default_rng([seed] + [ord(c) for c in name])
    n = k + max(MIXED, MIN_ROWS - k)
    rows = np.array(TM.probe_rows(rng, trees, n, width))              # the constant prefix, then the mixed part; column 0 is 0
    rows = rows[rng.permutation(n)]
    if name == "width":
        for c in range(width):
            if c not in (1, 3, 5, 12):
                rows[:, c] = np.nan                                     # columns no node reads, column 0 among them (as the case has it)
    if name == "col0_garbage":                                          # its own column 0, as the case has it
        rows[:, 0] = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 123.0], np.float32)[np.arange(n) % 7]
    if name == "feature_0":                                             # the model reads column 0: it holds values that matter, as the case has it
        rows[:, 0] = rows[:, 1][::-1]
    if name in EDGE_MODELS:
        rows = _rules_in_front(trees, rows)
    return np.ascontiguousarray(rows, np.float32)


def _rules_in_front(trees, rows, front=65):
    """every wrong rule must change a row among the first 65: a rule that changes none there gets the first row it does change swapped in
    from behind (a rule that changes no row at all gets pool rows added, which has not been needed)"""
    rows = rows.copy()
    masks = {r: rows_changed(trees, rows, r) for r in RULES}
    for r in RULES:
        if not masks[r].any():
            pool = np.concatenate([TM.SPECIAL_VALUES, TM.probe_pool(trees)])
            extra = np.repeat(pool[:, None], rows.shape[1], axis=1)
            extra[:, 0] = 0.0
            extra = extra[rows_changed(trees, extra, r)][:1]
            assert len(extra), r
            rows = np.concatenate([rows, extra])
            masks = {q: rows_changed(trees, rows, q) for q in RULES}
    spot = front - 1
    for r in RULES:
        if masks[r][:front].any():
            continue
        src = int(np.nonzero(masks[r])[0][0])
        while any(masks[q][:front].sum() == 1 and masks[q][spot] for q in RULES):     # (do not move a rule's only witness out)
            spot -= 1
        rows[[spot, src]] = rows[[src, spot]]
        for q in RULES:
            masks[q][[spot, src]] = masks[q][[src, spot]]
        spot -= 1
    return rows


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _model_rows(name):
    return _frozen(_draw(name, 1))


@functools.lru_cache(maxsize=None)
def _model_background(name):
    return _frozen(_draw(name, 2))


def _cut(case, rows):
    return _frozen(np.ascontiguousarray(rows[:, :int(case[6:])])) if case.startswith("width_") else rows


@functools.lru_cache(maxsize=None)
def rows(case):
    return _cut(case, _model_rows(model_of(case)))


@functools.lru_cache(maxsize=None)
def background(case):
    """a second draw of the same kind with another seed"""
    return _cut(case, _model_background(model_of(case)))


def trees_of(case):
    return model(model_of(case))[:2]


def row_counts(case):
    n = len(rows(case))
    return sorted({n if c is None else c for c in ROW_COUNTS})


def bg_counts(case):
    n = len(background(case))
    return sorted({n if c is None else min(c, n) for c in BG_COUNTS})


def read_columns(case):
    """the columns of the case's rows that its model reads"""
    return [f for f in CR.model_features(trees_of(case)[0]) if f < rows(case).shape[1]]


def not_constant(case):
    """bool [rows]: the columns from 1 on that the model reads do not all hold one bit pattern (column 0 is set apart in every set)"""
    cols = [c for c in read_columns(case) if c > 0]
    if not cols:
        return np.zeros(len(rows(case)), bool)
    b = rows(case)[:, cols].view(np.uint32)
    return (b != b[:, :1]).any(axis=1)


# ---- columns --------------------------------------------------------------------------------------------------------------------------
def column_choices(case):
    """the choices of tests/test_gpu_shap.py -- none, one, unused, subset, descending -- and what these models are for: feature 0 where
    the model has it, the two largest ids of big_ids, a column at and one beyond the row width"""
    trees = trees_of(case)[0]
    feats = CR.model_features(trees)
    width = rows(case).shape[1]
    out = {"none": None, "one": [feats[0]], "unused": [max(f for f in feats if f < BIG) + 7] + feats[:2], "subset": feats[1::2],
           "descending": sorted(feats, reverse=True)}
    if 0 in feats:
        out["feature_0"] = [0, feats[-1]]
    if model_of(case) == "big_ids":
        out["big"] = [BIG, 65536]
    if case.startswith("width_"):
        out["at_the_width"] = [width, 3 if width == 1 else 1]
        out["beyond_the_width"] = list(dict.fromkeys([12 if width <= 12 else width + 3, 5, width]))
    return out


def cell_columns(case):
    """the columns of the partial and permuted calls: three of the model's features (the first, the middle one, the last), feature 0
    where the model has it, and one column at the row width"""
    feats = CR.model_features(trees_of(case)[0])
    pick = [feats[0], feats[len(feats) // 2], feats[-1]]
    out = []
    for c in pick + [0] * (0 in feats) + [rows(case).shape[1]]:
        if c not in out:
            out.append(c)
    return out


def cell_grids(case):
    """PD.thresholds_grid of every column of cell_columns; PD.TWO where no tree tests it"""
    trees = trees_of(case)[0]
    out = []
    for c in cell_columns(case):
        g = PD.thresholds_grid(trees, c)
        out.append(PD.TWO if g is None else g)
    return out


def donors(case):
    """a permutation and a reversal, so constant and mixed rows swap values"""
    n = len(rows(case))
    return np.stack([np.random.default_rng(7).permutation(n), np.arange(n)[::-1]]).astype(np.int32)


def compact(trees, rows_, columns):
    """the model, the rows and the columns with the ids renamed to 0 .. k: the ids the rows hold keep their place, the others follow
    in ascending order and read 0.  The materialised restatements take a matrix as wide as the largest id; renamed, that of an id of
    2^31 - 1 is a few columns wide and the definition is the same."""
    width = rows_.shape[1]
    far = sorted({f for f in CR.model_features(trees) + [int(c) for c in columns] if f >= width})
    name = {f: width + i for i, f in enumerate(far)}
    out = []
    for t in trees:
        t = dict(t)
        t["feature"] = np.array([name.get(int(f), int(f)) for f in t["feature"]], np.int32)
        out.append(t)
    wide = np.zeros((len(rows_), width + len(far)), np.float32)
    wide[:, :width] = rows_
    return out, wide, [name.get(int(c), int(c)) for c in columns]


# ---- references, made once ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scores(case):
    trees, w = trees_of(case)
    return _frozen(TM.eval_ensemble_np(trees, w, rows(case)))


@functools.lru_cache(maxsize=None)
def paths(case):
    return CR.paths(trees_of(case)[0], rows(case))


@functools.lru_cache(maxsize=None)
def leaf_sums(case):
    trees, w = trees_of(case)
    return _frozen(CR.leaf_sums(trees, w, rows(case), paths(case)))


@functools.lru_cache(maxsize=None)
def covers(case, n_bg):
    return CR.covers_np(trees_of(case)[0], background(case)[:n_bg])


@functools.lru_cache(maxsize=None)
def contribs(case, n_bg, columns):
    trees, w = trees_of(case)
    return _frozen(CR.contribs(trees, w, CR.node_values(trees, covers(case, n_bg)), rows(case), list(columns), paths(case)))


@functools.lru_cache(maxsize=None)
def shap_terms(case, n_bg):
    trees, w = trees_of(case)
    mag = []
    return SR.terms(trees, w, covers(case, n_bg), rows(case), abs_leaf=mag), sum(mag)


@functools.lru_cache(maxsize=None)
def pair_terms(case, n_bg):
    trees, w = trees_of(case)
    return IR.pair_terms(trees, w, covers(case, n_bg), rows(case))


def shap(case, n_bg, columns):
    return SR.accumulate(shap_terms(case, n_bg)[0], len(rows(case)), list(columns))


def interactions(case, n_bg, columns):
    return IR.assemble(pair_terms(case, n_bg), shap(case, n_bg, columns), len(rows(case)), list(columns))


@functools.lru_cache(maxsize=None)
def partial(case):
    """(base, scores [cells][n], mean, shift2) by the materialised restatement, on the renamed model"""
    trees, w = trees_of(case)
    ct, cr, cc = compact(trees, rows(case), cell_columns(case))
    base, sc = PD.partial_scores(ct, w, cr, cc, cell_grids(case))
    mean, shift2 = PD.reduce_cells(base, sc)
    return tuple(_frozen(a) for a in (base, sc, mean, shift2))


@functools.lru_cache(maxsize=None)
def permuted(case):
    """(base, scores [C][R][n]) by the materialised restatement"""
    import permuted_restatement as PR
    trees, w = trees_of(case)
    return tuple(_frozen(a) for a in PR.permuted_scores(trees, w, rows(case), cell_columns(case), donors(case)))


def stages_of(case):
    n = len(trees_of(case)[0])
    return sorted({1, max(1, n // 2), n})
