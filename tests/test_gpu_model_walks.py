"""Every walk of a model's trees but the scoring kernels' own -- rl_model_cover, rl_model_predict_contribs, _leaf_sums, _shap,
_interactions, _stages, _partial and _permuted, each a loop of its own -- on the adversarial models of tests/walk_cases.py: thresholds
that are NaN, -0.0, subnormal, +-Float.MAX_VALUE or nine-digit decimals, row values one ulp beside them, feature 0, the feature ids 254,
255 and 2^31 - 1, rows narrower than the model, garbage in column 0.  The references are the project's restatements, which
tests/test_model_walks_cpu.py holds against something independent on these inputs first.  Every comparison is a bit pattern
(tree_models.same_scores for f32, contrib_restatement.same_f64 for f64: where the reference is NaN the kernel's value is NaN); there
is no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest

import contrib_restatement as CR
import partial_restatement as PD
import permuted_restatement as PR
import stages_restatement as ST
import tree_models as TM
import walk_cases as WC
from ranklib_amd import _native as N

pytestmark = pytest.mark.gpu

# the kernel rl_model_predict takes per model: tree_models' cases say it for theirs, the width family at every width
TILED = {"thresholds": True, "feature_0": False, "col0_garbage": True, "feat_254": True, "feat_255": False, "width": True}


@functools.lru_cache(maxsize=None)
def handle(name):
    """one handle per model of WC.MODELS, made once"""
    trees, w, _ = WC.model(name)
    return N.Model(TM.model_text(trees, w))


def fresh(name):
    trees, w, _ = WC.model(name)
    return N.Model(TM.model_text(trees, w))


def same32(got, want):
    return TM.same_scores(np.ravel(got), np.ravel(want)) if np.shape(got) == np.shape(want) else "shape %r != %r" % (np.shape(got), np.shape(want))


def scoring_path(m, rows):
    m.predict_rows(rows[:1])
    return m.path()


@functools.lru_cache(maxsize=None)
def donors_of(n):
    """a permutation and a reversal, so constant and mixed rows swap values"""
    return np.stack([np.random.default_rng(7).permutation(n), np.arange(n)[::-1]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def permuted_want(case, n):
    if n == len(WC.rows(case)):
        assert np.array_equal(donors_of(n), WC.donors(case))
        return WC.permuted(case)
    trees, w = WC.trees_of(case)
    return PR.permuted_scores(trees, w, WC.rows(case)[:n], WC.cell_columns(case), donors_of(n))


# ---- 1. covers and the three attributions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [0, 1, 2])
@pytest.mark.parametrize("case", WC.CASES)
def test_covers_and_attributions_equal_the_restatements(case, bg):
    trees, w = WC.trees_of(case)
    m, rows = handle(WC.model_of(case)), WC.rows(case)
    n_bg = WC.bg_counts(case)[bg]
    feats = CR.model_features(trees)
    m.cover(WC.background(case)[:n_bg])
    assert m.path() == N.MODEL_PATH_COVER and m.cover_rows() == n_bg
    cov = WC.covers(case, n_bg)
    for t, (c, v) in enumerate(zip(cov, CR.node_values(trees, cov))):
        gc, gv = m.cover_of(t)
        assert np.array_equal(gc, c), (case, n_bg, t, gc, c)
        assert CR.same_f64(gv, v) is None, (case, n_bg, t, CR.same_f64(gv, v))
    for what, cols in WC.column_choices(case).items():
        ids = feats if cols is None else cols
        want = {"contribs": WC.contribs(case, n_bg, tuple(ids)), "shap": WC.shap(case, n_bg, ids), "interactions": WC.interactions(case, n_bg, ids)}
        for n in WC.row_counts(case):
            for entry, path in (("contribs", N.MODEL_PATH_CONTRIBS), ("shap", N.MODEL_PATH_SHAP), ("interactions", N.MODEL_PATH_INTERACT)):
                got, gids = getattr(m, "predict_" + entry)(rows[:n], cols)
                assert m.path() == path and gids == ids
                assert CR.same_f64(got, want[entry][:n]) is None, (case, n_bg, what, n, entry, CR.same_f64(got, want[entry][:n]))
        if what == "unused":
            assert not want["shap"][:, 0].view(np.uint64).any() and not want["contribs"][:, 0].view(np.uint64).any()
    if n_bg and case != "width_1":                            # the requested features do get something: the comparison is not of zeros
        # (at width 1 every row and every background row reads 0 everywhere: one path, and nothing to attribute)
        assert WC.shap(case, n_bg, feats)[:, :len(feats)].any() and WC.contribs(case, n_bg, tuple(feats))[:, :len(feats)].any()


# ---- 2. the walks that score --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.CASES)
def test_leaf_sums_stages_partial_and_permuted_equal_the_restatements(case):
    trees, w = WC.trees_of(case)
    name = WC.model_of(case)
    m, rows = handle(name), WC.rows(case)
    cols, grids, stages = WC.cell_columns(case), WC.cell_grids(case), WC.stages_of(case)
    want_stage = ST.stage_scores(trees, w, rows, stages)
    pbase, psc = WC.partial(case)[:2]
    assert same32(want_stage[-1], WC.scores(case)) is None
    scoring = scoring_path(m, rows)
    if name in TILED:
        assert scoring == (N.MODEL_PATH_TILED if TILED[name] else N.MODEL_PATH_GENERIC)
    for n in WC.row_counts(case):
        r = rows[:n]
        score = m.predict_rows(r)
        assert m.path() == scoring and same32(score, WC.scores(case)[:n]) is None, (case, n, same32(score, WC.scores(case)[:n]))
        leaf = m.leaf_sums(r)
        assert m.path() == scoring                            # (the leaf sums have no path constant of their own: the call before stays)
        assert CR.same_f64(leaf, WC.leaf_sums(case)[:n]) is None, (case, n, CR.same_f64(leaf, WC.leaf_sums(case)[:n]))
        st = m.predict_stages(r, stages)
        assert m.path() == scoring and same32(st, want_stage[:, :n]) is None, (case, n, same32(st, want_stage[:, :n]))
        gb, gm, gs, gi = m.predict_partial(r, cols, grids, ice=True)
        assert m.path() == N.MODEL_PATH_PARTIAL
        assert same32(gb, pbase[:n]) is None and same32(gi, psc[:, :n]) is None, (case, n, same32(gi, psc[:, :n]))
        wm, ws = (WC.partial(case)[2:] if n == len(rows) else PD.reduce_cells(pbase[:n], psc[:, :n]))
        assert CR.same_f64(gm, wm) is None and CR.same_f64(gs, ws) is None, (case, n)
        wb, wp = permuted_want(case, n)
        qb, qp = m.predict_permuted(r, cols, donors_of(n))
        assert m.path() == N.MODEL_PATH_PERMUTED
        assert same32(qb, wb) is None and same32(qp, wp) is None, (case, n, same32(qp, wp))
        # without any restatement: the last stage, the partial base and the permuted base carry predict_rows' bits
        for other in (st[-1], gb, qb):
            assert np.array_equal(PD.bits32(other), PD.bits32(score)), (case, n)
    moved = (PD.bits32(psc) != PD.bits32(pbase)[None, :]).any(axis=1)      # the cells do move scores: the comparison is not of copies of the base
    assert moved.any()
    if case != "width_1":                                     # (rows of one column hold none that a donor could change: every cell is the base)
        assert (PD.bits32(WC.permuted(case)[1]) != PD.bits32(pbase)[None, None, :]).any()


# ---- 3. the width family, and garbage in column 0 -----------------------------------------------------------------------------------------
def everything(m, rows, bg, cols, grids, columns, stages):
    """every entry point's result on one handle: name -> array"""
    out = {}
    m.cover(bg)
    for t in range(m.num_trees()):
        out["cover_%d" % t], out["value_%d" % t] = m.cover_of(t)
    out["rows"] = m.predict_rows(rows)
    out["contribs"] = m.predict_contribs(rows, columns)[0]
    out["shap"] = m.predict_shap(rows, columns)[0]
    out["interactions"] = m.predict_interactions(rows, columns)[0]
    out["leaf_sums"] = m.leaf_sums(rows)
    out["stages"] = m.predict_stages(rows, stages)
    out["partial_base"], out["partial_mean"], out["partial_shift2"], out["partial_ice"] = m.predict_partial(rows, cols, grids, ice=True)
    out["permuted_base"], out["permuted"] = m.predict_permuted(rows, cols, donors_of(len(rows)))
    return out


def same_everything(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        nan = np.isnan(y) if y.dtype.kind == "f" else np.zeros(y.shape, bool)
        u = np.uint32 if y.dtype.itemsize == 4 else np.uint64
        assert np.where(nan, np.isnan(x) if y.dtype.kind == "f" else False, x.view(u) == y.view(u)).all(), k


def test_width_13_is_width_20():
    """columns beyond the model's largest feature change nothing: each width is a call of its own on rows[:, :w] made contiguous"""
    m = handle("width")
    cols, grids = [1, 5, 12, 13, 20], [PD.thresholds_grid(WC.model("width")[0], c) for c in (1, 5, 12)] + [PD.TWO, PD.TWO]
    stages = WC.stages_of("width_20")
    res = {w: everything(m, WC.rows("width_%d" % w), WC.background("width_%d" % w), cols, grids, [12, 1, 13, 20, 3], stages) for w in (20, 13, 12)}
    assert WC.rows("width_13").flags.c_contiguous and WC.rows("width_13").shape[1] == 13
    same_everything(res[13], res[20])
    assert not np.array_equal(PD.bits32(res[12]["rows"]), PD.bits32(res[20]["rows"]))      # (one column fewer is another matter: feature 12 reads 0)


def test_column_0_does_not_matter_where_no_tree_reads_it():
    m = handle("col0_garbage")
    rows, bg = WC.rows("col0_garbage"), WC.background("col0_garbage")
    assert np.isnan(rows[:, 0]).any() and np.isnan(bg[:, 0]).any()
    clean, clean_bg = rows.copy(), bg.copy()
    clean[:, 0] = 0.0
    clean_bg[:, 0] = 0.0
    cols, grids = WC.cell_columns("col0_garbage") + [0], WC.cell_grids("col0_garbage") + [PD.TWO]
    args = (cols, grids, None, WC.stages_of("col0_garbage"))
    same_everything(everything(m, rows, bg, *args), everything(m, clean, clean_bg, *args))


# ---- 4. the order of calls ----------------------------------------------------------------------------------------------------------------
def test_no_call_leaves_anything_behind_for_the_next():
    """one handle, the entry points in one order and in the reverse, a predict_rows between any two, then the covers of another
    background: the bits of every result are those of a fresh handle given only that call and its cover"""
    case = "thresholds_deep"
    rows, bg = WC.rows(case), WC.background(case)
    cols, grids, stages = WC.cell_columns(case), WC.cell_grids(case), WC.stages_of(case)
    calls = {"shap": lambda m: m.predict_shap(rows)[0], "interactions": lambda m: m.predict_interactions(rows)[0],
             "contribs": lambda m: m.predict_contribs(rows)[0], "stages": lambda m: m.predict_stages(rows, stages),
             "partial": lambda m: np.concatenate([np.ravel(a).view(np.uint8) for a in m.predict_partial(rows, cols, grids, ice=True)]),
             "permuted": lambda m: np.concatenate([np.ravel(a).view(np.uint8) for a in m.predict_permuted(rows, cols, donors_of(len(rows)))]),
             "leaf_sums": lambda m: m.leaf_sums(rows)}

    def alone(name, background):
        f = fresh(case)
        f.cover(background)
        return calls[name](f)

    def same(a, b):
        return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    want = {name: alone(name, bg[:257]) for name in calls}
    score = fresh(case).predict_rows(rows)
    m = fresh(case)
    m.cover(bg[:257])
    for name in list(calls) + list(calls)[::-1]:
        assert same(calls[name](m), want[name]), name
        assert same(m.predict_rows(rows), score), name
    m.cover(bg[:257])
    for t in range(m.num_trees()):
        assert np.array_equal(m.cover_of(t)[0], WC.covers(case, 257)[t])
    m.cover(bg[100:])                                         # another background: nothing of the first is left
    for name in ("shap", "interactions", "contribs"):
        got = calls[name](m)
        assert same(got, alone(name, bg[100:])) and not same(got, want[name]), name


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_these_models_by_code_and_message():
    """None of these models is refused by any entry point for its shape (the tests above call every one); what is refused on them is what
    include/rlhip.h promises for the arguments, with the path of the call before left as it was"""
    lib = N.lib()
    m = fresh("big_ids")
    rows = np.ascontiguousarray(WC.rows("big_ids")[:4])
    X = rows.ctypes.data
    out = np.zeros((4, 6, 6))
    O = out.ctypes.data                                           # noqa: E741
    twice, neg = np.array([WC.BIG, 65536, WC.BIG], np.int32), np.array([WC.BIG, -1], np.int32)

    def err(rc_want, rc, text, path):
        assert rc == rc_want and lib.rl_last_error().decode() == text, (rc, lib.rl_last_error().decode(), text)
        assert m.path() == path and not out.any()
    for entry in ("contribs", "shap", "interactions"):
        who = "rl_model_predict_%s: " % entry
        err(-3, getattr(lib, "rl_model_predict_" + entry)(m.h, X, 4, 3, None, 0, 0, O), who + "no rl_model_cover call has been made on this model",
            N.MODEL_PATH_NONE)
    m.cover(WC.background("big_ids"))
    for entry in ("contribs", "shap", "interactions"):
        who = "rl_model_predict_%s: " % entry
        fn = getattr(lib, "rl_model_predict_" + entry)
        err(-1, fn(m.h, X, 4, 3, twice.ctypes.data, 3, 0, O), who + "columns[2] = 2147483647 is listed twice", N.MODEL_PATH_COVER)
        err(-1, fn(m.h, X, 4, 3, neg.ctypes.data, 2, 0, O), who + "columns[1] = -1 is negative", N.MODEL_PATH_COVER)
    st = np.array([1, 11], np.int32)
    o32 = np.zeros((2, 4), np.float32)
    err(-1, lib.rl_model_predict_stages(m.h, X, 4, 3, st.ctypes.data, 2, o32.ctypes.data), "rl_model_predict_stages: stages[1] = 11 is outside [1, 10]",
        N.MODEL_PATH_COVER)
    with pytest.raises(N.RankLibError, match=r"rl_model_predict_partial: grid\[1\]\[1\] = nan is NaN"):
        m.predict_partial(rows, [WC.BIG, 65536], [[0.0], [0.0, np.nan]])
    with pytest.raises(N.RankLibError, match=r"rl_model_predict_partial: columns\[0\] = -2147483647 is negative"):
        m.predict_partial(rows, [-WC.BIG], [[0.0]])
    with pytest.raises(N.RankLibError, match=r"rl_model_predict_permuted: donor\[0\]\[3\] = 4 is outside \[0, 4\)"):
        m.predict_permuted(rows, [WC.BIG], [0, 1, 2, 4])
    assert m.path() == N.MODEL_PATH_COVER and not o32.any()
    got, ids = m.predict_interactions(rows, [WC.BIG, 65536])      # and the same arguments in order are taken
    assert m.path() == N.MODEL_PATH_INTERACT and ids == [WC.BIG, 65536] and got.shape == (4, 4, 4)
