"""The references of tests/test_gpu_model_walks.py on the ground they have not stood on -- thresholds that are NaN, -0.0, subnormal,
+-Float.MAX_VALUE or nine-digit decimals, row values one ulp beside them, feature 0, feature ids at the packing boundary and at
2^31 - 1, rows narrower than the model -- held against something independent of each, without a GPU, and the conditions on the inputs
of tests/walk_cases.py.  No comparison here takes a new tolerance: scores and walks are compared bit for bit, the attributions within
the bounds tests/test_shap_cpu.py (b) and tests/test_interact_cpu.py (b) measured."""
from fractions import Fraction

import numpy as np
import pytest

import contrib_restatement as CR
import interact_restatement as IR
import partial_restatement as PD
import permuted_restatement as PR
import shap_restatement as SR
import tree_models as TM
import walk_cases as WC

BRUTE_MODELS = ("thresholds", "thresholds_deep", "dup_path", "feature_0", "big_ids")
BRUTE_ROWS = 24


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WC.MODELS)
def test_the_wrong_rules_change_rows(name):
    """per model, the rows whose leaf each wrong rule changes in some tree, among the first 65 and among all.  On the three models that
    are there for the comparison's edges none may be 0."""
    case = "width_20" if name == "width" else name
    trees, rows = WC.trees_of(case)[0], WC.rows(case)
    for rule in WC.RULES:
        ch = WC.rows_changed(trees, rows, rule)
        print("%s: %s changes %d of the first 65 rows, %d of %d" % (name, rule, ch[:65].sum(), ch.sum(), len(rows)))
        if name in WC.EDGE_MODELS:
            assert ch[:65].any() and ch.any(), (name, rule)


@pytest.mark.parametrize("name", WC.MODELS)
def test_the_rows_are_what_the_recipe_says(name):
    case = "width_20" if name == "width" else name
    trees, rows, bg = WC.trees_of(case)[0], WC.rows(case), WC.background(case)
    k = len(TM.probe_pool(trees)) + len(TM.SPECIAL_VALUES)
    assert len(rows) >= max(k + WC.MIXED, WC.MIN_ROWS) and len(bg) == len(rows) and not np.array_equal(rows.view(np.uint32), bg.view(np.uint32))
    assert not rows.flags.writeable and not bg.flags.writeable
    mixed = WC.not_constant(case)
    print("%s: %d rows, %d of them not constant over the columns the model reads" % (name, len(rows), mixed.sum()))
    if name != "big_ids":                                    # (its rows hold two columns the model reads)
        assert 3 * mixed.sum() >= len(rows)
        for b in range(0, len(rows) - 63, 64):               # constant and mixed rows in every block of 64
            assert mixed[b:b + 64].any() and not mixed[b:b + 64].all(), (name, b)
    if name == "col0_garbage":
        assert np.isnan(rows[:, 0]).any() and np.isinf(rows[:, 0]).any() and 0 not in CR.model_features(trees)
    elif name == "feature_0":
        assert 0 in CR.model_features(trees) and len(np.unique(rows[:, 0])) > 20
    elif name == "width":
        assert np.isnan(rows[:, 0]).all() and CR.model_features(trees) == [1, 3, 5, 12]
    else:
        assert not rows[:, 0].view(np.uint32).any()
    assert WC.row_counts(case) == [1, 63, 64, 65, len(rows)] and WC.bg_counts(case) == [0, 257, len(bg)]


def test_the_models_hold_what_they_are_for():
    assert CR.model_features(WC.model("big_ids")[0]) == [1, 2, 65535, 65536, WC.BIG] and WC.model("big_ids")[2] == 3
    assert max(CR.model_features(WC.model("feat_254")[0])) == 254 and max(CR.model_features(WC.model("feat_255")[0])) == 255
    trees = WC.model("thresholds_deep")[0]
    assert {TM.depth_of(t) for t in trees} == {3}
    th = np.concatenate([t["threshold"][t["feature"] != -1] for t in trees])
    want = set(TM.THRESHOLDS[~np.isnan(TM.THRESHOLDS)].view(np.uint32).tolist())
    assert set(th[~np.isnan(th)].view(np.uint32).tolist()) == want and np.isnan(th).any()       # every threshold of the list, -0.0 and NaN among them
    several = 0
    for t in trees:
        for _, els in SR.leaf_elements(t, np.zeros(len(t["feature"]), np.uint64), SR.f64):
            several += len(els) >= 3
    assert several > 40                                       # paths of three distinct features
    trees = WC.model("dup_path")[0]
    twice = thrice = 0
    for t in trees:
        for _, els in SR.leaf_elements(t, np.zeros(len(t["feature"]), np.uint64), SR.f64):
            twice += any(len(e[2]) == 2 for e in els)
            thrice += any(len(e[2]) == 3 for e in els)
    assert twice >= 20 and thrice >= 4
    for n_bg in WC.bg_counts("dup_path"):                     # the contradictory paths' leaves: reached by no row, zero cover under every background
        cov = WC.covers("dup_path", n_bg)
        for t, j in WC.DUP_UNREACHED:
            assert trees[t]["feature"][j] == -1 and cov[t][j] == 0
        if n_bg:
            assert sum(int((c[t["feature"] == -1] == 0).sum()) for t, c in zip(trees, cov)) == len(WC.DUP_UNREACHED)      # and every other leaf is reached
    for t, j in WC.DUP_UNREACHED:
        assert all(p[t][-1] != j for p in WC.paths("dup_path"))


# ---- leaves -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.CASES)
def test_the_leaves_of_the_walk_give_the_scores(case):
    """the leaf CR.walk reaches, put through Ensemble.eval's f32 chain, gives TM.eval_ensemble_np's scores bit for bit"""
    trees, w = WC.trees_of(case)
    s = np.zeros(len(WC.rows(case)), np.float32)
    with np.errstate(all="ignore"):
        for t, (tree, wt) in enumerate(zip(trees, w)):
            out = np.array([tree["output"][p[t][-1]] for p in WC.paths(case)], np.float32)
            s = (s.astype(np.float64) + out.astype(np.float64) * np.float64(np.float32(wt))).astype(np.float32)
    assert TM.same_scores(s, WC.scores(case)) is None, TM.same_scores(s, WC.scores(case))
    if case.startswith("width_") and int(case[6:]) >= 13:
        assert TM.same_scores(WC.scores(case), WC.scores("width_20")) is None
    if case == "width_12":
        assert TM.same_scores(WC.scores(case), WC.scores("width_20")) is not None       # column 12 reads 0


# ---- covers -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.CASES)
def test_the_covers(case):
    trees = WC.trees_of(case)[0]
    bg = WC.background(case)
    cov = WC.covers(case, len(bg))
    for a, b, t in zip(CR.covers(trees, bg), cov, trees):
        assert np.array_equal(a, b)
        assert int(b[t["feature"] == -1].sum()) == len(bg) == int(b[0])
    assert all(not c.any() for c in WC.covers(case, 0))


# ---- SHAP and interaction values against the definition ---------------------------------------------------------------------------------------
def _gap(got, exact):
    return max(sum(abs(Fraction(float(g)) - e) for g, e in zip(gr.ravel(), er.ravel())) for gr, er in zip(got, exact))


@pytest.mark.parametrize("name", BRUTE_MODELS)
def test_shap_is_the_shapley_value(name):
    """the f64 run against the Shapley sum over subsets, within SR.BOUND times the model's magnitude"""
    trees, w = WC.trees_of(name)
    rows = WC.rows(name)[:BRUTE_ROWS]
    cov = WC.covers(name, len(WC.background(name)))
    feats = CR.model_features(trees)
    mag = []
    got = SR.shap(trees, w, cov, rows, feats, abs_leaf=mag)
    assert np.isfinite(got).all() and WC.not_constant(name)[:BRUTE_ROWS].any()
    gap = float(_gap(got, SR.brute(trees, w, cov, rows, feats)))
    print("%s: worst gap %.3g, %.3f x 2^-52 x sum |W out|" % (name, gap, gap / sum(mag) / SR.U))
    assert gap <= SR.BOUND * sum(mag)


@pytest.mark.parametrize("name", BRUTE_MODELS)
def test_interactions_are_the_interaction_index(name):
    """the same for the interaction values, on at most 4 requested columns so that the subsets stay few"""
    trees, w = WC.trees_of(name)
    rows = WC.rows(name)[:BRUTE_ROWS]
    cov = WC.covers(name, len(WC.background(name)))
    cols = CR.model_features(trees)[-4:]
    mag = []
    got = IR.interactions(trees, w, cov, rows, cols, abs_leaf=mag)
    assert np.isfinite(got).all()
    gap = float(_gap(got, IR.brute(trees, w, cov, rows, cols)))
    asym = float(np.abs(got - got.transpose(0, 2, 1)).max())
    print("%s: worst gap %.3f, worst asymmetry %.3f x 2^-52 x sum |W out|" % (name, gap / sum(mag) / IR.U, asym / sum(mag) / IR.U))
    assert gap <= IR.BOUND_GAP * sum(mag) and asym <= IR.BOUND_ASYM * sum(mag)


# ---- partial and permuted -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.CASES)
def test_the_path_rules_are_the_materialised_definitions(case):
    trees, w = WC.trees_of(case)
    rows, cols, grids = WC.rows(case), WC.cell_columns(case), WC.cell_grids(case)
    feats = CR.model_features(trees)
    assert rows.shape[1] in cols and (0 in cols) == (0 in feats) and sum(c in feats for c in cols) >= min(3, len(feats))
    base, sc = WC.partial(case)[:2]
    pb, ps = PD.partial_scores_path_rule(trees, w, rows, cols, grids)
    assert TM.same_scores(pb, base) is None and TM.same_scores(ps.ravel(), sc.ravel()) is None, TM.same_scores(ps.ravel(), sc.ravel())
    assert TM.same_scores(base, WC.scores(case)) is None
    base, sc = WC.permuted(case)
    pb, ps = PR.permuted_scores_path_rule(trees, w, rows, cols, WC.donors(case))
    assert TM.same_scores(pb, base) is None and TM.same_scores(ps.ravel(), sc.ravel()) is None, TM.same_scores(ps.ravel(), sc.ravel())
    assert TM.same_scores(base, WC.scores(case)) is None
    if case == "thresholds":                                  # the grids hold the edge values themselves
        held = set(np.concatenate(grids).view(np.uint32).tolist())
        for v in (TM.F32_MIN, np.float32(1e-40), TM.F32_MAX, -TM.F32_MAX):
            assert int(np.float32(v).view(np.uint32)) in held
    if case == "big_ids":
        at = sum(len(g) for g in grids[:cols.index(WC.BIG)])     # the id 2^31 - 1 at its lowest threshold, -1.0: the base reads 0 there
        assert grids[cols.index(WC.BIG)][0] == -1.0 and TM.same_scores(WC.partial(case)[1][at], WC.scores(case)) is not None


def test_the_renamed_model_is_the_model():
    """WC.compact renames ids; where the ids are small enough to materialise, the renamed model's partial scores are the model's"""
    trees, w = WC.trees_of("width_5")
    rows, cols, grids = WC.rows("width_5"), WC.cell_columns("width_5"), WC.cell_grids("width_5")
    assert max(cols) == 12 and rows.shape[1] == 5
    base, sc = PD.partial_scores(trees, w, rows, cols, grids)
    assert TM.same_scores(base, WC.partial("width_5")[0]) is None and TM.same_scores(sc.ravel(), WC.partial("width_5")[1].ravel()) is None
