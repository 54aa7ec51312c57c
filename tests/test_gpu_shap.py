"""Exact TreeSHAP contributions on the GPU (rl_model_predict_shap: k_model_shap, rl_shap.inc) against the f64 run of
tests/shap_restatement.py, the computed form of include/rlhip.h in plain NumPy.  Everything is compared as bit patterns; no tolerance
anywhere but local accuracy (where the reference value is NaN the kernel's is NaN: contrib_restatement.same_f64)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import contrib_restatement as CR
import shap_restatement as SR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import LambdaMART, MART, RankerFactory, java_double_str, java_float_str

pytestmark = pytest.mark.gpu

L, S = TM.L, TM.S
BG_COUNTS = (257, 5000, 0)
ROW_COUNTS = (1, 63, 64, 65, 257)                # both sides of a block of 64 documents, and of one of 256
WIDTH = 35                                       # the 30, 32 and 33 distinct features of the chains are all columns of the rows


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(autouse=True)
def _restore_statics():
    """the command line writes the evaluator's statics, as every command line here does"""
    from ranklib_amd.evaluator import Evaluator
    saved = (Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile)
    yield
    Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile = saved


def _single_leaves():
    rng = np.random.default_rng(31)
    g = TM.Gen(rng)
    return [TM.single_leaf(g) for _ in range(5)], np.array([0.1, 1.0, -0.25, 3.0, 0.5], np.float32)


def _tm(name):
    c = TM.case(name)[0]
    return c.trees, c.weights


MODELS = {"count_37": lambda: _tm("count_37"), "nodes_81": lambda: _tm("nodes_81"), "single_leaves": _single_leaves,
          "nan_leaf": lambda: _tm("nan_leaf"), "accum_specials": lambda: _tm("accum_specials"),
          "chain_left": lambda: CR.chain_model("left"), "chain_right": lambda: CR.chain_model("right", seed=6),
          "stump": lambda: CR.hand_stump()[:2], "and_tree": lambda: SR.and_tree()[:2], "distinct_30": lambda: SR.distinct_chain(30)}


@functools.lru_cache(maxsize=None)
def background():
    rows = CR.grid_rows(np.random.default_rng(41), max(BG_COUNTS), WIDTH)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def doc_rows():
    rows = CR.grid_rows(np.random.default_rng(42), ROW_COUNTS[-1], WIDTH)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def model(name):
    """the trees, the weights and the handle: made once"""
    trees, w = MODELS[name]()
    return trees, w, N.Model(TM.model_text(trees, w))


@functools.lru_cache(maxsize=None)
def reference(name, n_bg):
    """the covers of the background's first n_bg rows and what the chains of doc_rows() add under them: made once, whatever the columns"""
    trees, w, _ = model(name)
    cov = CR.covers_np(trees, background()[:n_bg])
    mag = []
    return cov, SR.terms(trees, w, cov, doc_rows(), abs_leaf=mag), sum(mag)


def column_choices(trees):
    feats = CR.model_features(trees)
    out = {"none": None, "one": [feats[0] if feats else 1], "unused": [max(feats, default=0) + 7] + feats[:2]}
    if len(feats) >= 2:
        out["subset"] = feats[1::2]
        out["descending"] = sorted(feats, reverse=True)
    return out


# ---- 1. the kernel is the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_shap_equals_the_restatement(name):
    trees, w, m = model(name)
    rows = doc_rows()
    feats = CR.model_features(trees)
    assert m.shap_limits() == (SR.max_path(trees), SR.P_LIMIT)
    for n_bg in BG_COUNTS:
        cov, terms, mag = reference(name, n_bg)
        m.cover(background()[:n_bg])
        saabas = m.predict_contribs(rows)[0]
        for what, cols in column_choices(trees).items():
            ids = feats if cols is None else cols
            want = SR.accumulate(terms, len(rows), ids)
            for n in ROW_COUNTS:
                got, gids = m.predict_shap(rows[:n], cols)
                assert m.path() == N.MODEL_PATH_SHAP and N.shap_passes() == 1
                assert gids == ids and got.shape == (n, len(ids) + 2) and got.dtype == np.float64
                assert CR.same_f64(got, want[:n]) is None, (name, n_bg, what, n, CR.same_f64(got, want[:n]))
            if cols is None:
                assert not u64(want[:, len(ids)]).any()                        # every feature has its slot: rest is +0.0, the bits
                assert CR.same_f64(got[:, -1], saabas[:, -1]) is None          # the bias slot: the bits of rl_model_predict_contribs'
                leaf = m.leaf_sums(rows)                                       # local accuracy, within the bound of the CPU test's (b)
                total = np.zeros(len(rows))
                with np.errstate(all="ignore"):
                    for c in range(got.shape[1]):
                        total = total + got[:, c]
                    ok = np.isfinite(leaf) & np.isfinite(total)
                    assert (np.abs(total - leaf)[ok] <= SR.BOUND * mag).all(), (name, n_bg, float(np.abs(total - leaf)[ok].max()), SR.BOUND * mag)
                # (a NaN or infinite leaf is met by every row, so those two models may leave no finite row to measure)
                assert ok.all() or name in ("nan_leaf", "accum_specials")
            if what == "unused":
                assert not u64(want[:, 0]).any()                               # a feature the model never splits on: +0.0
            if what == "subset" and n_bg:
                assert want[:, len(ids)].any()                                 # the other features' terms are in rest
    if name in ("nan_leaf", "accum_specials"):
        want = SR.accumulate(reference(name, 257)[1], len(rows), feats)
        assert not np.isfinite(want).all() and np.isfinite(want).any()
    if name == "single_leaves":
        only = SR.accumulate(reference(name, 257)[1], len(rows), [])
        assert feats == [] and not u64(only[:, 0]).any() and only[:, 1].all()   # single leaves add to bias only
    if name == "distinct_30":
        assert m.shap_limits()[0] == 30


def test_the_hand_cases():
    trees, w, bg = CR.hand_stump()
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    rows = np.array([[0, -3.0], [0, 0.0], [0, 7.0], [0, np.nan]], np.float32)
    got, ids = m.predict_shap(rows, [1])
    assert ids == [1] and u64(got).tolist() == u64([[-0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 0.0, 0.0]]).tolist()
    trees, w, bg = SR.and_tree()
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    rows = np.array([[0, 1.0, 1.0]], np.float32)
    got, _ = m.predict_shap(rows)
    assert abs(got[0, 0] - 0.375) <= 1e-15 and abs(got[0, 1] - 0.375) <= 1e-15 and got[0, 2] == 0.0 and got[0, 3] == 0.25
    assert m.predict_contribs(rows)[0][0].tolist() == [0.25, 0.5, 0.0, 0.25]     # Saabas: the lower feature gets the larger share


def test_a_requested_column_at_or_beyond_row_stride_that_the_model_splits_on():
    """the background has the column, the rows do not: every row reads 0 there"""
    trees, w, m = model("count_37")
    cov = reference("count_37", 257)[0]
    m.cover(background()[:257])
    narrow = np.ascontiguousarray(doc_rows()[:, :6])
    feats = CR.model_features(trees)
    cols = [f for f in feats if f >= 6][:2] + [2]
    assert len(cols) == 3
    want = SR.shap(trees, w, cov, narrow, cols)
    assert want[:, 0].any() and not np.array_equal(u64(want), u64(SR.accumulate(reference("count_37", 257)[1], 257, cols)))
    got, _ = m.predict_shap(narrow, cols)
    assert CR.same_f64(got, want) is None, CR.same_f64(got, want)


# ---- 2. column passes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide():
    """test_gpu_contribs.py's model, by the same generator calls: 200 trees of 5 nodes that between them split on 400 distinct features,
    ids 1 .. 400, over 70 rows.  402 slots; beside w[3][64] a block of 64 documents holds 312"""
    rng = np.random.default_rng(9)
    order = rng.permutation(400) + 1
    th = lambda: np.float32(rng.choice(TM.GRID))                       # noqa: E731
    out = lambda: np.float32(rng.standard_normal())                    # noqa: E731
    trees = [TM.flatten(S(int(order[2 * i]), th(), L(out()), S(int(order[2 * i + 1]), th(), L(out()), L(out())))) for i in range(200)]
    w = TM.WEIGHTS[rng.integers(0, len(TM.WEIGHTS), 200)]
    bg = CR.grid_rows(rng, 90, 401)
    rows = CR.grid_rows(rng, 70, 401)
    cov = CR.covers_np(trees, bg)
    terms = SR.terms(trees, w, cov, rows)
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    return trees, w, rows, terms, m


def test_more_slots_than_the_lds_holds_take_several_column_passes():
    trees, w, rows, terms, m = wide()
    assert m.shap_limits()[0] == 2 and SR.slot_limit(3, 64) == 312 < 400 + 2
    want = SR.accumulate(terms, len(rows), list(range(1, 401)))
    got, ids = m.predict_shap(rows)
    assert N.shap_passes() == 2 and N.shap_passes() > 1 and ids == list(range(1, 401))
    assert CR.same_f64(got, want) is None, CR.same_f64(got, want)
    pick = sorted(np.random.default_rng(3).choice(400, 20, replace=False) + 1)
    one, _ = m.predict_shap(rows, pick)
    assert N.shap_passes() == 1                                            # 22 slots: one pass, blocks of 256
    assert np.array_equal(u64(one[:, :20]), u64(got[:, [p - 1 for p in pick]])) and np.array_equal(u64(one[:, 21]), u64(got[:, 401]))
    mid = list(range(400, 250, -1))                                        # 152 slots: one pass, blocks of 128
    assert SR.slot_limit(3, 256) < 152 <= SR.slot_limit(3, 128)
    two, _ = m.predict_shap(rows, mid)
    assert N.shap_passes() == 1
    assert np.array_equal(u64(two[:, :150]), u64(got[:, [p - 1 for p in mid]]))
    assert CR.same_f64(two, SR.accumulate(terms, len(rows), mid)) is None


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------------------
def test_row_chunks_change_no_bit():
    trees, w, m = model("count_37")
    m.cover(background()[:257])
    rows = doc_rows()
    feats = CR.model_features(trees)
    whole, _ = m.predict_shap(rows)
    per_row = WIDTH * 4 + 8 * (len(feats) + 2)
    three, _ = m.predict_shap(rows, scratch_bytes=per_row * 100)          # 100 + 100 + 57 rows
    assert np.array_equal(u64(three), u64(whole))
    each, _ = m.predict_shap(rows[:5], scratch_bytes=1)                    # a chunk holds at least one row
    assert np.array_equal(u64(each), u64(whole[:5]))
    assert CR.same_f64(whole, SR.accumulate(reference("count_37", 257)[1], 257, feats)) is None


# ---- 4. the path limit ---------------------------------------------------------------------------------------------------------------------
def test_a_path_of_32_distinct_features_is_taken_and_one_of_33_is_refused():
    rows, bg = doc_rows()[:65], background()[:5000]
    trees, w = SR.distinct_chain(SR.P_LIMIT, seed=13)
    m = N.Model(TM.model_text(trees, w))
    assert m.shap_limits() == (SR.P_LIMIT, SR.P_LIMIT) and len(trees[0]["feature"]) == 2 * 33 - 1
    m.cover(bg)
    cov = CR.covers_np(trees, bg)
    got, ids = m.predict_shap(rows)
    want = SR.shap(trees, w, cov, rows, ids)
    assert len(ids) == 32 and CR.same_f64(got, want) is None, CR.same_f64(got, want)
    trees, w = SR.distinct_chain(SR.P_LIMIT + 1, seed=14)
    m = N.Model(TM.model_text(trees, w))
    assert m.shap_limits() == (SR.P_LIMIT + 1, SR.P_LIMIT)
    m.cover(bg)
    lib, out = N.lib(), np.zeros((65, 35))
    assert lib.rl_model_predict_shap(m.h, rows.ctypes.data, 65, WIDTH, None, 0, 0, out.ctypes.data) == -4          # RL_ERR_UNSUPPORTED
    assert lib.rl_last_error().decode() == "rl_model_predict_shap: the path to leaf 0 (node 33) of tree 0 holds 33 distinct features, more than 32"
    assert m.path() == N.MODEL_PATH_COVER and not out.any()                  # refused before any launch
    assert m.predict_contribs(rows)[0].shape == (65, 35)                     # Saabas' walk has no such limit


# ---- 5. against the public path ------------------------------------------------------------------------------------------------------------
def letor_text(rows, lab, qoff):
    out = []
    for q in range(len(qoff) - 1):
        for i in range(qoff[q], qoff[q + 1]):
            out.append("%d qid:q%d %s\n" % (int(lab[i]), q, " ".join("%d:%s" % (f, java_float_str(rows[i, f])) for f in range(1, rows.shape[1]))))
    return "".join(out)


@pytest.mark.parametrize("head, cls", [("## LambdaMART", LambdaMART), ("## MART", MART)])
def test_the_rankers_and_the_command_line(head, cls, tmp_path):
    trees, w, _ = model("count_37")
    rng = np.random.default_rng(17)
    text = TM.model_text(trees, w).replace("## LambdaMART", head, 1)
    files = {}
    for nm, lens in (("bg", [40, 3, 77, 30]), ("test", [5, 1, 64, 20])):
        qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        rows = rng.choice(TM.GRID, (int(qoff[-1]), 13)).astype(np.float32)
        rows[:, 0] = 0.0
        path = str(tmp_path / (nm + ".txt"))
        with open(path, "w") as f:
            f.write(letor_text(rows, rng.integers(0, 5, len(rows)), qoff))
        files[nm] = (path, rows, qoff)
    mpath = str(tmp_path / "model.txt")
    with open(mpath, "w") as f:
        f.write(text)
    ranker = RankerFactory().loadRankerFromString(text)
    assert type(ranker) is cls
    direct = N.Model(text)
    direct.cover(files["bg"][1])
    for feats in (None, [7, 2, 30]):
        want, wids = direct.predict_shap(files["test"][1], feats)
        got, ids = ranker.contributions(FeatureManager.readInput(files["test"][0]), FeatureManager.readInput(files["bg"][0]), features=feats,
                                        exact=True)
        assert ids == wids and np.array_equal(u64(got), u64(want))
        saabas, _ = ranker.contributions(FeatureManager.readInput(files["test"][0]), None, features=feats)      # exact=False: today's call
        assert np.array_equal(u64(saabas), u64(direct.predict_contribs(files["test"][1], feats)[0])) and not np.array_equal(u64(saabas), u64(got))
    assert CR.same_f64(want, SR.shap(trees, w, CR.covers_np(trees, files["bg"][1]), files["test"][1], [7, 2, 30])) is None
    fpath = str(tmp_path / "features.txt")
    with open(fpath, "w") as f:
        f.write("7\n2\n30\n")
    out, summ = str(tmp_path / "contribs.tsv"), str(tmp_path / "summary.tsv")
    assert CL.main(["-load", mpath, "-background", files["bg"][0], "-test", files["test"][0], "-feature", fpath, "-exact", "-out", out,
                    "-summary", summ]) == 0
    scores = direct.predict_rows(files["test"][1])
    qoff = files["test"][2]
    lines = open(out).read().splitlines()
    assert len(lines) == len(scores)
    d = 0
    for q in range(len(qoff) - 1):
        for k in range(qoff[q + 1] - qoff[q]):
            cells = lines[d].split("\t")
            assert cells[:3] == ["q%d" % q, str(k), java_float_str(scores[d])]
            assert cells[3:] == ["%s:%s" % (nm, java_double_str(float(v))) for nm, v in zip(["7", "2", "30", "rest", "bias"], want[d])]
            d += 1
    n = len(scores)
    mean = lambda c: (math.fsum(abs(float(v)) for v in want[:, c]) / n, math.fsum(float(v) for v in want[:, c]) / n)      # noqa: E731
    feat = sorted(((f,) + mean(c) for c, f in enumerate([7, 2, 30])), key=lambda r: (-r[1], r[0]))
    assert open(summ).read().splitlines() == ["%d\t%s\t%s" % (f, java_double_str(a), java_double_str(s)) for f, a, s in feat]
    assert feat[-1][0] == 30 and feat[-1][1] == 0.0                        # a feature the model does not have
    fresh = RankerFactory().loadRankerFromString(text)                     # no covers yet: refused even with nothing to explain
    with pytest.raises(N.RankLibError, match="rl_model_predict_shap: no rl_model_cover call has been made on this model"):
        fresh.contributions([], None, exact=True)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    trees, w, _ = model("count_37")
    m = N.Model(TM.model_text(trees, w))
    lib = N.lib()
    rows, out = np.zeros((4, WIDTH), np.float32), np.zeros((4, 5))
    cols, neg, twice = np.array([1, 2, 3], np.int32), np.array([1, -2, 3], np.int32), np.array([1, 2, 3, 2], np.int32)

    def err(rc_want, rc, text):
        assert rc == rc_want and lib.rl_last_error().decode() == text, (rc, lib.rl_last_error().decode(), text)
    X, O, cp = rows.ctypes.data, out.ctypes.data, cols.ctypes.data
    who = "rl_model_predict_shap: "
    err(-3, lib.rl_model_predict_shap(m.h, X, 4, WIDTH, cp, 3, 0, O), who + "no rl_model_cover call has been made on this model")
    assert m.path() == N.MODEL_PATH_NONE and m.shap_limits() == (SR.max_path(trees), 32)         # the limits need no cover
    m.cover(rows)
    for args, text in (((None, X, 4, WIDTH, cp, 3, 0, O), "null model"), ((m.h, None, 4, WIDTH, cp, 3, 0, O), "null X"),
                       ((m.h, X, 4, WIDTH, cp, 3, 0, None), "null output"), ((m.h, X, -1, WIDTH, cp, 3, 0, O), "n_docs must be >= 0"),
                       ((m.h, X, 4, 0, cp, 3, 0, O), "row_stride must be >= 1"), ((m.h, X, 4, WIDTH, None, -1, 0, O), "n_columns must be >= 0"),
                       ((m.h, X, 4, WIDTH, cp, 0, 0, O), "n_columns must be >= 1 with columns given"),
                       ((m.h, X, 4, WIDTH, neg.ctypes.data, 3, 0, O), "columns[1] = -2 is negative"),
                       ((m.h, X, 4, WIDTH, twice.ctypes.data, 4, 0, O), "columns[3] = 2 is listed twice"),
                       ((m.h, X, 4, WIDTH, cp, 3, -1, O), "scratch_bytes must be >= 0")):
        err(-1, lib.rl_model_predict_shap(*args), who + text)
    err(-4, lib.rl_model_predict_shap(m.h, X, 2 ** 31, WIDTH, cp, 3, 0, O), who + "more than 2^31 documents per call")
    assert m.path() == N.MODEL_PATH_COVER
    a = C.c_int32(0)
    err(-1, lib.rl_model_shap_limits(m.h, None, C.byref(a)), "rl_model_shap_limits: null argument")
    with pytest.raises(N.RankLibError, match="columns\\[1\\] = 5 is listed twice"):
        m.predict_shap(rows, [5, 5])
    with pytest.raises(N.RankLibError, match="n_columns must be >= 1 with columns given"):
        m.predict_shap(rows, [])
    empty = N.Model("<ensemble>\n</ensemble>\n")
    with pytest.raises(N.RankLibError, match="rl_model_predict_shap: the model has no trees"):
        empty.predict_shap(rows)
    got, ids = m.predict_shap(rows[:0])                                    # no rows: legal, nothing to do
    assert got.shape == (0, len(CR.model_features(trees)) + 2) and m.path() == N.MODEL_PATH_COVER
    got, ids = m.predict_shap(rows)
    assert m.path() == N.MODEL_PATH_SHAP and N.shap_times() >= 0.0


def test_random_forests_and_linear_models_are_refused():
    trees, w, _ = model("count_37")
    body = TM.model_text(trees[:9], w[:9])
    forest = RankerFactory().loadRankerFromString("## Random Forests\n## No. of bags = 1\n\n" + body.split("\n\n", 1)[1])
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Random Forests model has no trees of one ensemble: "
                                             "a forest is several ensembles averaged"):
        forest.contributions([], [], exact=True)
    lin = RankerFactory().loadRankerFromString("## Coordinate Ascent\n## Restart = 5\n2:0.5 4:-0.25 6:0.125")
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        lin.contributions([], [], exact=True)
