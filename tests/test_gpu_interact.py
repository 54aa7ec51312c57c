"""SHAP interaction values on the GPU (rl_model_predict_interactions: k_model_interact, k_interact_finish, rl_interact.inc)
against the f64 run of tests/interact_restatement.py, the computed form of include/rlhip.h in plain NumPy.  Everything is compared as
bit patterns (where the reference value is NaN the kernel's is NaN: contrib_restatement.same_f64); the only tolerances are those of the
three properties -- row sums, symmetry, the cells' sum -- which take the bounds tests/test_interact_cpu.py (b) measured."""
import ctypes as C
import functools

import numpy as np
import pytest

import contrib_restatement as CR
import interact_restatement as IR
import shap_restatement as SR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import LambdaMART, MART, Ranker, RankerFactory, java_double_str, java_float_str

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


# the models, backgrounds and rows of tests/test_gpu_shap.py, by the same generator calls
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
    """the covers of the background's first n_bg rows and what the chains of doc_rows() add under them -- the SHAP slots' terms and the
    off-diagonal cells' pair terms: made once, whatever the columns"""
    trees, w, _ = model(name)
    cov = CR.covers_np(trees, background()[:n_bg])
    mag = []
    return cov, SR.terms(trees, w, cov, doc_rows()), IR.pair_terms(trees, w, cov, doc_rows(), abs_leaf=mag), sum(mag)


def want_of(ref, n, ids):
    return IR.assemble(ref[2], SR.accumulate(ref[1], n, ids), n, ids)


def column_choices(trees):
    feats = CR.model_features(trees)
    out = {"none": None, "one": [feats[0] if feats else 1], "unused": [max(feats, default=0) + 7] + feats[:2]}
    if len(feats) >= 2:
        out["subset"] = feats[1::2]
        out["descending"] = sorted(feats, reverse=True)
    return out


def diagonal_by_the_chain(got, phi):
    """the diagonal and the bias row and column from the off-diagonal cells and rl_model_predict_shap's values, by the stated chain"""
    n, S_, _ = got.shape
    out = got.copy()
    with np.errstate(all="ignore"):
        for i in range(S_ - 1):
            r = phi[:, i].copy()
            for j in range(S_ - 1):
                if j != i:
                    r = r - got[:, i, j]
            out[:, i, i] = r
    out[:, S_ - 1, :] = 0.0
    out[:, :, S_ - 1] = 0.0
    out[:, S_ - 1, S_ - 1] = phi[:, S_ - 1]
    return out


# ---- 1. the kernel is the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_interactions_equal_the_restatement(name):
    trees, w, m = model(name)
    rows = doc_rows()
    feats = CR.model_features(trees)
    for n_bg in BG_COUNTS:
        ref = reference(name, n_bg)
        mag = ref[3]
        m.cover(background()[:n_bg])
        for what, cols in column_choices(trees).items():
            ids = feats if cols is None else cols
            want = want_of(ref, len(rows), ids)
            for n in ROW_COUNTS:
                got, gids = m.predict_interactions(rows[:n], cols)
                assert m.path() == N.MODEL_PATH_INTERACT and N.interact_passes() == 1
                assert gids == ids and got.shape == (n, len(ids) + 2, len(ids) + 2) and got.dtype == np.float64
                assert CR.same_f64(got, want[:n]) is None, (name, n_bg, what, n, CR.same_f64(got, want[:n]))
            phi = m.predict_shap(rows, cols)[0]                            # diagonal and bias from the same handle's SHAP values
            assert CR.same_f64(got, diagonal_by_the_chain(got, phi)) is None, (name, n_bg, what)
            C_ = len(ids)
            assert not u64(got[:, C_ + 1, :C_ + 1]).any() and not u64(got[:, :C_ + 1, C_ + 1]).any()      # the bias row and column: +0.0
            if cols is None:
                assert not u64(got[:, C_, :]).any() and not u64(got[:, :, C_]).any()       # rest: +0.0, the bits, row and column
            if what == "unused":
                assert not u64(got[:, 0, :]).any() and not u64(got[:, :, 0]).any()         # a feature the model never splits on
            with np.errstate(all="ignore"):                                # the three properties, within the bounds of the CPU test's (b)
                rs = np.zeros((len(rows), C_ + 2))
                for c in range(C_ + 2):
                    rs = rs + got[:, :, c]
                total = np.zeros(len(rows))
                for c in range(C_ + 2):
                    total = total + rs[:, c]
                leaf = m.leaf_sums(rows)
                asym = np.abs(got - got.transpose(0, 2, 1))
                ok = np.isfinite(leaf) & np.isfinite(total)
                figures = (float(np.abs(rs - phi)[ok].max(initial=0.0)), float(asym[ok].max(initial=0.0)), float(np.abs(total - leaf)[ok].max(initial=0.0)))
            print("%s bg %d %s: row sums %.3g, asymmetry %.3g, cells' sum %.3g of 2^-52 x %.3g" % ((name, n_bg, what) + tuple(
                f / (IR.U * mag) if mag else f for f in figures) + (mag,)))
            if ok.any():                                                   # (no finite row: nothing to measure, and the unit itself is not finite)
                assert figures[0] <= IR.BOUND_GAP * mag and figures[1] <= IR.BOUND_ASYM * mag and figures[2] <= IR.BOUND_GAP * mag, (name, n_bg, what, figures)
            # (a NaN or infinite leaf is met by every row, so those two models may leave no finite row to measure)
            assert ok.all() or name in ("nan_leaf", "accum_specials")
            if what == "subset" and n_bg and name not in ("stump", "and_tree"):
                assert want[:, C_, :C_].any() or want[:, C_, C_].any()             # the other features are in rest
    if name == "single_leaves":
        only = want_of(reference(name, 257), len(rows), [])
        assert feats == [] and only.shape == (257, 2, 2) and not u64(only[:, 0, :]).any() and not u64(only[:, 1, 0]).any() and only[:, 1, 1].all()
    if name == "distinct_30":
        assert m.shap_limits()[0] == 30


def test_the_hand_cases():
    trees, w, bg = SR.and_tree()
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    got, ids = m.predict_interactions(np.array([[0, 1.0, 1.0]], np.float32))
    assert ids == [1, 2]
    assert u64(got[0]).tolist() == u64([[0.25, 0.125, 0.0, 0.0], [0.125, 0.25, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.25]]).tolist()
    trees, w, bg = CR.hand_stump()
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    rows = np.array([[0, -3.0], [0, 0.0], [0, 7.0], [0, np.nan]], np.float32)
    got, ids = m.predict_interactions(rows, [1])
    want = np.zeros((4, 3, 3))
    want[:, 0, 0] = [-0.5, -0.5, 1.5, 1.5]                                # the diagonal is the SHAP value, every other cell +0.0
    assert ids == [1] and u64(got).tolist() == u64(want).tolist()


def test_a_requested_column_at_or_beyond_row_stride_that_the_model_splits_on():
    """the background has the column, the rows do not: every row reads 0 there"""
    trees, w, m = model("count_37")
    cov = reference("count_37", 257)[0]
    m.cover(background()[:257])
    narrow = np.ascontiguousarray(doc_rows()[:, :6])
    feats = CR.model_features(trees)
    cols = [f for f in feats if f >= 6][:2] + [2]
    assert len(cols) == 3
    want = IR.interactions(trees, w, cov, narrow, cols)
    assert want[:, 0, 1:4].any() and not np.array_equal(u64(want), u64(want_of(reference("count_37", 257), 257, cols)))
    got, _ = m.predict_interactions(narrow, cols)
    assert CR.same_f64(got, want) is None, CR.same_f64(got, want)


# ---- 2. column passes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide():
    """test_gpu_contribs.py's model, by the same generator calls: 200 trees of 5 nodes that between them split on 400 distinct features,
    ids 1 .. 400, over 65 of its 70 rows.  401 attributed slots; beside w[2][64] a block of 64 documents holds 313"""
    rng = np.random.default_rng(9)
    order = rng.permutation(400) + 1
    th = lambda: np.float32(rng.choice(TM.GRID))                       # noqa: E731
    out = lambda: np.float32(rng.standard_normal())                    # noqa: E731
    trees = [TM.flatten(S(int(order[2 * i]), th(), L(out()), S(int(order[2 * i + 1]), th(), L(out()), L(out())))) for i in range(200)]
    w = TM.WEIGHTS[rng.integers(0, len(TM.WEIGHTS), 200)]
    bg = CR.grid_rows(rng, 90, 401)
    rows = CR.grid_rows(rng, 70, 401)[:65]
    cov = CR.covers_np(trees, bg)
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    return trees, w, rows, SR.terms(trees, w, cov, rows), IR.pair_terms(trees, w, cov, rows), m


def test_more_attributed_slots_than_the_lds_holds_take_several_column_passes():
    trees, w, rows, terms, pairs, m = wide()
    assert m.shap_limits()[0] == 2 and IR.slot_limit(2, 64) == 313 < 400 + 1
    ids = list(range(1, 401))
    want = IR.assemble(pairs, SR.accumulate(terms, len(rows), ids), len(rows), ids)
    got, gids = m.predict_interactions(rows)
    assert N.interact_passes() == 2 and gids == ids and got.shape == (65, 402, 402)
    assert CR.same_f64(got, want) is None, CR.same_f64(got, want)
    assert np.count_nonzero(got[:, :400, :400]) > 65 * 400                  # (every tree pairs two features)
    pick = sorted(np.random.default_rng(3).choice(400, 20, replace=False) + 1)
    one, _ = m.predict_interactions(rows, pick)
    assert N.interact_passes() == 1                                        # 21 attributed slots: one pass, blocks of 256
    at = [p - 1 for p in pick]
    off = ~np.eye(20, dtype=bool)
    assert np.array_equal(u64(one[:, :20, :20][:, off]), u64(got[:, at][:, :, at][:, off]))      # the off-diagonal cells keep their bits
    assert np.array_equal(u64(one[:, 21, 21]), u64(got[:, 401, 401]))
    assert CR.same_f64(one, IR.assemble(pairs, SR.accumulate(terms, len(rows), pick), len(rows), pick)) is None
    mid = list(range(400, 250, -1))                                        # 151 attributed slots: one pass, blocks of 128
    assert IR.slot_limit(2, 256) < 151 <= IR.slot_limit(2, 128)
    two, _ = m.predict_interactions(rows, mid)
    assert N.interact_passes() == 1
    assert CR.same_f64(two, IR.assemble(pairs, SR.accumulate(terms, len(rows), mid), len(rows), mid)) is None


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------------------
def test_row_chunks_change_no_bit():
    trees, w, m = model("count_37")
    m.cover(background()[:257])
    rows = doc_rows()
    feats = CR.model_features(trees)
    whole, _ = m.predict_interactions(rows)
    per_row = WIDTH * 4 + 8 * (len(feats) + 2) ** 2 + 8 * (len(feats) + 2)
    assert IR.chunk_rows(257, WIDTH, len(feats), per_row * 100) == 100
    three, _ = m.predict_interactions(rows, scratch_bytes=per_row * 100)   # 100 + 100 + 57 rows
    assert np.array_equal(u64(three), u64(whole))
    each, _ = m.predict_interactions(rows[:5], scratch_bytes=1)            # a chunk holds at least one row
    assert np.array_equal(u64(each), u64(whole[:5]))
    assert CR.same_f64(whole, want_of(reference("count_37", 257), 257, feats)) is None


# ---- 4. the path limit ---------------------------------------------------------------------------------------------------------------------
def test_a_path_of_32_distinct_features_is_taken_and_one_of_33_is_refused():
    rows, bg = doc_rows()[:65], background()[:5000]
    trees, w = SR.distinct_chain(SR.P_LIMIT, seed=13)
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    cov = CR.covers_np(trees, bg)
    got, ids = m.predict_interactions(rows)
    want = IR.interactions(trees, w, cov, rows, ids)
    assert len(ids) == 32 and CR.same_f64(got, want) is None, CR.same_f64(got, want)
    trees, w = SR.distinct_chain(SR.P_LIMIT + 1, seed=14)
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    lib, out = N.lib(), np.zeros((65, 35, 35))
    assert lib.rl_model_predict_interactions(m.h, rows.ctypes.data, 65, WIDTH, None, 0, 0, out.ctypes.data) == -4          # RL_ERR_UNSUPPORTED
    assert lib.rl_last_error().decode() == ("rl_model_predict_interactions: the path to leaf 0 (node 33) of tree 0 holds 33 distinct features, "
                                            "more than 32")
    assert m.path() == N.MODEL_PATH_COVER and not out.any()                  # refused before any launch


# ---- 5. against the public path ------------------------------------------------------------------------------------------------------------
def letor_text(rows, lab, qoff):
    out = []
    for q in range(len(qoff) - 1):
        for i in range(qoff[q], qoff[q + 1]):
            out.append("%d qid:q%d %s\n" % (int(lab[i]), q, " ".join("%d:%s" % (f, java_float_str(rows[i, f])) for f in range(1, rows.shape[1]))))
    return "".join(out)


def pairs_restated(ids, inter):
    """the -interactions lines from interaction values [docs][C + 2][C + 2] of the whole file: every sum one serial f64 chain in file
    order from +0.0, divided once"""
    n, C_ = len(inter), len(ids)
    lines = []
    for i in range(C_):
        for j in range(i, C_):
            a = s = np.float64(0.0)
            for d in range(n):
                v = inter[d, i, i] if i == j else inter[d, i, j] + inter[d, j, i]
                a, s = a + abs(v), s + v
            lines.append((float(a) / n, float(s) / n, ids[i], ids[j]))
    lines.sort(key=lambda r: (-r[0], r[2], r[3]))
    return ["%d\t%d\t%s\t%s" % (fi, fj, java_double_str(a), java_double_str(s)) for a, s, fi, fj in lines]


@pytest.mark.parametrize("head, cls", [("## LambdaMART", LambdaMART), ("## MART", MART)])
def test_the_rankers_and_the_command_line(head, cls, tmp_path, monkeypatch):
    trees, w, _ = model("count_37")
    rng = np.random.default_rng(17)
    text = TM.model_text(trees, w).replace("## LambdaMART", head, 1)
    files = {}
    for nm, lens in (("bg", [40, 3, 77, 30]), ("test", [5, 1, 20])):      # a test file of three lists
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
        want, wids = direct.predict_interactions(files["test"][1], feats)
        got, ids = ranker.interactions(FeatureManager.readInput(files["test"][0]), FeatureManager.readInput(files["bg"][0]), features=feats)
        assert ids == wids and got.shape == want.shape and np.array_equal(u64(got), u64(want))
        again, _ = ranker.interactions(FeatureManager.readInput(files["test"][0]), None, features=feats)        # the covers of the call before
        assert np.array_equal(u64(again), u64(want))
    assert CR.same_f64(want, IR.interactions(trees, w, CR.covers_np(trees, files["bg"][1]), files["test"][1], [7, 2, 30])) is None
    monkeypatch.setattr(Ranker, "EVAL_ROW_BYTES", 64)                      # chunks of one list, their matrices document by document
    small, _ = ranker.interactions(FeatureManager.readInput(files["test"][0]), None, features=[7, 2, 30])
    assert np.array_equal(u64(small), u64(want))
    monkeypatch.undo()
    fpath = str(tmp_path / "features.txt")
    with open(fpath, "w") as f:
        f.write("7\n2\n30\n")
    lines = pairs_restated([7, 2, 30], want)
    assert len(lines) == 6 and lines[-1].split("\t")[2:] == ["0.0", "0.0"] and "30" in lines[-1].split("\t")[:2]       # a feature the model does not have
    phi, _ = direct.predict_shap(files["test"][1], [7, 2, 30])
    for k, eval_bytes in enumerate((None, 64)):                            # the file in one chunk, and in chunks of one list
        if eval_bytes:
            monkeypatch.setattr(Ranker, "EVAL_ROW_BYTES", eval_bytes)
        pairs, out, summ = (str(tmp_path / ("%s%d.tsv" % (nm, k))) for nm in ("pairs", "contribs", "summary"))
        assert CL.main(["-load", mpath, "-background", files["bg"][0], "-test", files["test"][0], "-feature", fpath, "-interactions", pairs,
                        "-out", out, "-summary", summ]) == 0
        assert open(pairs).read().splitlines() == lines
        rows_out = open(out).read().splitlines()                           # -interactions implies -exact: -out holds the SHAP values
        assert len(rows_out) == 26 and rows_out[7].split("\t")[3:] == ["%s:%s" % (nm, java_double_str(float(v))) for nm, v in zip(
            ["7", "2", "30", "rest", "bias"], phi[7])]
        assert len(open(summ).read().splitlines()) == 3
    fresh = RankerFactory().loadRankerFromString(text)                     # no covers yet: refused even with nothing to explain
    with pytest.raises(N.RankLibError, match="rl_model_predict_interactions: no rl_model_cover call has been made on this model"):
        fresh.interactions([], None)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    trees, w, _ = model("count_37")
    m = N.Model(TM.model_text(trees, w))
    lib = N.lib()
    rows, out = np.zeros((4, WIDTH), np.float32), np.zeros((4, 5, 5))
    cols, neg, twice = np.array([1, 2, 3], np.int32), np.array([1, -2, 3], np.int32), np.array([1, 2, 3, 2], np.int32)

    def err(rc_want, rc, text):
        assert rc == rc_want and lib.rl_last_error().decode() == text, (rc, lib.rl_last_error().decode(), text)
    X, O, cp = rows.ctypes.data, out.ctypes.data, cols.ctypes.data
    who = "rl_model_predict_interactions: "
    err(-3, lib.rl_model_predict_interactions(m.h, X, 4, WIDTH, cp, 3, 0, O), who + "no rl_model_cover call has been made on this model")
    assert m.path() == N.MODEL_PATH_NONE
    m.cover(rows)
    for args, text in (((None, X, 4, WIDTH, cp, 3, 0, O), "null model"), ((m.h, None, 4, WIDTH, cp, 3, 0, O), "null X"),
                       ((m.h, X, 4, WIDTH, cp, 3, 0, None), "null output"), ((m.h, X, -1, WIDTH, cp, 3, 0, O), "n_docs must be >= 0"),
                       ((m.h, X, 4, 0, cp, 3, 0, O), "row_stride must be >= 1"), ((m.h, X, 4, WIDTH, None, -1, 0, O), "n_columns must be >= 0"),
                       ((m.h, X, 4, WIDTH, cp, 0, 0, O), "n_columns must be >= 1 with columns given"),
                       ((m.h, X, 4, WIDTH, neg.ctypes.data, 3, 0, O), "columns[1] = -2 is negative"),
                       ((m.h, X, 4, WIDTH, twice.ctypes.data, 4, 0, O), "columns[3] = 2 is listed twice"),
                       ((m.h, X, 4, WIDTH, cp, 3, -1, O), "scratch_bytes must be >= 0")):
        err(-1, lib.rl_model_predict_interactions(*args), who + text)
    err(-4, lib.rl_model_predict_interactions(m.h, X, 2 ** 31, WIDTH, cp, 3, 0, O), who + "more than 2^31 documents per call")
    many = np.arange(65535, dtype=np.int32)                                # 65 536 conditioned slots: refused before anything of that size is made
    err(-4, lib.rl_model_predict_interactions(m.h, X, 4, WIDTH, many.ctypes.data, 65535, 0, O), who + "65536 conditioned slots, more than 65535")
    assert m.path() == N.MODEL_PATH_COVER
    a = C.c_double(0)
    err(-1, lib.rl_debug_interact_times(None, C.byref(a)), "rl_debug_interact_times: null argument")
    err(-1, lib.rl_debug_interact_passes(None), "rl_debug_interact_passes: null argument")
    with pytest.raises(N.RankLibError, match="columns\\[1\\] = 5 is listed twice"):
        m.predict_interactions(rows, [5, 5])
    with pytest.raises(N.RankLibError, match="n_columns must be >= 1 with columns given"):
        m.predict_interactions(rows, [])
    empty = N.Model("<ensemble>\n</ensemble>\n")
    with pytest.raises(N.RankLibError, match="rl_model_predict_interactions: the model has no trees"):
        empty.predict_interactions(rows)
    got, ids = m.predict_interactions(rows[:0])                            # no rows: legal, nothing to do
    n_ = len(CR.model_features(trees)) + 2
    assert got.shape == (0, n_, n_) and m.path() == N.MODEL_PATH_COVER
    got, ids = m.predict_interactions(rows)
    assert m.path() == N.MODEL_PATH_INTERACT == 8 and min(N.interact_times()) >= 0.0 and N.interact_passes() == 1


def test_random_forests_and_linear_models_are_refused():
    trees, w, _ = model("count_37")
    body = TM.model_text(trees[:9], w[:9])
    forest = RankerFactory().loadRankerFromString("## Random Forests\n## No. of bags = 1\n\n" + body.split("\n\n", 1)[1])
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Random Forests model has no trees of one ensemble: "
                                             "a forest is several ensembles averaged"):
        forest.interactions([], [])
    lin = RankerFactory().loadRankerFromString("## Coordinate Ascent\n## Restart = 5\n2:0.5 4:-0.25 6:0.125")
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        lin.interactions([], [])
