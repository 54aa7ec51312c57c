"""Per-document feature contributions on the GPU (rl_model_cover / rl_model_predict_contribs: k_model_cover and k_model_contribs,
rl_contrib.inc) against tests/contrib_restatement.py, the definitions of include/rlhip.h in plain Python.  Everything is
compared as bit patterns; no tolerance anywhere (where the reference value is NaN the kernel's is NaN: contrib_restatement.same_f64)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import contrib_restatement as CR
import list_cases as LC
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import LambdaMART, MART, Ranker, RankerFactory, java_double_str, java_float_str

pytestmark = pytest.mark.gpu

L, S = TM.L, TM.S
BG_COUNTS = (0, 1, 63, 64, 65, 257, 5000)        # both sides of a block's 256-row tile, and several blocks (20 of one row tile each)
STRIDE_ROWS = 140000                             # more than k_model_cover's 512 blocks x 256 rows: blocks that take a second row tile before they flush
ROW_COUNTS = (1, 63, 64, 65, 257)                # both sides of a block of 64 documents, and of one of 256
WIDTH = 13


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
          "stump": lambda: CR.hand_stump()[:2]}
COVER_MODELS = ["count_37", "nodes_81", "single_leaves", "nan_leaf", "chain_left", "chain_right", "stump"]


@functools.lru_cache(maxsize=None)
def background():
    rows = CR.grid_rows(np.random.default_rng(41), BG_COUNTS[-1], WIDTH)
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
    trees = model(name)[0]
    cov = CR.covers_np(trees, background()[:n_bg])
    return cov, CR.node_values(trees, cov)


def assert_cover(m, trees, cov, val, what):
    for t in range(len(trees)):
        gc, gv = m.cover_of(t)
        assert gc.dtype == np.uint64 and np.array_equal(gc, cov[t]), (what, t, gc, cov[t])
        assert CR.same_f64(gv, val[t]) is None, (what, t, CR.same_f64(gv, val[t]))


# ---- 1. covers, 2. values -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COVER_MODELS)
def test_covers_and_values_equal_the_restatement(name):
    trees, w, m = model(name)
    for n in BG_COUNTS:
        cov, val = reference(name, n)
        m.cover(background()[:n])
        assert m.path() == N.MODEL_PATH_COVER and m.cover_rows() == n
        assert all(int(c[0]) == n for c in cov)
        assert_cover(m, trees, cov, val, (name, n))


def test_blocks_that_stride_over_several_row_tiles_before_they_flush():
    """k_model_cover launches at most 512 blocks of 256 rows: above 131 072 rows a block walks a second row tile into the same LDS
    counters and flushes once.  35 blocks of the 512 take two tiles here, one of them a partial tile; covers, values and a contribution
    call on those values against the restatement."""
    trees, w, m = model("count_37")
    assert 512 * 256 < STRIDE_ROWS < 2 * 512 * 256 and (STRIDE_ROWS - 512 * 256) % 256
    bg = CR.grid_rows(np.random.default_rng(43), STRIDE_ROWS, WIDTH)
    cov = CR.covers_np(trees, bg)
    val = CR.node_values(trees, cov)
    m.cover(bg)
    assert m.cover_rows() == STRIDE_ROWS and all(int(c[0]) == STRIDE_ROWS for c in cov)
    assert_cover(m, trees, cov, val, "stride")
    m.cover(bg[:70000])
    m.cover(bg[70000:], accumulate=True)                     # neither call strides: the same counts
    assert_cover(m, trees, cov, val, "two calls")
    rows = doc_rows()[:65]
    got, ids = m.predict_contribs(rows)
    assert CR.same_f64(got, CR.contribs(trees, w, val, rows, ids)) is None


def test_covers_of_two_calls_add_up():
    trees, w, m = model("count_37")
    bg = background()
    m.cover(bg[:100])
    m.cover(bg[100:257], accumulate=True)
    assert m.cover_rows() == 257
    assert_cover(m, trees, *reference("count_37", 257), "100 + 157")
    m.cover(bg[:0], accumulate=True)                         # no rows: with accumulate the counts stay
    assert m.cover_rows() == 257
    assert_cover(m, trees, *reference("count_37", 257), "+ 0")
    m.cover(bg[:64])                                         # without it they are replaced
    assert m.cover_rows() == 64
    assert_cover(m, trees, *reference("count_37", 64), "replaced")


def test_a_model_column_at_or_beyond_row_stride_reads_zero():
    trees, w, m = model("count_37")
    assert max(CR.model_features(trees)) >= 6
    narrow = np.ascontiguousarray(background()[:257, :6])
    cov = CR.covers_np(trees, narrow)
    assert any(not np.array_equal(a, b) for a, b in zip(cov, reference("count_37", 257)[0]))
    m.cover(narrow)
    assert_cover(m, trees, cov, CR.node_values(trees, cov), "narrow")


def test_the_empty_node_rule_with_a_background_on_one_side_of_the_root():
    rng = np.random.default_rng(8)
    g = TM.Gen(rng)
    trees = [TM.flatten(S(1, 0.0, L(0.5), S(2, 0.25, S(3, -0.5, L(1.0), L(-2.0)), L(4.0))))]
    trees += [TM.flatten(S(1, 0.0, S(4, 0.5, L(0.1), L(0.7)), S(5, 0.0, L(2.0), L(9.0)))), TM.random_tree(g, 9)]
    w = np.array([1.0, 0.5, -0.25], np.float32)
    bg = background()[:300].copy()
    bg[:, 1] = -np.abs(np.nan_to_num(bg[:, 1], nan=1.0, posinf=1.0, neginf=-1.0)) - 0.0625          # all left of a root that splits feature 1 at 0.0
    cov = CR.covers_np(trees, bg)
    assert cov[0].tolist()[:2] == [300, 300] and not cov[0][2:].any() and not cov[1][4:].any() and cov[1][1] == 300
    val = CR.node_values(trees, cov)
    assert val[0][2] == (((1.0 + -2.0) / 2) + 4.0) / 2 and val[0][0] == 0.5          # plain averages below; the root is its left child
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    assert_cover(m, trees, cov, val, "one side")
    rows = doc_rows()[:65]
    got, ids = m.predict_contribs(rows)
    want = CR.contribs(trees, w, val, rows, ids)
    assert CR.same_f64(got, want) is None, CR.same_f64(got, want)


# ---- 3. contributions ----------------------------------------------------------------------------------------------------------------------
def column_choices(trees):
    feats = CR.model_features(trees)
    out = {"none": None, "one": [feats[0] if feats else 1], "unused": [max(feats, default=0) + 7] + feats[:2]}
    if len(feats) >= 2:
        out["subset"] = feats[1::2]
        out["descending"] = sorted(feats, reverse=True)
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_contributions_equal_the_restatement(name):
    trees, w, m = model(name)
    cov, val = reference(name, 257)
    m.cover(background()[:257])
    rows = doc_rows()
    paths = CR.paths(trees, rows)
    feats = CR.model_features(trees)
    for what, cols in column_choices(trees).items():
        ids = feats if cols is None else cols
        want = CR.contribs(trees, w, val, rows, ids, paths)
        for n in ROW_COUNTS:
            got, gids = m.predict_contribs(rows[:n], cols)
            assert m.path() == N.MODEL_PATH_CONTRIBS and N.contrib_passes() == 1
            assert gids == ids and got.shape == (n, len(ids) + 2) and got.dtype == np.float64
            assert CR.same_f64(got, want[:n]) is None, (name, what, n, CR.same_f64(got, want[:n]))
        if cols is None:
            assert not u64(want[:, len(ids)]).any()                        # every feature has its slot: rest is +0.0, the bits
        if what == "unused":
            assert not u64(want[:, 0]).any()                               # a feature the model never splits on: +0.0
        if what == "subset":
            assert want[:, len(ids)].any()                                 # the other features' steps are in rest
    leaf = CR.leaf_sums(trees, w, rows, paths)                            # the walk of its own that the command line measures against
    for n in ROW_COUNTS:
        assert CR.same_f64(m.leaf_sums(rows[:n]), leaf[:n]) is None, (name, n, CR.same_f64(m.leaf_sums(rows[:n]), leaf[:n]))
    if name in ("nan_leaf", "accum_specials"):
        want = CR.contribs(trees, w, val, rows, feats, paths)
        assert not np.isfinite(want).all() and np.isfinite(want).any()
    if name == "single_leaves":
        assert len(set(w.tolist())) > 1 and feats == []


def test_the_hand_derived_stump():
    trees, w, bg = CR.hand_stump()
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    gc, gv = m.cover_of(0)
    assert gc.tolist() == [4, 3, 1] and u64(gv).tolist() == u64([0.0, -1.0, 3.0]).tolist()
    rows = np.array([[0, -3.0], [0, 0.0], [0, 7.0], [0, np.nan]], np.float32)
    got, ids = m.predict_contribs(rows, [1])
    assert ids == [1] and u64(got).tolist() == u64([[-0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 0.0, 0.0]]).tolist()


def test_a_requested_column_at_or_beyond_row_stride_that_the_model_splits_on():
    """the background has the column, the rows do not: every row reads 0 there, and the steps at its splits still move the value"""
    trees, w, m = model("count_37")
    cov, val = reference("count_37", 257)
    m.cover(background()[:257])
    narrow = np.ascontiguousarray(doc_rows()[:, :6])
    feats = CR.model_features(trees)
    cols = [f for f in feats if f >= 6][:2] + [2]
    assert len(cols) == 3
    want = CR.contribs(trees, w, val, narrow, cols)
    assert want[:, 0].any() and not np.array_equal(u64(want), u64(CR.contribs(trees, w, val, doc_rows(), cols)))
    got, _ = m.predict_contribs(narrow, cols)
    assert CR.same_f64(got, want) is None, CR.same_f64(got, want)


# ---- 4. column passes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide():
    """200 trees of 5 nodes that between them split on 400 distinct features, ids 1 .. 400, over 70 rows.  The issue's 300 features are
    302 slots, and blocks of 64 documents hold 312 slots beside a tile of such trees (contrib_slot_limit(5, 64)): 302 would fit one pass,
    so it is 400 features here, 402 slots, two passes."""
    rng = np.random.default_rng(9)
    order = rng.permutation(400) + 1
    th = lambda: np.float32(rng.choice(TM.GRID))                       # noqa: E731
    out = lambda: np.float32(rng.standard_normal())                    # noqa: E731
    trees = [TM.flatten(S(int(order[2 * i]), th(), L(out()), S(int(order[2 * i + 1]), th(), L(out()), L(out())))) for i in range(200)]
    w = TM.WEIGHTS[rng.integers(0, len(TM.WEIGHTS), 200)]
    bg = CR.grid_rows(rng, 90, 401)
    rows = CR.grid_rows(rng, 70, 401)
    cov = CR.covers_np(trees, bg)
    val = CR.node_values(trees, cov)
    want = CR.contribs(trees, w, val, rows, list(range(1, 401)))
    m = N.Model(TM.model_text(trees, w))
    m.cover(bg)
    return trees, w, rows, val, want, m


def test_more_slots_than_the_lds_holds_take_several_column_passes():
    trees, w, rows, val, want, m = wide()
    assert CR.slot_limit(5, 64) == 312 and 300 + 2 <= 312 < 400 + 2
    got, ids = m.predict_contribs(rows)
    assert N.contrib_passes() == 2 and ids == list(range(1, 401))
    assert CR.same_f64(got, want) is None, CR.same_f64(got, want)
    pick = sorted(np.random.default_rng(3).choice(400, 20, replace=False) + 1)
    one, _ = m.predict_contribs(rows, pick)
    assert N.contrib_passes() == 1                                         # 22 slots: one pass, blocks of 256
    assert np.array_equal(u64(one[:, :20]), u64(got[:, [p - 1 for p in pick]])) and np.array_equal(u64(one[:, 21]), u64(got[:, 401]))
    mid = list(range(400, 250, -1))                                        # 152 slots: one pass, blocks of 128
    assert CR.slot_limit(5, 256) < 152 <= CR.slot_limit(5, 128)
    two, _ = m.predict_contribs(rows, mid)
    assert N.contrib_passes() == 1
    assert np.array_equal(u64(two[:, :150]), u64(got[:, [p - 1 for p in mid]]))
    assert CR.same_f64(two, CR.contribs(trees, w, val, rows, mid)) is None


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------------------------
def test_row_chunks_change_no_bit():
    trees, w, m = model("count_37")
    m.cover(background()[:257])
    rows = doc_rows()
    feats = CR.model_features(trees)
    whole, _ = m.predict_contribs(rows)
    per_row = WIDTH * 4 + 8 * (len(feats) + 2)
    three, _ = m.predict_contribs(rows, scratch_bytes=per_row * 100)      # 100 + 100 + 57 rows
    assert np.array_equal(u64(three), u64(whole))
    each, _ = m.predict_contribs(rows[:5], scratch_bytes=1)                # a chunk holds at least one row
    assert np.array_equal(u64(each), u64(whole[:5]))
    assert CR.same_f64(whole, CR.contribs(trees, w, reference("count_37", 257)[1], rows, feats)) is None


def test_covers_and_contributions_in_chunks_of_whole_lists_equal_the_one_chunk(monkeypatch):
    """list_cases under its small limit: countCover and both kinds of contributions go in five calls each (one list alone over the
    limit, an empty list inside a chunk) and give the bits of the one call"""
    samples, bg = LC.lists(), LC.lists(seed=10)
    ranker = RankerFactory().loadRankerFromString(LC.model_text())
    calls = {"cover": [], "predict_contribs": [], "predict_shap": []}
    for nm in calls:
        monkeypatch.setattr(ranker._model, nm, lambda rows, *a, _f=getattr(ranker._model, nm), _c=calls[nm], **kw: (_c.append(len(rows)), _f(rows, *a, **kw))[1])

    def run():
        for c in calls.values():
            del c[:]
        ranker.countCover(bg)
        return ranker._model.cover_rows(), ranker.contributions(samples, None, exact=False), ranker.contributions(samples, None, exact=True)
    n_one, (approx_one, ids), (exact_one, _) = run()
    assert calls == {"cover": [0, sum(LC.SIZES)], "predict_contribs": [sum(LC.SIZES)], "predict_shap": [sum(LC.SIZES)]}      # (the reset, then the file)
    monkeypatch.setattr(Ranker, "EVAL_ROW_BYTES", LC.SMALL_LIMIT)
    n_many, (approx_many, ids_many), (exact_many, _) = run()
    assert calls == {"cover": [0] + LC.CHUNK_ROWS, "predict_contribs": LC.CHUNK_ROWS, "predict_shap": LC.CHUNK_ROWS}
    assert n_many == n_one == sum(LC.SIZES) and ids_many == ids
    assert approx_one.shape == exact_one.shape == (sum(LC.SIZES), len(ids) + 2)
    assert np.array_equal(u64(approx_many), u64(approx_one)) and np.array_equal(u64(exact_many), u64(exact_one))
    assert not np.array_equal(u64(approx_one), u64(exact_one)) and approx_one[:, :len(ids)].any()


# ---- 6. against the public path ------------------------------------------------------------------------------------------------------------
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
        rows = rng.choice(TM.GRID, (int(qoff[-1]), WIDTH)).astype(np.float32)
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
        want, wids = direct.predict_contribs(files["test"][1], feats)
        got, ids = ranker.contributions(FeatureManager.readInput(files["test"][0]), FeatureManager.readInput(files["bg"][0]), features=feats)
        assert ids == wids and np.array_equal(u64(got), u64(want))
    assert ranker._model.cover_rows() == 150
    fpath = str(tmp_path / "features.txt")
    with open(fpath, "w") as f:
        f.write("7\n2\n30\n")
    out, summ = str(tmp_path / "contribs.tsv"), str(tmp_path / "summary.tsv")
    assert CL.main(["-load", mpath, "-background", files["bg"][0], "-test", files["test"][0], "-feature", fpath, "-out", out, "-summary", summ]) == 0
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
    leaf = direct.leaf_sums(files["test"][1])                              # what the command line measures the slots' sum against
    assert np.array_equal(u64(leaf), u64(CR.leaf_sums(trees, w, files["test"][1])))
    fresh = RankerFactory().loadRankerFromString(text)                     # no covers yet: refused even with nothing to explain
    with pytest.raises(N.RankLibError, match="no rl_model_cover call has been made on this model"):
        fresh.contributions([], None)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    trees, w, _ = model("count_37")
    m = N.Model(TM.model_text(trees, w))
    lib = N.lib()
    rows, out = np.zeros((4, WIDTH), np.float32), np.zeros((4, 5))
    cols, neg, twice = np.array([1, 2, 3], np.int32), np.array([1, -2, 3], np.int32), np.array([1, 2, 3, 2], np.int32)
    cnt, val, n = np.zeros(400, np.uint64), np.zeros(400), C.c_int32(-7)

    def err(rc_want, rc, text):
        assert rc == rc_want and lib.rl_last_error().decode() == text, (rc, lib.rl_last_error().decode(), text)
    X, O, cp = rows.ctypes.data, out.ctypes.data, cols.ctypes.data
    who = "rl_model_predict_contribs: "
    err(-3, lib.rl_model_predict_contribs(m.h, X, 4, WIDTH, cp, 3, 0, O), who + "no rl_model_cover call has been made on this model")
    err(-3, lib.rl_model_get_cover(m.h, 0, cnt.ctypes.data, val.ctypes.data, 400, C.byref(n)),
        "rl_model_get_cover: no rl_model_cover call has been made on this model")
    assert n.value == len(trees[0]["feature"]) and m.cover_rows() == 0
    for args, text in (((None, X, 4, WIDTH, 0), "null model"), ((m.h, None, 4, WIDTH, 0), "null X"), ((m.h, X, -1, WIDTH, 0), "n_docs must be >= 0"),
                       ((m.h, X, 4, 0, 0), "row_stride must be >= 1")):
        err(-1, lib.rl_model_cover(*args), "rl_model_cover: " + text)
    assert m.cover_rows() == 0
    m.cover(rows)
    for args, text in (((None, X, 4, WIDTH, cp, 3, 0, O), "null model"), ((m.h, None, 4, WIDTH, cp, 3, 0, O), "null X"),
                       ((m.h, X, 4, WIDTH, cp, 3, 0, None), "null output"), ((m.h, X, -1, WIDTH, cp, 3, 0, O), "n_docs must be >= 0"),
                       ((m.h, X, 4, 0, cp, 3, 0, O), "row_stride must be >= 1"), ((m.h, X, 4, WIDTH, None, -1, 0, O), "n_columns must be >= 0"),
                       ((m.h, X, 4, WIDTH, cp, 0, 0, O), "n_columns must be >= 1 with columns given"),
                       ((m.h, X, 4, WIDTH, neg.ctypes.data, 3, 0, O), "columns[1] = -2 is negative"),
                       ((m.h, X, 4, WIDTH, twice.ctypes.data, 4, 0, O), "columns[3] = 2 is listed twice"),
                       ((m.h, X, 4, WIDTH, cp, 3, -1, O), "scratch_bytes must be >= 0")):
        err(-1, lib.rl_model_predict_contribs(*args), who + text)
    nn = len(trees[0]["feature"])
    err(-1, lib.rl_model_get_cover(m.h, -1, None, None, 400, None), "rl_model_get_cover: tree = -1 is outside [0, 37)")
    err(-1, lib.rl_model_get_cover(m.h, 37, None, None, 400, None), "rl_model_get_cover: tree = 37 is outside [0, 37)")
    n.value = -7
    err(-1, lib.rl_model_get_cover(m.h, 0, cnt.ctypes.data, val.ctypes.data, nn - 1, C.byref(n)),
        "rl_model_get_cover: cap = %d is below the tree's %d nodes" % (nn - 1, nn))
    assert n.value == nn
    with pytest.raises(N.RankLibError, match="columns\\[1\\] = 5 is listed twice"):
        m.predict_contribs(rows, [5, 5])
    with pytest.raises(N.RankLibError, match="n_columns must be >= 1 with columns given"):
        m.predict_contribs(rows, [])
    empty = N.Model("<ensemble>\n</ensemble>\n")
    for call, name in ((lambda: empty.cover(rows), "rl_model_cover"), (lambda: empty.predict_contribs(rows), "rl_model_predict_contribs"),
                       (lambda: empty.cover_of(0), "rl_model_get_cover"), (lambda: empty.leaf_sums(rows), "rl_model_predict_leaf_sums")):
        with pytest.raises(N.RankLibError, match=name + ": the model has no trees"):
            call()
    sums = np.zeros(4)
    for args, text in (((m.h, None, 4, WIDTH, sums.ctypes.data), "null X"), ((m.h, X, 4, WIDTH, None), "null output"),
                       ((m.h, X, -1, WIDTH, sums.ctypes.data), "n_docs must be >= 0"), ((m.h, X, 4, 0, sums.ctypes.data), "row_stride must be >= 1")):
        err(-1, lib.rl_model_predict_leaf_sums(*args), "rl_model_predict_leaf_sums: " + text)
    assert m.leaf_sums(rows[:0]).shape == (0,)
    got, ids = m.predict_contribs(rows[:0])                                # no rows: legal, nothing to do
    assert got.shape == (0, len(CR.model_features(trees)) + 2)
    cover_ms, walk_ms = N.contrib_times()
    assert cover_ms >= 0.0 and walk_ms >= 0.0


def test_random_forests_and_linear_models_are_refused():
    trees, w, _ = model("count_37")
    body = TM.model_text(trees[:9], w[:9])
    forest = RankerFactory().loadRankerFromString("## Random Forests\n## No. of bags = 1\n\n" + body.split("\n\n", 1)[1])
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Random Forests model has no trees of one ensemble: "
                                             "a forest is several ensembles averaged"):
        forest.contributions([], [])
    lin = RankerFactory().loadRankerFromString("## Coordinate Ascent\n## Restart = 5\n2:0.5 4:-0.25 6:0.125")
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        lin.contributions([], [])
