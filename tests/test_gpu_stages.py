"""Staged evaluation on the GPU (rl_model_predict_stages / rl_model_eval_stages: k_model_stage_scores and k_stage_eval, rl_stage.inc;
DESIGN.md 23) against tests/stages_restatement.py and against the public path that exists without it -- one truncated model per stage
through predict_rows and eval_lists.  Everything is compared as bit patterns; no tolerance anywhere."""
import functools

import numpy as np
import pytest

import eval_lists_restatement as ER
import list_cases as LC
import stages_restatement as SR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import evaluator, stages
from ranklib_amd import metric as M
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import Ranker, RankerFactory, java_float_str

pytestmark = pytest.mark.gpu

L, S = TM.L, TM.S
LENS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600]       # both sides of kEvTiny and kEvWave, several blocks of tiny lists' worth
NT = 37
WHOLE = 1000                                                    # a k past every list: the whole list (k = 0 is that too, but plain RR scores 0 there)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def grid_rows(rng, n, width=13):
    rows = rng.choice(TM.GRID, (n, width)).astype(np.float32)
    rows[:, 0] = 0.0
    return rows


@functools.lru_cache(maxsize=None)
def main_data():
    """37 random trees of 2 - 8 leaves with weight 0.1 over rows from the 65-value grid (so documents share leaves and tie), labels
    0 - 4; the restatement's scores and rankings of every stage, made once"""
    rng = np.random.default_rng(5)
    g = TM.Gen(rng)
    trees = [TM.random_tree(g, int(rng.integers(2, 9))) for _ in range(NT)]
    w = np.full(NT, 0.1, np.float32)
    qoff = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    rows = grid_rows(rng, int(qoff[-1]))
    lab = rng.integers(0, 5, int(qoff[-1])).astype(np.float32)
    allst = list(range(1, NT + 1))
    sc = SR.stage_scores(trees, w, rows, allst)
    pos = SR.stage_positions(sc, qoff)
    for a in (w, qoff, rows, lab, sc, pos):
        a.setflags(write=False)
    return trees, w, rows, lab, qoff, sc, pos


@functools.lru_cache(maxsize=None)
def main_model():
    trees, w = main_data()[:2]
    return N.Model(TM.model_text(trees, w))


# ---- 1. the stage scores ---------------------------------------------------------------------------------------------------------------
def _single_leaves():
    rng = np.random.default_rng(31)
    g = TM.Gen(rng)
    trees = [TM.single_leaf(g) for _ in range(5)]
    return TM.Case(trees, np.array([0.1, 1.0, -0.25, 3.0, 0.5], np.float32), grid_rows(rng, 70), True)


SCORE_CASES = {"count_37": lambda: TM.case("count_37")[0], "single_leaves": _single_leaves, "accum_specials": lambda: TM.case("accum_specials")[0],
               "nan_leaf": lambda: TM.case("nan_leaf")[0], "nodes_81": lambda: TM.case("nodes_81")[0]}


@pytest.mark.parametrize("name", sorted(SCORE_CASES))
def test_predict_stages_equals_every_prefix(name):
    c = SCORE_CASES[name]()
    T = len(c.trees)
    want = SR.stage_scores(c.trees, c.weights, c.rows, list(range(1, T + 1)))
    m = N.Model(TM.model_text(c.trees, c.weights))
    for st in ([1], [T], list(range(1, T + 1)), sorted(set(range(3, T + 1, 3)) | {T})):
        got = m.predict_stages(c.rows, st)
        assert got.shape == (len(st), len(c.rows))
        assert TM.same_scores(got, want[np.array(st) - 1]) is None, (name, st[:4], TM.same_scores(got, want[np.array(st) - 1]))
    last = m.predict_stages(c.rows, [T])[0]
    assert TM.same_scores(last, m.predict_rows(c.rows)) is None
    assert m.path() == (N.MODEL_PATH_TILED if c.tiled else N.MODEL_PATH_GENERIC)      # the last stage equals both scoring kernels' bits
    if name == "accum_specials":
        assert np.isinf(want).any() and np.isnan(want).any()


# ---- 2. ranking and scoring every stage ------------------------------------------------------------------------------------------------
def test_the_restatement_itself_tells_the_stages_apart():
    """a kernel that ignored the stage would have to fail test 2: under NDCG@10 at least 90 % of consecutive stages differ in some list,
    and every list of 63 documents or more takes at least 20 distinct values"""
    trees, w, rows, lab, qoff, sc, pos = main_data()
    v, nan, _ = SR.eval_stages(trees, w, rows, lab, qoff, "NDCG", 10, list(range(1, NT + 1)), scores=sc, pos=pos)
    assert not nan.any()
    differ = sum(1 for s in range(NT - 1) if (bits(v[s]) != bits(v[s + 1])).any())
    assert differ >= 0.9 * (NT - 1), differ
    for q, n in enumerate(LENS):
        if n >= 63:
            assert len(set(bits(v[:, q]).tolist())) >= 20, (n, len(set(bits(v[:, q]).tolist())))


@pytest.mark.parametrize("metric", ER.METRICS)
def test_eval_stages_equals_the_restatement(metric):
    trees, w, rows, lab, qoff, sc, pos = main_data()
    allst = list(range(1, NT + 1))
    for k in (1, 3, 10, WHOLE):
        want, wnan, wideal = SR.eval_stages(trees, w, rows, lab, qoff, metric, k, allst, scores=sc, pos=pos)
        got, gnan, gideal = main_model().eval_stages(rows, lab, qoff, metric, k, allst)
        assert not gnan.any() and not wnan.any()
        assert SR.same_bits(got, want) is None, (metric, k, SR.same_bits(got, want))
        assert np.array_equal(bits(gideal), bits(wideal))


# ---- 3. the public path that exists without the feature --------------------------------------------------------------------------------
@pytest.mark.parametrize("metric, k", [("NDCG", 10), ("MAP", 0), ("ERR", 3)])
def test_a_stage_equals_the_truncated_model_through_predict_rows_and_eval_lists(metric, k):
    trees, w, rows, lab, qoff, _, _ = main_data()
    st = [1, 2, 17, 36, 37]
    got, gnan, _ = main_model().eval_stages(rows, lab, qoff, metric, k, st)
    assert not gnan.any()
    for i, t in enumerate(st):
        sc = N.Model(TM.model_text(trees[:t], w[:t])).predict_rows(rows).astype(np.float64)
        want, _, _ = N.eval_lists(sc, lab, qoff, metric, k)
        assert np.array_equal(bits(got[i]), bits(want)), (metric, t)


# ---- 4. chunk edges --------------------------------------------------------------------------------------------------------------------
def test_chunks_of_1_2_and_5_stages_equal_the_single_chunk():
    trees, w, rows, lab, qoff, _, _ = main_data()
    st = list(range(3, 36, 3))
    assert len(st) == 11
    one, onan, _ = main_model().eval_stages(rows, lab, qoff, "NDCG", 10, st)
    for per in (1, 2, 5):                                   # 4 bytes per document and stage: 11, 6 and 3 chunks, the last one short
        got, gnan, _ = main_model().eval_stages(rows, lab, qoff, "NDCG", 10, st, scratch_bytes=per * len(rows) * 4 + 3)
        assert np.array_equal(bits(got), bits(one)) and np.array_equal(gnan, onan), per
    assert np.array_equal(bits(main_model().eval_stages(rows, lab, qoff, "NDCG", 10, st, scratch_bytes=1)[0]), bits(one))      # a chunk holds at least one stage


@pytest.mark.parametrize("name", ["count_97", "nodes_81"])
def test_chunks_across_the_tiles_of_the_tiled_walk(name):
    """97 trees are four tiles of the tiled kernel, whose chunks carry the sum at tile boundaries and walk the trees behind the last
    boundary again: chunk ends before, at and after trees 32, 64 and 96.  nodes_81: the same chunks through the per-document kernel."""
    c = TM.case(name)[0]
    T = len(c.trees)
    rng = np.random.default_rng(97)
    qoff = np.array([0, 16, 80, len(c.rows)], np.int32)
    lab = rng.integers(0, 5, len(c.rows)).astype(np.float32)
    m = N.Model(TM.model_text(c.trees, c.weights))
    for st in (sorted(set(range(3, T + 1, 3)) | {31, 32, 33, 64, T}), [min(40, T)], sorted({32, min(64, T)})):
        st = [t for t in st if t <= T]
        want, wnan, _ = SR.eval_stages(c.trees, c.weights, c.rows, lab, qoff, "NDCG", 10, st)
        for per in (0, 1, 2, 5):
            got, gnan, _ = m.eval_stages(c.rows, lab, qoff, "NDCG", 10, st, scratch_bytes=per * len(c.rows) * 4)
            assert np.array_equal(gnan, wnan) and SR.same_bits(got, want) is None, (name, per, st[:5], SR.same_bits(got, want))
    assert m.path() == (N.MODEL_PATH_TILED if c.tiled else N.MODEL_PATH_GENERIC)


# ---- 5. the long classes ---------------------------------------------------------------------------------------------------------------
def test_lists_around_the_lds_class():
    rng = np.random.default_rng(55)
    g = TM.Gen(rng)
    trees = [TM.random_tree(g, int(rng.integers(3, 9))) for _ in range(5)]
    w = np.array([0.1, 1.0, 0.5, -0.25, 0.1], np.float32)
    lens = [6143, 6144, 6145]
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = grid_rows(rng, int(qoff[-1]))
    lab = rng.integers(0, 5, int(qoff[-1])).astype(np.float32)
    st = [1, 3, 5]
    sc = SR.stage_scores(trees, w, rows, st)
    pos = SR.stage_positions(sc, qoff)
    m = N.Model(TM.model_text(trees, w))
    for metric, k in (("NDCG", 10), ("BEST", 3), ("MAP", 0)):
        want, wnan, _ = SR.eval_stages(trees, w, rows, lab, qoff, metric, k, st, scores=sc, pos=pos)
        got, gnan, _ = m.eval_stages(rows, lab, qoff, metric, k, st)
        assert not gnan.any() and SR.same_bits(got, want) is None, (metric, SR.same_bits(got, want))
    # the scratch of a stage is 16 bytes per document here: two chunks
    got2, _, _ = m.eval_stages(rows, lab, qoff, "MAP", 0, st, scratch_bytes=2 * 16 * len(rows))
    assert np.array_equal(bits(got2), bits(got))


# ---- 6. whole lists that tie -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [(-0.0, 0.0, 0.5), (-0.0, 0.0, 0.5, -float(TM.F32_MIN))])
def test_whole_lists_that_tie(outputs):
    rng = np.random.default_rng(66)
    g = TM.Gen(rng, outputs=np.array(outputs, np.float32))
    trees = [TM.random_tree(g, int(rng.integers(2, 6))) for _ in range(8)]
    # scores that reach +-Infinity through Float.MAX_VALUE outputs (and NaN where both meet)
    trees += [TM.flatten(S(1, 0.0, L(TM.F32_MAX), L(0.5))), TM.flatten(S(1, 0.0, L(TM.F32_MAX), L(0.0))),
              TM.flatten(S(2, -1.5, L(-TM.F32_MAX), L(-0.0))), TM.flatten(S(2, -1.5, L(-TM.F32_MAX), L(0.5)))]
    w = np.concatenate([np.full(8, 0.1, np.float32), np.ones(4, np.float32)])
    lens = [1, 7, 16, 40, 64, 130, 300]
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = np.concatenate([grid_rows(rng, 3)[rng.integers(0, 3, n)] if i % 2 == 0 else grid_rows(rng, n)
                           for i, n in enumerate(lens)])    # every other list repeats three rows: whole runs of equal scores
    lab = rng.integers(0, 5, len(rows)).astype(np.float32)
    st = list(range(1, len(trees) + 1))
    sc = SR.stage_scores(trees, w, rows, st)
    assert np.isposinf(sc).any() and np.isneginf(sc).any()
    if len(outputs) == 4:
        assert (sc.view(np.uint32) == 0x80000000).any() and (sc.view(np.uint32) == 0).any()      # -0.0 beside +0.0
    m = N.Model(TM.model_text(trees, w))
    for metric, k in (("NDCG", 10), ("P", 3), ("MAP", 0)):
        want, wnan, _ = SR.eval_stages(trees, w, rows, lab, qoff, metric, k, st, scores=sc)
        got, gnan, _ = m.eval_stages(rows, lab, qoff, metric, k, st)
        assert np.array_equal(gnan, wnan) and SR.same_bits(got, want) is None, (metric, SR.same_bits(got, want))


# ---- 7. a NaN leaf ---------------------------------------------------------------------------------------------------------------------
def letor_text(rows, lab, qoff):
    out = []
    for q in range(len(qoff) - 1):
        for i in range(qoff[q], qoff[q + 1]):
            out.append("%d qid:q%d %s\n" % (int(lab[i]), q, " ".join("%d:%s" % (f, java_float_str(rows[i, f])) for f in range(1, rows.shape[1]))))
    return "".join(out)


def test_a_nan_leaf_from_tree_4_on(tmp_path):
    rng = np.random.default_rng(77)
    g = TM.Gen(rng)
    trees = [TM.random_tree(g, int(rng.integers(2, 9))) for _ in range(8)]
    trees[3] = TM.flatten(S(3, -1.9, L(np.nan), L(0.25)))   # two of the grid's 65 values go left
    w = np.full(8, 0.1, np.float32)
    lens = [5, 12, 3, 20, 40, 8, 16, 100, 2, 30]
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = grid_rows(rng, int(qoff[-1]))
    lab = rng.integers(0, 5, int(qoff[-1])).astype(np.float32)
    holds = np.array([(rows[qoff[q]:qoff[q + 1], 3] <= -1.9).any() for q in range(len(lens))])
    assert holds.any() and not holds.all()
    st = list(range(1, 9))
    text = TM.model_text(trees, w)
    m = N.Model(text)
    got, gnan, _ = m.eval_stages(rows, lab, qoff, "NDCG", 10, st)
    want, wnan, _ = SR.eval_stages(trees, w, rows, lab, qoff, "NDCG", 10, st)
    assert np.array_equal(gnan != 0, (np.array(st)[:, None] >= 4) & holds[None, :]) and np.array_equal(gnan, wnan)
    assert SR.same_bits(got, want) is None and not got[gnan != 0].any()
    # stagedScores fills the flagged cells with what the per-list host path gives for the truncated model
    path = str(tmp_path / "nan.txt")
    with open(path, "w") as f:
        f.write(letor_text(rows, lab, qoff))
    samples = FeatureManager.readInput(path)
    ranker = RankerFactory().loadRankerFromString(text)
    for scorer in (lambda: M.NDCGScorer(10), M.APScorer):
        staged = ranker.stagedScores(samples, scorer())
        assert staged.shape == (8, len(lens))
        for t in st:
            cut = ranker.truncated(t)
            assert cut._model.num_trees() == t and type(cut) is type(ranker)
            flat, _ = cut.evalLists(samples)
            per, _ = M.score_lists(scorer(), samples, flat)
            assert np.array_equal(bits(staged[t - 1]), bits(per)), t
    three = ranker.stagedScores(samples, M.NDCGScorer(10), stages=[2, 5, 8])
    assert np.array_equal(bits(three), bits(ranker.stagedScores(samples, M.NDCGScorer(10))[[1, 4, 7]]))


# ---- 8. external tables ----------------------------------------------------------------------------------------------------------------
def test_external_tables_and_the_first_list_of_a_key():
    trees, w, rows, lab, qoff, sc, pos = main_data()
    st = [5, 37]
    at = np.array(st) - 1
    qkey = np.array([0, 1, 2, 3, 4, 5, 5, 6, 7, 3, 8, 8], np.int32)       # lists of other lengths and labels share keys: the first decides
    given = np.full(len(LENS), np.nan)
    given[[2, 7, 10]] = [3.5, 100.0, 0.0]                   # entries beside NaN ones; list 11 shares key 8 with the given list 10
    got, gnan, gideal = main_model().eval_stages(rows, lab, qoff, "NDCG", 10, st, qkey=qkey, ideal_dcg=given)
    want, _, wideal = SR.eval_stages(trees, w, rows, lab, qoff, "NDCG", 10, st, qkey=qkey, ideal_dcg=given, scores=sc[at], pos=pos[at])
    assert SR.same_bits(got, want) is None and not gnan.any()
    _, _, lideal = N.eval_lists(sc[36].astype(np.float64), lab, qoff, "NDCG", 10, qkey=qkey, ideal_dcg=given)
    assert np.array_equal(bits(gideal), bits(wideal)) and np.array_equal(bits(gideal), bits(lideal))
    assert gideal[6] == gideal[5] and gideal[9] == gideal[3] and gideal[11] == 0.0 and gideal[2] == 3.5
    rdc = np.array([0, 1, 2, 30, 4, 5, 6, 7, 300, 9, 10, 11], np.int32)
    got, _, gideal = main_model().eval_stages(rows, lab, qoff, "MAP", 0, st, rel_doc_count=rdc)
    want, _, _ = SR.eval_stages(trees, w, rows, lab, qoff, "MAP", 0, st, rel_doc_count=rdc, scores=sc[at], pos=pos[at])
    assert SR.same_bits(got, want) is None and np.isnan(gideal).all() and not got[:, 0].any()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_has_its_status_and_message():
    lib = N.lib()
    trees, w, rows, lab, qoff, _, _ = main_data()
    m = main_model()
    st = np.array([1, 5, 37], np.int32)
    nl = len(LENS)
    out, nan = np.zeros((3, nl)), np.zeros((3, nl), np.uint8)
    base = dict(m=m.h, X=rows.ctypes.data, n=len(rows), stride=rows.shape[1], lab=lab.ctypes.data, qoff=qoff.ctypes.data, nl=nl, qkey=None,
                ideal=None, rdc=None, metric=0, k=10, err_max=16.0, st=st.ctypes.data, ns=3, scratch=0, out=out.ctypes.data, nan=nan.ctypes.data,
                oideal=None)

    def ev(**kw):
        a = dict(base, **kw)
        rc = lib.rl_model_eval_stages(a["m"], a["X"], a["n"], a["stride"], a["lab"], a["qoff"], a["nl"], a["qkey"], a["ideal"], a["rdc"],
                                      a["metric"], a["k"], a["err_max"], a["st"], a["ns"], a["scratch"], a["out"], a["nan"], a["oideal"])
        return rc, lib.rl_last_error().decode()

    assert ev()[0] == 0
    empty = N.Model("## LambdaMART\n\n<ensemble>\n</ensemble>\n")
    assert empty.num_trees() == 0
    bad = lambda a: np.array(a, np.int32)      # noqa: E731
    s0, s99, sdup, sdown = bad([0, 1, 2]), bad([1, 2, 38]), bad([1, 5, 5]), bad([1, 5, 4])
    q1, qgap = bad([1] + list(qoff[1:])), bad(list(qoff[:-1]) + [int(qoff[-1]) - 1])
    neg = lab.copy(); neg[7] = -1.0
    for kw, text in ((dict(m=None), "null model"), (dict(X=None), "null X"), (dict(st=None), "null stages"), (dict(out=None), "null output"),
                     (dict(nan=None), "null out_nan"), (dict(lab=None), "null argument"), (dict(qoff=None), "null argument"),
                     (dict(ns=0), "n_stages must be >= 1"), (dict(st=s0.ctypes.data), "stages[0] = 0 is outside [1, 37]"),
                     (dict(st=s99.ctypes.data), "stages[2] = 38 is outside [1, 37]"), (dict(st=sdup.ctypes.data), "stages must be strictly increasing (stages[2])"),
                     (dict(st=sdown.ctypes.data), "stages must be strictly increasing (stages[2])"), (dict(stride=0), "row_stride must be >= 1"),
                     (dict(scratch=-1), "scratch_bytes must be >= 0"), (dict(m=empty.h), "the model has no trees"),
                     (dict(metric=7), "unknown metric 7"), (dict(nl=0), "n_lists and n_docs must be >= 1"), (dict(qoff=q1.ctypes.data), "qoff must start at 0"),
                     (dict(qoff=qgap.ctypes.data), "qoff must end at n_docs"), (dict(lab=neg.ctypes.data), "Relevance label cannot be negative. System will now exit."),
                     (dict(metric=3, err_max=0.0), "err_max (ERRScorer.MAX) must be positive and finite")):
        rc, msg = ev(**kw)
        assert rc == -1 and msg == "rl_model_eval_stages: " + text, (kw, rc, msg)
    sco = np.zeros((3, len(rows)), np.float32)

    def pr(**kw):
        a = dict(dict(m=m.h, X=rows.ctypes.data, n=len(rows), stride=rows.shape[1], st=st.ctypes.data, ns=3, out=sco.ctypes.data), **kw)
        rc = lib.rl_model_predict_stages(a["m"], a["X"], a["n"], a["stride"], a["st"], a["ns"], a["out"])
        return rc, lib.rl_last_error().decode()

    assert pr()[0] == 0
    for kw, text in ((dict(m=None), "null model"), (dict(X=None), "null X"), (dict(st=None), "null stages"), (dict(out=None), "null output"),
                     (dict(ns=-1), "n_stages must be >= 1"), (dict(st=s99.ctypes.data), "stages[2] = 38 is outside [1, 37]"),
                     (dict(st=sdup.ctypes.data), "stages must be strictly increasing (stages[2])"), (dict(stride=0), "row_stride must be >= 1"),
                     (dict(n=-1), "n_docs must be >= 0"), (dict(m=empty.h), "the model has no trees")):
        rc, msg = pr(**kw)
        assert rc == -1 and msg == "rl_model_predict_stages: " + text, (kw, rc, msg)
    with pytest.raises(N.RankLibError, match="null argument"):
        N.check(lib.rl_debug_stage_times(None, None))
    with pytest.raises(N.RankLibError, match="metric must be one of"):
        m.eval_stages(rows, lab, qoff, "F1", 10, [1])
    walk, rank = N.stage_times()
    assert walk >= 0.0 and rank >= 0.0


# ---- 10. the command line --------------------------------------------------------------------------------------------------------------
def idv_all(path):
    line = open(path).read().splitlines()[-1].split("   ")
    assert line[1] == "all"
    return line[2]


def test_command_line(tmp_path):
    trees, w, rows, lab, qoff, _, _ = main_data()
    cut = int(qoff[8])                                      # lists of 1 .. 65 documents: 243 documents
    f1, f2, mf = str(tmp_path / "f1.txt"), str(tmp_path / "f2.txt"), str(tmp_path / "m.txt")
    with open(f1, "w") as f:
        f.write(letor_text(rows[:cut], lab[:cut], qoff[:9]))
    with open(f2, "w") as f:
        f.write(letor_text(rows[int(qoff[5]):cut], lab[int(qoff[5]):cut], qoff[5:9] - qoff[5]))
    with open(mf, "w", encoding="ascii") as f:
        f.write(TM.model_text(trees, w))
    curve, saved = str(tmp_path / "curve.txt"), str(tmp_path / "best.txt")
    metric = "NDCG@10"
    assert stages.main(["-load", mf, "-test", f1, "-test", f2, "-metric2T", metric, "-step", "7", "-curve", curve, "-save", saved, "-pick", "2"]) == 0
    table = [ln.split("\t") for ln in open(curve).read().splitlines()]
    assert [int(r[0]) for r in table] == [7, 14, 21, 28, 35, 37] and all(len(r) == 3 for r in table)
    for col, tf in ((1, f1), (2, f2)):                      # the whole model: what the evaluator reports for the file
        idv = str(tmp_path / ("all%d.idv" % col))
        assert evaluator.main(["-load", mf, "-test", tf, "-metric2T", metric, "-idv", idv]) == 0
        assert table[-1][col] == idv_all(idv)
    col2 = [float(r[2]) for r in table]
    best = col2.index(max(col2))                            # index(): the earliest of equal maxima
    text = open(saved).read()
    assert "## rlhip: first %d of 37 trees\n" % int(table[best][0]) in text and text.count("<tree ") == int(table[best][0])
    idv = str(tmp_path / "best.idv")
    assert evaluator.main(["-load", saved, "-test", f2, "-metric2T", metric, "-idv", idv]) == 0
    assert idv_all(idv) == table[best][2]
    one = str(tmp_path / "one.txt")                         # one file, every tree, the default pick
    assert stages.main(["-load", mf, "-test", f1, "-metric2T", "MAP", "-curve", one]) == 0
    rows1 = [ln.split("\t") for ln in open(one).read().splitlines()]
    assert [int(r[0]) for r in rows1] == list(range(1, 38)) and all(len(r) == 2 for r in rows1)
    lin = str(tmp_path / "lin.txt")
    with open(lin, "w") as f:
        f.write("## Coordinate Ascent\n## Restart = 5\n2:0.5 4:-0.25 6:0.125")
    with pytest.raises(N.RankLibError, match="Coordinate Ascent"):
        stages.main(["-load", lin, "-test", f1])


# ---- 11. chunks of whole lists ---------------------------------------------------------------------------------------------------------
SCORERS = {"NDCG@10": lambda: M.NDCGScorer(10), "MAP": M.APScorer, "ERR@3": lambda: M.ERRScorer(3)}


@pytest.mark.parametrize("metric", sorted(SCORERS))
def test_staged_scores_in_chunks_of_whole_lists_equal_the_one_chunk(metric, monkeypatch):
    """list_cases under its small limit: five eval_stages calls (one ends in the empty list, one list alone over the limit, the second
    list of the shared id in a later call than the first) give the bits of the one call, and leave the scorer with the same entries"""
    samples = LC.lists()
    ranker = RankerFactory().loadRankerFromString(LC.model_text())
    calls = []
    inner = ranker._model.eval_stages
    monkeypatch.setattr(ranker._model, "eval_stages", lambda rows, *a, **kw: (calls.append(len(rows)), inner(rows, *a, **kw))[1])
    one_scorer, many_scorer = SCORERS[metric](), SCORERS[metric]()
    one = ranker.stagedScores(samples, one_scorer)
    assert calls == [sum(LC.SIZES)] and one.shape == (6, len(LC.SIZES))
    del calls[:]
    monkeypatch.setattr(Ranker, "EVAL_ROW_BYTES", LC.SMALL_LIMIT)
    many = ranker.stagedScores(samples, many_scorer)
    assert calls == LC.CHUNK_ROWS
    assert np.array_equal(bits(many), bits(one))
    assert np.array_equal(bits(one[:, 2]), bits(np.zeros(6)))        # the empty list: the scorer's own answer
    assert (bits(one[0]) != bits(one[-1])).any()                     # the stages are told apart
    gains = getattr(one_scorer, "idealGains", None)
    assert getattr(many_scorer, "idealGains", None) == gains
    assert (set(gains) == set(LC.IDS) - {None}) if metric == "NDCG@10" else gains is None
