"""Permutation importance on the GPU (rl_model_predict_permuted / rl_model_eval_permuted: k_model_permuted_scores, rl_permimp.inc, ranked by
k_stage_eval) against tests/permuted_restatement.py and against the public path that exists without it -- the permuted
matrix materialised on the host, predict_rows on it, eval_lists on the result.  Everything is compared as bit patterns; no tolerance
anywhere (where the reference score is NaN the kernel's is NaN: tree_models.same_scores)."""
import functools
import os

import numpy as np
import pytest

import permuted_restatement as PR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import importance as I
from ranklib_amd import metric as M
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import LambdaMART, MART, Ranker, RankerFactory, RFRanker, java_float_str

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, S = TM.L, TM.S
B = N.PERMUTED_BATCH
WHOLE = 1000
METRICS = [("NDCG", 10), ("MAP", 0), ("ERR", 10), ("P", 3), ("RR", WHOLE)]


@functools.lru_cache(maxsize=None)
def main_model():
    trees, w = PR.main_data()[:2]
    return N.Model(TM.model_text(trees, w))


@functools.lru_cache(maxsize=None)
def public_scores():
    """the path that exists without the feature: every cell's matrix materialised, predict_rows on it -- f32 [14][3][n], made once"""
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    m = main_model()
    out = np.stack([np.stack([m.predict_rows(PR.materialise(rows, c, donor[r])) for r in range(3)]) for c in PR.COLUMNS])
    out.setflags(write=False)
    return out


def same64(got, want):
    return np.array_equal(PR.bits64(got), PR.bits64(want))


# ---- 1. all 14 columns, three repeats -----------------------------------------------------------------------------------------------------
def test_predict_permuted_equals_the_restatement_and_predict_rows():
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    assert ((PR.bits32(sc[1:13]) != PR.bits32(base)[None, None, :]).mean(axis=2) >= 0.5).all()      # every used column changes at least half of the scores
    gb, got = main_model().predict_permuted(rows, PR.COLUMNS, donor)
    assert main_model().path() == N.MODEL_PATH_PERMUTED
    assert got.shape == (14, 3, len(rows))
    assert TM.same_scores(gb, base) is None, TM.same_scores(gb, base)
    assert TM.same_scores(got.ravel(), sc.ravel()) is None, TM.same_scores(got.ravel(), sc.ravel())
    assert np.array_equal(PR.bits32(got), PR.bits32(public_scores()))
    assert np.array_equal(PR.bits32(gb), PR.bits32(main_model().predict_rows(rows)))
    assert np.array_equal(PR.bits32(got[0]), PR.bits32(np.tile(gb, (3, 1)))) and np.array_equal(PR.bits32(got[13]), PR.bits32(got[0]))


@pytest.mark.parametrize("metric, k", METRICS)
def test_eval_permuted_equals_the_restatement_and_eval_lists(metric, k):
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    wb, wbn, want, wnan, wideal = PR.eval_permuted(trees, w, rows, lab, qoff, metric, k, PR.COLUMNS, donor, scores=(base, sc))
    gb, gbn, got, gnan, gideal = main_model().eval_permuted(rows, lab, qoff, metric, k, PR.COLUMNS, donor)
    assert not gnan.any() and not gbn.any() and not wnan.any() and not wbn.any()
    assert same64(gb, wb) and same64(got, want) and same64(gideal, wideal), metric
    pub = public_scores()
    for c in range(14):
        for r in range(3):
            v, _, _ = N.eval_lists(pub[c, r].astype(np.float64), lab, qoff, metric, k)
            assert same64(got[c, r], v), (metric, c, r)
    v, _, _ = N.eval_lists(main_model().predict_rows(rows).astype(np.float64), lab, qoff, metric, k)
    assert same64(gb, v)
    if metric == "NDCG":
        assert all((PR.bits64(got[c, 0]) != PR.bits64(gb)).sum() >= 10 for c in range(1, 13))


# ---- 2. batch edges --------------------------------------------------------------------------------------------------------------------
UNSORTED = [9, 3, 3, 12, 0, 7, 13, 1, 8, 2, 11, 4, 6, 10, 5, 3, 9]       # 17 entries: unsorted, 3 and 9 repeated, 0 unused, 13 at the stride


@pytest.mark.parametrize("cols, reps", [([5], [0]), (UNSORTED[:5], [0, 1, 2]), (UNSORTED[2:10], [2, 0]), (UNSORTED, [1]), (UNSORTED[:11], [1, 2, 0])])
def test_cells_of_1_B_minus_1_B_B_plus_1_and_2B_plus_1(cols, reps):
    """B = 16: 1, 15, 16, 17 and 33 cells.  The base is one more cell: the last batch holds 2, B, 1, 2 and 2 cells"""
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    assert B == 16 and len(cols) * len(reps) == {1: 1, 5: B - 1, 8: B, 17: B + 1, 11: 2 * B + 1}[len(cols)]
    gb, got = main_model().predict_permuted(rows, cols, donor[reps])
    assert np.array_equal(PR.bits32(gb), PR.bits32(base))
    assert np.array_equal(PR.bits32(got), PR.bits32(sc[np.ix_(cols, reps)]))
    wb, _, want, _, _ = PR.eval_permuted(None, None, None, lab, qoff, "NDCG", 10, cols, None, scores=(base, np.ascontiguousarray(sc[np.ix_(cols, reps)])))
    eb, ebn, ev, enan, _ = main_model().eval_permuted(rows, lab, qoff, "NDCG", 10, cols, donor[reps])
    assert same64(eb, wb) and same64(ev, want) and not enan.any() and not ebn.any()


# ---- 3. chunking -----------------------------------------------------------------------------------------------------------------------
def test_chunks_of_1_2_and_5_cells_equal_the_single_chunk():
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    cols = [4, 1, 13, 8, 2]                                  # 5 x 2 cells and the base: 11, 6 and 3 chunks, the last one short
    one = main_model().eval_permuted(rows, lab, qoff, "NDCG", 10, cols, donor[:2])
    for per in (1, 2, 5):
        got = main_model().eval_permuted(rows, lab, qoff, "NDCG", 10, cols, donor[:2], scratch_bytes=per * len(rows) * 4 + 3)
        for a, b in zip(got, one):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), per
    got = main_model().eval_permuted(rows, lab, qoff, "NDCG", 10, cols, donor[:2], scratch_bytes=1)      # a chunk holds at least one cell
    assert same64(got[2], one[2]) and same64(got[0], one[0])
    wb, _, want, _, _ = PR.eval_permuted(None, None, None, lab, qoff, "NDCG", 10, cols, None, scores=(base, np.ascontiguousarray(sc[np.ix_(cols, [0, 1])])))
    assert same64(one[0], wb) and same64(one[2], want)


# ---- 4. trap trees ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra, tiled", [(None, True), ("nan_leaf", False), ("nodes_81", False)])
def test_trap_trees_on_packed_and_unpacked_models(extra, tiled):
    """a chain on one column, the column at the root and again below both children, single leaves, a tree that uses the column beside one
    that does not, thresholds equal to donated values, donated NaN, +-Infinity and -0.0 -- alone (a model the tiled kernel packs) and in
    front of the trees of a model it refuses.  Both take k_model_permuted_scores."""
    trees, w = PR.trap_trees()
    if extra:
        c = TM.case(extra)[0]
        trees, w = trees + list(c.trees), np.concatenate([w, c.weights])
    rng = np.random.default_rng(44)
    rows = PR.trap_rows(rng, 333)
    donor = np.stack([rng.permutation(333), rng.integers(0, 333, 333)]).astype(np.int32)
    sp = rows[donor[0], 3]
    assert np.isnan(sp).any() and np.isposinf(sp).any() and (sp.view(np.uint32) == 0x80000000).any()
    cols = [3, 5, 2, 7, 3, 12, 1, 4, 6]                      # 18 cells and the base: two batches
    wb, want = PR.permuted_scores(trees, w, rows, cols, donor)
    m = N.Model(TM.model_text(trees, w))
    gb, got = m.predict_permuted(rows, cols, donor)
    assert m.path() == N.MODEL_PATH_PERMUTED
    assert TM.same_scores(gb, wb) is None and TM.same_scores(got.ravel(), want.ravel()) is None, TM.same_scores(got.ravel(), want.ravel())
    assert (PR.bits32(want[0, 0]) != PR.bits32(wb)).mean() > 0.5
    pub = m.predict_rows(PR.materialise(rows, 3, donor[1]))
    assert m.path() == (N.MODEL_PATH_TILED if tiled else N.MODEL_PATH_GENERIC)
    assert TM.same_scores(got[0, 1], pub) is None


# ---- 5. a NaN cell ---------------------------------------------------------------------------------------------------------------------
def letor_text(rows, lab, qoff):
    out = []
    for q in range(len(qoff) - 1):
        for i in range(qoff[q], qoff[q + 1]):
            out.append("%d qid:q%d %s\n" % (int(lab[i]), q, " ".join("%d:%s" % (f, java_float_str(rows[i, f])) for f in range(1, rows.shape[1]))))
    return "".join(out)


def generic(ranker, *a, **kw):
    return Ranker.permutationImportance(ranker, *a, **kw)


def same_importance(a, b):
    return (a.features == b.features and same64(a.base, b.base) and same64(a.values, b.values) and same64(a.importance, b.importance)
            and same64(a.std, b.std) and same64(a.repeat_means, b.repeat_means) and same64([a.base_mean], [b.base_mean]))


def test_a_nan_cell_is_flagged_and_filled(tmp_path):
    rng = np.random.default_rng(77)
    g = TM.Gen(rng)
    trees = [TM.random_tree(g, int(rng.integers(2, 9))) for _ in range(8)]
    trees[3] = TM.flatten(S(3, -1.9, L(np.nan), L(0.25)))   # two of the grid's 65 values go left
    w = np.full(8, 0.1, np.float32)
    lens = [5, 12, 3, 20, 40, 8, 16, 100, 2, 30]
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = rng.choice(TM.GRID, (int(qoff[-1]), 13)).astype(np.float32)
    rows[:, 0] = 0.0
    lab = rng.integers(0, 5, int(qoff[-1])).astype(np.float32)
    donor = I.donor_maps(lens, 2, seed=1)
    holds = lambda x3: np.array([(x3[qoff[q]:qoff[q + 1]] <= -1.9).any() for q in range(len(lens))])      # noqa: E731
    hb, h0, h1 = holds(rows[:, 3]), holds(rows[donor[0], 3]), holds(rows[donor[1], 3])
    assert hb.any() and not hb.all() and (h0 != hb).any() and h0.any() and not h0.all()
    text = TM.model_text(trees, w)
    m = N.Model(text)
    gb, gbn, got, gnan, _ = m.eval_permuted(rows, lab, qoff, "NDCG", 10, [3, 5], donor)
    wb, wbn, want, wnan, _ = PR.eval_permuted(trees, w, rows, lab, qoff, "NDCG", 10, [3, 5], donor)
    assert np.array_equal(gbn != 0, hb) and np.array_equal(gnan[0, 0] != 0, h0) and np.array_equal(gnan[0, 1] != 0, h1)
    assert np.array_equal(gnan[1, 0] != 0, hb) and np.array_equal(gnan[1, 1] != 0, hb)                   # column 5 leaves the NaN where the base has it
    assert np.array_equal(gnan, wnan) and np.array_equal(gbn, wbn) and same64(got, want) and same64(gb, wb)
    assert not got[gnan != 0].any() and got[gnan == 0].any()                                              # the neighbours are ranked
    path = str(tmp_path / "nan.txt")
    with open(path, "w") as f:
        f.write(letor_text(rows, lab, qoff))
    samples = FeatureManager.readInput(path)
    ranker = RankerFactory().loadRankerFromString(text)
    for scorer in (lambda: M.NDCGScorer(10), M.APScorer):
        one = ranker.permutationImportance(samples, scorer(), features=[3, 5], repeats=2)
        assert same_importance(one, generic(ranker, samples, scorer(), features=[3, 5], repeats=2))
        assert np.isfinite(one.values).all()


# ---- 6. small and degenerate calls -----------------------------------------------------------------------------------------------------
def test_one_document_a_constant_donor_and_the_identity():
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    m = main_model()
    gb, got = m.predict_permuted(rows[40:41], [1, 2, 3], [[0], [0]])
    assert got.shape == (3, 2, 1) and np.array_equal(PR.bits32(got), PR.bits32(np.full((3, 2, 1), base[40]))) and PR.bits32(gb)[0] == PR.bits32(base)[40]
    eb, _, ev, enan, _ = m.eval_permuted(rows[40:41], lab[40:41], [0, 1], "NDCG", 10, [1], [0])
    assert ev.shape == (1, 1, 1) and same64(ev[0, 0], eb) and not enan.any()
    n = len(rows)
    two = np.stack([np.full(n, 17), np.arange(n)]).astype(np.int32)
    cols = list(range(1, 13))
    wb, want = PR.permuted_scores(trees, w, rows, cols, two)
    gb, got = m.predict_permuted(rows, cols, two)
    assert np.array_equal(PR.bits32(got), PR.bits32(want)) and np.array_equal(PR.bits32(gb), PR.bits32(base))
    assert np.array_equal(PR.bits32(got[:, 1]), PR.bits32(np.tile(base, (12, 1))))                        # the identity: every cell equals the base bit for bit
    assert ((PR.bits32(got[:, 0]) != PR.bits32(base)[None, :]).mean(axis=1) > 0.3).all()                  # a constant donor is a legal map
    eb, _, ev, _, _ = m.eval_permuted(rows, lab, qoff, "MAP", 0, cols, two)
    assert same64(ev[:, 1], np.tile(eb, (12, 1)))


def test_a_list_of_the_global_class():
    rng = np.random.default_rng(62)
    g = TM.Gen(rng)
    trees = [TM.random_tree(g, int(rng.integers(3, 9))) for _ in range(5)]
    w = np.array([0.1, 1.0, 0.5, -0.25, 0.1], np.float32)
    qoff = np.array([0, 6200, 6230], np.int32)
    rows = rng.choice(TM.GRID, (6230, 13)).astype(np.float32)
    rows[:, 0] = 0.0
    lab = rng.integers(0, 5, 6230).astype(np.float32)
    donor = np.random.RandomState(1).permutation(6230).astype(np.int32)
    col = int(trees[0]["feature"][0])
    wb, wbn, want, wnan, _ = PR.eval_permuted(trees, w, rows, lab, qoff, "NDCG", 10, [col, 13], donor)
    m = N.Model(TM.model_text(trees, w))
    gb, gbn, got, gnan, _ = m.eval_permuted(rows, lab, qoff, "NDCG", 10, [col, 13], donor)
    assert same64(gb, wb) and same64(got, want) and not gnan.any() and not gbn.any()
    assert not same64(got[0, 0], gb) and same64(got[1, 0], gb)
    got2 = m.eval_permuted(rows, lab, qoff, "NDCG", 10, [col, 13], donor, scratch_bytes=16 * 6230)       # 16 bytes per document and cell here: three chunks
    assert same64(got2[2], got) and same64(got2[0], gb)


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------------
def small_file(tmp):
    trees, w, rows, lab, qoff, _, _, _ = PR.main_data()
    cut = int(qoff[8])                                      # lists of 1 .. 65 documents: 243 documents
    path = os.path.join(tmp, "small.txt")
    with open(path, "w") as f:
        f.write(letor_text(rows[:cut], lab[:cut], qoff[:9]))
    return path


@pytest.mark.parametrize("head, cls", [("## LambdaMART", LambdaMART), ("## MART", MART)])
@pytest.mark.parametrize("within", [False, True])
def test_the_one_pass_path_equals_the_generic_path(head, cls, within, tmp_path, monkeypatch):
    trees, w = PR.main_data()[:2]
    text = TM.model_text(trees[:9], w[:9]).replace("## LambdaMART", head, 1)
    ranker = RankerFactory().loadRankerFromString(text)
    assert type(ranker) is cls
    samples = FeatureManager.readInput(small_file(str(tmp_path)))
    feats = [2, 7, 11]
    one = ranker.permutationImportance(samples, M.NDCGScorer(10), features=feats, repeats=2, seed=3, within=within)
    assert ranker._model.path() == N.MODEL_PATH_PERMUTED
    two = generic(ranker, samples, M.NDCGScorer(10), features=feats, repeats=2, seed=3, within=within)
    assert same_importance(one, two) and one.values.shape == (3, 2, 8) and one.importance.any()
    if within:                                              # chunks of whole lists: the donors stay inside them, so the cut changes no bit
        monkeypatch.setattr(Ranker, "EVAL_ROW_BYTES", 20 * 13 * 4)
        assert same_importance(ranker.permutationImportance(samples, M.NDCGScorer(10), features=feats, repeats=2, seed=3, within=True), one)
    else:                                                   # the model's own features, ascending
        all_f = ranker.permutationImportance(samples, M.APScorer(), repeats=1)
        assert all_f.features == sorted({int(f) for t in trees[:9] for f in t["feature"] if f != -1})


def test_random_forests_and_coordinate_ascent_take_the_generic_path(tmp_path):
    trees, w = PR.main_data()[:2]
    body = TM.model_text(trees[:9], w[:9])
    samples = FeatureManager.readInput(small_file(str(tmp_path)))
    forest = RankerFactory().loadRankerFromString("## Random Forests\n## No. of bags = 1\n\n" + body.split("\n\n", 1)[1])
    assert type(forest) is RFRanker and type(forest).permutationImportance is Ranker.permutationImportance
    rf = forest.permutationImportance(samples, M.NDCGScorer(10), features=[2, 7], repeats=2)
    lm = RankerFactory().loadRankerFromString(body).permutationImportance(samples, M.NDCGScorer(10), features=[2, 7], repeats=2)
    assert same_importance(rf, lm)                          # one bag: the bag's float score over 1, the same ranking
    lin = RankerFactory().loadRankerFromString("## Coordinate Ascent\n## Restart = 5\n2:0.5 4:-0.25 6:0.125")
    ca = lin.permutationImportance(samples, M.NDCGScorer(10), repeats=2)
    assert ca.features == [2, 4, 6] and ca.values.shape == (3, 2, 8) and ca.importance.any() and np.isfinite(ca.values).all()
    flat, _ = lin.evalLists(samples)
    assert same64(ca.base, M.score_lists(M.NDCGScorer(10), samples, flat)[0])


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_on_a_golden_file(tmp_path):
    rng = np.random.default_rng(12)
    g = TM.Gen(rng, features=range(1, 6), thresholds=np.array([0.0, 0.25, 0.5, 0.9, 2.0, 5.0, 10.0, 20.0], np.float32))
    trees = [TM.random_tree(g, int(rng.integers(2, 7))) for _ in range(12)]
    mf, ff, out = str(tmp_path / "m.txt"), str(tmp_path / "f.txt"), str(tmp_path / "imp.tsv")
    with open(mf, "w", encoding="ascii") as f:
        f.write(TM.model_text(trees, np.full(12, 0.1, np.float32)))
    with open(ff, "w") as f:
        f.write("4\n1\n5\n")
    test = os.path.join(ROOT, "tests", "golden", "letor", "mart_ndcg.train.txt")
    assert I.main(["-load", mf, "-test", test, "-metric2T", "NDCG@10", "-repeat", "2", "-seed", "4", "-feature", ff, "-out", out]) == 0
    ranker = RankerFactory().loadRankerFromFile(mf)
    want = generic(ranker, FeatureManager.readInput(test), M.NDCGScorer(10), features=[4, 1, 5], repeats=2, seed=4)
    assert open(out).read() == "".join(ln + "\n" for ln in I.table_lines(want))
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert sorted(int(r[0]) for r in rows) == [1, 4, 5] and all(len(r) == 6 for r in rows)
    imp = [float(r[1]) for r in rows]
    assert imp == sorted(imp, reverse=True) and any(imp)
    assert I.main(["-load", mf, "-test", test, "-metric2T", "MAP", "-repeat", "1", "-within", "-out", out]) == 0
    assert sorted(int(ln.split("\t")[0]) for ln in open(out).read().splitlines()) == [int(f) for f in ranker.getFeatures()]


# ---- 9. refusals that need a model -----------------------------------------------------------------------------------------------------
def test_refusals_behind_the_model():
    lib = N.lib()
    trees, w, rows, lab, qoff, donor, _, _ = PR.main_data()
    m = main_model()
    cols = np.array([1, 2], np.int32)
    nl = len(PR.LENS)
    ov, on, bv, bn = np.zeros((2, 3, nl)), np.zeros((2, 3, nl), np.uint8), np.zeros(nl), np.zeros(nl, np.uint8)
    base = dict(m=m.h, lab=lab.ctypes.data, qoff=qoff.ctypes.data, nl=nl, metric=0, k=10, err_max=16.0, scratch=0, bv=bv.ctypes.data, bn=bn.ctypes.data,
                ov=ov.ctypes.data, on=on.ctypes.data)

    def ev(**kw):
        a = dict(base, **kw)
        rc = lib.rl_model_eval_permuted(a["m"], rows.ctypes.data, len(rows), rows.shape[1], a["lab"], a["qoff"], a["nl"], None, None, None, a["metric"],
                                        a["k"], a["err_max"], cols.ctypes.data, 2, donor.ctypes.data, 3, a["scratch"], a["bv"], a["bn"], a["ov"], a["on"], None)
        return rc, lib.rl_last_error().decode()

    assert ev()[0] == 0
    empty = N.Model("## LambdaMART\n\n<ensemble>\n</ensemble>\n")
    q1 = np.array([1] + list(qoff[1:]), np.int32)
    neg = lab.copy(); neg[7] = -1.0
    for kw, text in ((dict(m=empty.h), "the model has no trees"), (dict(on=None), "null out_nan"), (dict(bv=None), "null out_base"),
                     (dict(bn=None), "null out_base_nan"), (dict(scratch=-1), "scratch_bytes must be >= 0"), (dict(lab=None), "null argument"),
                     (dict(metric=7), "unknown metric 7"), (dict(nl=0), "n_lists and n_docs must be >= 1"), (dict(qoff=q1.ctypes.data), "qoff must start at 0"),
                     (dict(lab=neg.ctypes.data), "Relevance label cannot be negative. System will now exit."),
                     (dict(metric=3, err_max=0.0), "err_max (ERRScorer.MAX) must be positive and finite")):
        rc, msg = ev(**kw)
        assert rc == -1 and msg == "rl_model_eval_permuted: " + text, (kw, rc, msg)
    with pytest.raises(N.RankLibError, match="the model has no trees"):
        empty.predict_permuted(rows, [1], donor)
    with pytest.raises(N.RankLibError, match="metric must be one of"):
        m.eval_permuted(rows, lab, qoff, "F1", 10, [1], donor)
    with pytest.raises(N.RankLibError, match="donor \\[n_repeats\\]\\[n_docs\\]"):
        m.predict_permuted(rows, [1], donor[:, :5])
    walk, rank = N.permuted_times()
    assert walk >= 0.0 and rank >= 0.0
