"""Accumulated local effects on the GPU (rl_model_predict_ale, rl_ale.inc) against tests/ale_restatement.py and against
predict_rows on the two materialised matrices.  Bit patterns everywhere, no tolerance (where the reference is NaN the kernel's is NaN)."""
import functools
import os

import numpy as np
import pytest

import ale_restatement as AR
import partial_restatement as PD
import permuted_restatement as PR
import tree_models as TM
import walk_cases as WC
from ranklib_amd import _native as N
from ranklib_amd import partial as P
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import LambdaMART, MART, Ranker, RankerFactory, RFRanker, java_float_str

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = N.ALE_BATCH
EDGES = {1: np.array([-2, 2], np.float32), 2: np.array([-1, 0.5, 1.75], np.float32), 8: TM.GRID[::8], 4: TM.GRID[20:45:6],
         255: ((np.arange(256) - 128) / 64.0).astype(np.float32)}      # 255 intervals of 1/64: every grid value of the rows lies on an edge, 2.0 outside


@functools.lru_cache(maxsize=None)
def main_model():
    trees, w = PR.main_data()[:2]
    return N.Model(TM.model_text(trees, w))


def hold(m, trees, w, rows, cols, edges, renamed=None):      # every output of one call against the restatement (renamed: WC.compact's)
    rt, rr, rc = renamed or (trees, rows, cols)
    iv, lo, hi = AR.ale_scores(rt, w, rr, rc, edges)
    parts = [AR.cell_sums(iv[c], lo[c], hi[c], len(z) - 1) for c, z in enumerate(edges)]
    n, s = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    gn, gs, glo, ghi, giv, gb = m.predict_ale(rows, cols, edges, local=True, base=True)
    assert m.path() == N.MODEL_PATH_ALE == 11
    assert np.array_equal(giv, iv) and TM.same_scores(glo.ravel(), lo.ravel()) is None and TM.same_scores(ghi.ravel(), hi.ravel()) is None
    assert TM.same_scores(gb, TM.eval_ensemble_np(rt, w, rr)) is None and np.array_equal(gn, n)
    nan = np.isnan(s)
    assert np.array_equal(np.isnan(gs), nan) and np.array_equal(AR.bits64(gs[~nan]), AR.bits64(s[~nan]))
    return gn, gs, glo, ghi, giv, gb


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("K", [1, 2, 255])
def test_document_counts_and_interval_counts_at_their_edges(n, K):
    trees, w, rows = PR.main_data()[:3]
    rows, m = rows[100:100 + n], main_model()
    gn, gs, glo, ghi, giv, gb = hold(m, trees, w, rows, [3, 7], [EDGES[K], EDGES[8]])
    assert gn[:K].sum() + (giv[0] == 0).sum() == n and gn[K:].sum() == n
    for c, z, sc in ((3, EDGES[K], (glo[0], ghi[0])), (7, EDGES[8], (glo[1], ghi[1]))):      # the path that exists without it
        iv = P.ale_intervals(rows[:, c], z)
        for side in (0, 1):
            assert np.array_equal(AR.bits32(sc[side]), AR.bits32(m.predict_rows(PD.materialise(rows, c, np.where(iv > 0, z[np.maximum(iv, 1) - 1 + side], rows[:, c])))))
    if n > 255 and K > 1:
        assert (AR.bits32(glo) != AR.bits32(ghi)).mean() > 0.1 and (gs != 0).sum() > 2
    assert min(N.ale_times()) > 0.0


@pytest.mark.parametrize("C", [1, B - 1, B, B + 1, 2 * B + 1])
def test_column_counts_at_the_edges_of_a_batch_and_chunks_of_1_2_and_all_columns(C):      # columns repeat; 13 is at the stride, 0 untested
    trees, w, rows = PR.main_data()[:3]
    rows, m = rows[:300], main_model()
    cols = [[3, 7, 13, 1, 3, 0, 12, 5, 9][j % 9] for j in range(C)]
    edges = [EDGES[(8, 4, 2, 255, 1)[j % 5]] for j in range(C)]
    one = hold(m, trees, w, rows, cols, edges)
    for per in sorted({1, 2, C}):
        got = m.predict_ale(rows, cols, edges, local=True, base=True, scratch_bytes=300 * 4 + per * 300 * 12 + 11)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, one)), per
    got = m.predict_ale(rows, cols, edges, scratch_bytes=1)      # a chunk holds at least one column; NULL optional outputs
    assert got[2:] == (None, None, None, None) and np.array_equal(got[0], one[0]) and np.array_equal(AR.bits64(got[1]), AR.bits64(one[1]))


@pytest.mark.parametrize("case", WC.CASES)
def test_the_adversarial_models_of_the_walk_cases(case):      # the edges are the model's own thresholds: own values lie exactly on them
    trees, w = WC.trees_of(case)
    rows, cols = WC.rows(case), WC.cell_columns(case)
    edges = [g if 2 <= len(g) <= 256 else PD.TWO for g in WC.cell_grids(case)]
    gn = hold(N.Model(TM.model_text(trees, w)), trees, w, rows, cols, edges, renamed=WC.compact(trees, rows, cols))[0]
    assert gn.sum() > 0


@pytest.mark.parametrize("extra", [None, "nodes_81"])
@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_own_values_on_below_above_and_between_the_edges(extra, zero):      # a +-0.0 inner edge; a packed and an unpacked model
    trees, w = PR.trap_trees()
    if extra:
        c = TM.case(extra)[0]
        trees, w = trees + list(c.trees), np.concatenate([w, c.weights])
    rows = PR.trap_rows(np.random.default_rng(44), 333)
    z = np.array([-1, zero, 0.5, 1], np.float32)
    v = rows[:, 3]
    assert all(m.any() for m in (v == -1, (v == 0) & np.signbit(v), (v == 0) & ~np.signbit(v), v == 1, v < -1, v > 1, np.isnan(v), (v > 0) & (v < 0.5)))
    giv = hold(N.Model(TM.model_text(trees, w)), trees, w, rows, [3, 5, 2], [z, np.array([-np.inf, -0.5, np.inf], np.float32), z])[4]
    assert set(giv[0][v == 0].tolist()) == {1} and set(giv[0][v == 1].tolist()) == {3} and set(giv[0][np.isnan(v) | (v > 1) | (v < -1)].tolist()) == {0}


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
def small_file(tmp):
    rows, lab, qoff = PR.main_data()[2:5]
    path = os.path.join(tmp, "small.txt")
    with open(path, "w") as f:                               # lists of 1 .. 256 documents: 754 documents, three partial sums
        for q in range(10):
            f.write("".join("%d qid:q%d %s\n" % (int(lab[i]), q, " ".join("%d:%s" % (c, java_float_str(rows[i, c])) for c in range(1, rows.shape[1])))
                            for i in range(qoff[q], qoff[q + 1])))
    return path


def same_ale(a, b):
    return a.features == b.features and a.centre == b.centre and all(
        x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for xs, ys in zip(a[1:5] + a[6:], b[1:5] + b[6:]) for x, y in zip(xs, ys))


@pytest.mark.parametrize("head, cls", [("## LambdaMART", LambdaMART), ("## MART", MART)])
def test_the_one_pass_path_equals_the_generic_path(head, cls, tmp_path):
    trees, w = PR.main_data()[:2]
    body = TM.model_text(trees[:9], w[:9])
    ranker = RankerFactory().loadRankerFromString(body.replace("## LambdaMART", head, 1))
    assert type(ranker) is cls and type(ranker).accumulatedEffects is LambdaMART.accumulatedEffects
    samples = FeatureManager.readInput(small_file(str(tmp_path)))
    one = ranker.accumulatedEffects(samples, intervals=6, local=True)
    assert ranker._model.path() == N.MODEL_PATH_ALE
    two = Ranker.accumulatedEffects(ranker, samples, intervals=6, local=True)
    assert same_ale(one, two) and len(one.interval[0]) == 754 and all(len(z) == 7 and a.any() for z, a in zip(one.edges, one.ale))
    if cls is MART:                                          # Random Forests and Coordinate Ascent take the generic path
        forest = RankerFactory().loadRankerFromString("## Random Forests\n## No. of bags = 1\n\n" + body.split("\n\n", 1)[1])
        lin = RankerFactory().loadRankerFromString("## Coordinate Ascent\n## Restart = 5\n2:0.5 4:-0.25 6:0.125")
        assert type(forest) is RFRanker and type(forest).accumulatedEffects is type(lin).accumulatedEffects is Ranker.accumulatedEffects
        assert same_ale(forest.accumulatedEffects(samples, features=one.features, intervals=6, local=True), one)      # one bag: the bag's float score over 1
        ca = lin.accumulatedEffects(samples, intervals=4)
        assert ca.features == [2, 4, 6] and ca.lo is None and np.allclose(np.diff(ca.ale[0]) / np.diff(ca.edges[0].astype(np.float64)), 0.5)


def test_command_line_on_a_golden_file(tmp_path):
    rng = np.random.default_rng(12)
    g = TM.Gen(rng, features=range(1, 6), thresholds=np.array([0.0, 0.25, 0.5, 0.9, 2.0, 5.0, 10.0, 20.0], np.float32))
    mf, ff, out, loc = str(tmp_path / "m.txt"), str(tmp_path / "f.txt"), str(tmp_path / "ale.tsv"), str(tmp_path / "local.tsv")
    open(mf, "w", encoding="ascii").write(TM.model_text([TM.random_tree(g, int(rng.integers(2, 7))) for _ in range(12)], np.full(12, 0.1, np.float32)))
    open(ff, "w").write("4\n1\n5\n")
    test = os.path.join(ROOT, "tests", "golden", "letor", "mart_ndcg.train.txt")
    assert P.main(["-load", mf, "-test", test, "-feature", ff, "-ale", out, "-intervals", "7", "-local", loc]) == 0      # without -out
    want = Ranker.accumulatedEffects(RankerFactory().loadRankerFromFile(mf), FeatureManager.readInput(test), features=[4, 1, 5], intervals=7, local=True)
    assert open(out).read() == "".join(ln + "\n" for ln in P.ale_lines(want)) and open(loc).read() == "".join(ln + "\n" for ln in P.local_lines(want))
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert [int(r[0]) for r in rows] == sorted(int(r[0]) for r in rows) and any(float(r[3]) != 0 for r in rows) and sum(int(r[4]) for r in rows) > 0
