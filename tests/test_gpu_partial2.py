"""Two-feature partial dependence on the GPU (rl_model_predict_partial2: k_model_partial2_scores, rl_partial2.inc, and k_partial_reduce;
DESIGN.md 35) against tests/partial2_restatement.py and against the public path that exists without it -- the matrix with both columns
substituted materialised on the host, predict_rows on it.  Everything is compared as bit patterns; no tolerance anywhere (where the
reference score is NaN the kernel's is NaN: tree_models.same_scores)."""
import functools
import os

import numpy as np
import pytest

import partial2_restatement as P2
import partial_restatement as PD
import permuted_restatement as PR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import partial as P
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import LambdaMART, MART, Ranker, RankerFactory, RFRanker
from test_gpu_partial import same32, same64, small_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, S = TM.L, TM.S
T = N.PARTIAL2_TILE_A
INF = np.float32(np.inf)
TRAP_GRID = np.array([-INF, -1, -0.5, 0, 0.25, 0.5, 1, INF], np.float32)


@functools.lru_cache(maxsize=None)
def main_model():
    trees, w = PR.main_data()[:2]
    return N.Model(TM.model_text(trees, w))


def check(m, trees, w, rows, pairs, grids, **kw):
    """predict_partial2 against the materialised restatement in ICE, base, mean and shift2; returns (got, want scores)"""
    wb, want = P2.partial2_scores(trees, w, rows, pairs, grids)
    wm, ws = PD.reduce_cells(wb, want)
    got = m.predict_partial2(rows, pairs, grids, ice=True, **kw)
    assert m.path() == N.MODEL_PATH_PARTIAL2
    assert TM.same_scores(got[0], wb) is None and TM.same_scores(got[3].ravel(), want.ravel()) is None, TM.same_scores(got[3].ravel(), want.ravel())
    nan = np.isnan(ws)                                          # (NaN - NaN: the payload is open, as tests/test_gpu_partial.py has it)
    assert same64(got[1], wm) and np.array_equal(np.isnan(got[2]), nan) and same64(got[2][~nan], ws[~nan])
    return got, want


# ---- 1. the main data: three pairs that trees test together, 9 x 10 cells each -----------------------------------------------------------
def test_predict_partial2_equals_the_restatement_and_predict_rows():
    assert N.PARTIAL2_TILE_A == N.PARTIAL2_TILE_B
    rows = PR.main_data()[2]
    pairs, grids, base, sc, mean, shift2 = P2.main_partial2()
    m = main_model()
    gb, gm, gs, gi = m.predict_partial2(rows, pairs, grids, ice=True)
    assert m.path() == N.MODEL_PATH_PARTIAL2 and gi.shape == (270, len(rows))
    assert same32(gb, base) and same32(gi, sc), TM.same_scores(gi.ravel(), sc.ravel())
    assert same64(gm, mean) and same64(gs, shift2)
    at = [(p, u, v) for p in range(3) for u in (0, 4, 8) for v in (0, 9)]      # the path that exists without it, on 18 cells
    for p, u, v in at:
        pub = m.predict_rows(P2.materialise2(rows, pairs[p][0], grids[p][0][u], pairs[p][1], grids[p][1][v]))
        assert same32(gi[90 * p + 10 * u + v], pub)
    assert same32(gb, m.predict_rows(rows))
    walk, red = N.partial2_times()
    assert walk > 0.0 and red > 0.0


# ---- 2. tile edges, transposition, repeats, untested columns -------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("k", [1, T - 1, T, T + 1, 2 * T + 1])
def test_grids_of_1_T_minus_1_T_T_plus_1_and_2T_plus_1_values_on_each_axis(axis, k):
    """one pair's grid of k values on one axis between other pairs: (b, a) is the transposed (a, b), a pair repeats, column 0 is tested
    by no tree (only a, only b, neither), 13 lies at the row stride"""
    trees, w, rows = PR.main_data()[:3]
    rows = rows[:300]
    a, b = P2.main_pairs()[0]
    gk, g3 = TM.GRID[np.unique(np.arange(k) * 64 // max(1, k - 1))], TM.GRID[[10, 30, 50]]
    assert len(gk) == k
    pairs = [(a, b), (b, a), (a, 0), (0, b), (0, 13), (a, b)]
    grids = [(gk, g3) if axis == 0 else (g3, gk), (g3, gk) if axis == 0 else (gk, g3), (g3, PD.TWO), (PD.TWO, g3), (PD.TWO, PD.TWO), (g3, g3)]
    (gb, gm, gs, gi), want = check(main_model(), trees, w, rows, pairs, grids)
    n = 3 * k
    first = gi[:n].reshape(grids[0][0].size, grids[0][1].size, -1)
    assert same32(gi[n:2 * n].reshape(grids[1][0].size, grids[1][1].size, -1).transpose(1, 0, 2), first)
    assert same32(gi[2 * n + 12:2 * n + 16], np.tile(gb, (4, 1)))                               # (0, 13): the base in every cell
    assert same32(gi[2 * n:2 * n + 6:2], gi[2 * n + 1:2 * n + 6:2]) and same32(gi[2 * n + 6:2 * n + 9], gi[2 * n + 9:2 * n + 12])      # column 0 moves nothing
    assert (PD.bits32(first) != PD.bits32(gb)).any(axis=2).mean() >= 0.25


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_document_counts_at_the_edges_of_the_reduction_block(n):
    trees, w, rows = PR.main_data()[:3]
    pairs = P2.main_pairs()[:2]
    check(main_model(), trees, w, rows[100:100 + n], pairs, P2.pair_grids(pairs, 5, 9))


def test_chunks_of_one_tile_and_of_a_few_equal_the_single_chunk():
    rows = PR.main_data()[2]
    n = len(rows)
    pairs, grids, base, sc, mean, shift2 = P2.main_partial2()
    m = main_model()
    for cells in (T * T, 3 * T * T + 5, 7, 1):                # one tile, three tiles, less than a tile (the tiles are cut), one cell
        got = m.predict_partial2(rows, pairs, grids, ice=True, scratch_bytes=n * 4 + cells * n * 4 + 3)
        assert same32(got[0], base) and same32(got[3], sc) and same64(got[1], mean) and same64(got[2], shift2), cells


# ---- 3. trap trees, a column beyond the stride, a deep chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("extra, tiled", [(None, True), ("nodes_81", False)])
def test_trap_trees_on_packed_and_unpacked_models(extra, tiled):
    """grid values equal to thresholds, +-Infinity, -0.0 against the threshold 0.0 and +-F32_MAX; NaN, +-Infinity and -0.0 in the rows' own
    columns 3 and 5, which stay the documents' own where the pair is another"""
    trees, w = PR.trap_trees()
    if extra:
        c = TM.case(extra)[0]
        trees, w = trees + list(c.trees), np.concatenate([w, c.weights])
    rows = PR.trap_rows(np.random.default_rng(44), 333)
    assert np.isnan(rows[:, 3]).any() and np.isnan(rows[:, 5]).any()
    edge = np.array([-TM.F32_MAX, -0.0, TM.F32_MAX], np.float32)
    pairs = [(3, 5), (5, 3), (3, 7), (2, 7), (5, 13), (3, 2)]
    grids = [(TRAP_GRID, TRAP_GRID), (edge, TRAP_GRID), (TRAP_GRID, [0.25]), (TRAP_GRID, edge), (TRAP_GRID[2:], [0.0]), (edge, edge)]
    m = N.Model(TM.model_text(trees, w))
    (gb, gm, gs, gi), want = check(m, trees, w, rows, pairs, grids)
    assert (PD.bits32(want[:64]) != PD.bits32(gb)[None, :]).mean(axis=1).min() > 0.25
    pub = m.predict_rows(P2.materialise2(rows, 3, -INF, 5, INF))
    assert m.path() == (N.MODEL_PATH_TILED if tiled else N.MODEL_PATH_GENERIC) and TM.same_scores(gi[7], pub) is None


def test_a_column_beyond_the_row_stride_that_the_model_tests():
    trees, w, rows = PR.main_data()[:3]
    narrow = np.ascontiguousarray(rows[:400, :4])
    pairs = [(12, 2), (5, 12), (3, 40)]
    grids = [(TM.GRID[::7], TM.GRID[2::9]), (TM.GRID[1::6], TM.GRID[::13]), (TM.GRID[::9], PD.TWO)]
    (gb, gm, gs, gi), want = check(main_model(), trees, w, narrow, pairs, grids)
    assert same32(gb, main_model().predict_rows(narrow)) and (PD.bits32(want[:80]) != PD.bits32(gb)[None, :]).mean() > 0.25


def test_a_chain_of_depth_48_keeps_the_stack_within_its_bound():
    """a chain that tests a and b in turn at 48 levels and goes on to the LEFT, thresholds descending: every level parts a suffix of one
    axis' values, whose leaf waits on the stack while the chain goes on -- with 17 values on either axis many wait at once, yet never
    more than 2 T - 2"""
    nested = L(100.0)
    for d in reversed(range(48)):
        nested = S(1 + d % 2, 12.0 - float(d // 2) - 0.5 * (d % 2), nested, L(float(d) + 0.5))
    trees, w = [TM.flatten(nested), TM.flatten(S(3, 0.0, L(-1.0), L(1.0)))], np.array([0.5, 1.0], np.float32)
    assert TM.depth_of(trees[0]) >= 40
    rows = np.random.default_rng(5).choice(TM.GRID, (130, 4)).astype(np.float32)
    g = (np.arange(2 * T + 1) * 1.75 - 14.0).astype(np.float32)
    grids = [(g, g + np.float32(0.25))]
    assert P2.partial2_scores_descent(trees, w, rows[:3], [(1, 2)], grids, T, T)[1] >= T   # (the restatement's descent: the stack is used in depth)
    (gb, gm, gs, gi), want = check(N.Model(TM.model_text(trees, w)), trees, w, rows, [(1, 2)], grids)
    assert len({x for x in gm.tolist()}) > 20


# ---- 4. optional outputs and refusals ---------------------------------------------------------------------------------------------------
def test_null_ice_null_base_and_the_refusals_behind_a_model():
    rows = PR.main_data()[2]
    pairs, grids, base, sc, mean, shift2 = P2.main_partial2()
    m, lib = main_model(), N.lib()
    nb, nm, ns, ni = m.predict_partial2(rows, pairs, grids)
    assert ni is None and same32(nb, base) and same64(nm, mean) and same64(ns, shift2)
    prs = np.array(pairs, np.int32)
    off = np.concatenate([[0], np.cumsum([len(g) for pr in grids for g in pr])]).astype(np.int32)
    grid = np.concatenate([g for pr in grids for g in pr]).astype(np.float32)
    gm, gs = np.zeros(270), np.zeros(270)
    N.check(lib.rl_model_predict_partial2(m.h, rows.ctypes.data, len(rows), rows.shape[1], prs.ctypes.data, 3, off.ctypes.data, grid.ctypes.data, 0,
                                          None, gm.ctypes.data, gs.ctypes.data, None))
    assert same64(gm, mean) and same64(gs, shift2)
    empty = N.Model("## LambdaMART\n\n<ensemble>\n</ensemble>\n")
    with pytest.raises(N.RankLibError, match="rl_model_predict_partial2: the model has no trees"):
        empty.predict_partial2(rows, [(1, 2)], [([0.0], [0.0])])
    with pytest.raises(N.RankLibError, match=r"rl_model_predict_partial2: pairs\[1\] = \(4, 4\) names one column twice"):
        m.predict_partial2(rows, [(1, 2), (4, 4)], [([0.0], [0.0])] * 2)
    with pytest.raises(N.RankLibError, match=r"rl_model_predict_partial2: grid\[1\]\[2\] = 0.5 is not greater than its predecessor 0.5"):
        m.predict_partial2(rows, [(1, 2)], [([0.0], [0.0, 0.5, 0.5])])
    with pytest.raises(N.RankLibError, match="one \\(grid_a, grid_b\\) of 1-d grids per pair"):
        m.predict_partial2(rows, [(1, 2), (2, 3)], [([0.0], [0.0])])
    assert same32(m.predict_partial2(rows, pairs[:1], grids[:1])[0], base) and m.path() == N.MODEL_PATH_PARTIAL2      # and the model still answers


# ---- 5. the Python layer and the command line ----------------------------------------------------------------------------------------------
def same_partial2(a, b):
    ok = a.pairs == b.pairs and same64(a.base, b.base) and a.base_mean == b.base_mean and same64(a.h2, b.h2) and (a.ice is None) == (b.ice is None)
    for p in range(len(a.pairs)):
        ok = ok and all(same32(x, y) for x, y in zip(a.grids[p], b.grids[p])) and same64(a.mean[p], b.mean[p]) and same64(a.centred[p], b.centred[p])
        ok = ok and same64(a.rms[p], b.rms[p]) and (a.ice is None or same64(a.ice[p], b.ice[p]))
    return bool(ok)


@pytest.mark.parametrize("head, cls", [("## LambdaMART", LambdaMART), ("## MART", MART), ("## Random Forests", RFRanker)])
def test_the_one_pass_path_equals_the_generic_path(head, cls, tmp_path):
    trees, w = PR.main_data()[:2]
    text = TM.model_text(trees[:9], w[:9])
    text = text.replace("## LambdaMART", head, 1) if cls is not RFRanker else "## Random Forests\n## No. of bags = 1\n\n" + text.split("\n\n", 1)[1]
    ranker = RankerFactory().loadRankerFromString(text)
    assert type(ranker) is cls
    assert type(ranker).partialDependence2 is (Ranker.partialDependence2 if cls is RFRanker else LambdaMART.partialDependence2)
    samples = FeatureManager.readInput(small_file(str(tmp_path)))
    pr = sorted(P2.together(trees[:9]))[0]
    one = ranker.partialDependence2(samples, [pr, pr[::-1]], grid=4, ice=True)
    if cls is not RFRanker:
        assert same_partial2(one, Ranker.partialDependence2(ranker, samples, [pr, pr[::-1]], grid=4, ice=True))
    lm = RankerFactory().loadRankerFromString(TM.model_text(trees[:9], w[:9])).partialDependence2(samples, [pr, pr[::-1]], grid=4, ice=True)
    assert same_partial2(one, lm) and one.h2[0] > 0 and np.array_equal(one.mean[0], one.mean[1].T) and len(one.base) == 754


def test_command_line_on_a_golden_file(tmp_path):
    rng = np.random.default_rng(12)
    g = TM.Gen(rng, features=range(1, 6), thresholds=np.array([0.0, 0.25, 0.5, 0.9, 2.0, 5.0, 10.0, 20.0], np.float32))
    trees = [TM.random_tree(g, int(rng.integers(2, 7))) for _ in range(12)]
    mf, pf, out, out2, ice2, alone = (str(tmp_path / n) for n in ("m.txt", "p.txt", "pd.tsv", "pd2.tsv", "ice2.tsv", "alone.tsv"))
    with open(mf, "w", encoding="ascii") as f:
        f.write(TM.model_text(trees, np.full(12, 0.1, np.float32)))
    with open(pf, "w") as f:
        f.write("4 1\n2 5\n")
    test = os.path.join(ROOT, "tests", "golden", "letor", "mart_ndcg.train.txt")
    assert P.main(["-load", mf, "-test", test, "-grid", "7", "-out", out, "-pairs", pf, "-grid2", "5", "-out2", out2, "-ice2", ice2]) == 0
    assert P.main(["-load", mf, "-test", test, "-grid", "7", "-out", alone]) == 0 and open(alone).read() == open(out).read()
    ranker = RankerFactory().loadRankerFromFile(mf)
    want = Ranker.partialDependence2(ranker, FeatureManager.readInput(test), [(4, 1), (2, 5)], grid=5, ice=True)
    assert open(out2).read() == "".join(ln + "\n" for ln in P.table2_lines(want))
    assert open(ice2).read() == "".join(ln + "\n" for ln in P.ice2_lines(want))
    lines = [ln.split("\t") for ln in open(out2).read().splitlines()]
    cells = [r for r in lines if len(r) == 7]
    assert [r[:3] for r in lines if len(r) == 4] == [["2", "5", "h2"], ["4", "1", "h2"]] and len(cells) + 2 == len(lines)
    assert [(int(r[0]), int(r[1]), float(r[2]), float(r[3])) for r in cells] == sorted((int(r[0]), int(r[1]), float(r[2]), float(r[3])) for r in cells)
    assert len({r[4] for r in cells}) > 6 and any(float(r[6]) > 0 for r in cells)
