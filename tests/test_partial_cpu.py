"""Partial dependence without a GPU: the restatements (tests/partial_restatement.py) against a table derived by hand and
against each other -- so the path rule the kernel follows is pinned here --, the fixed order of the sums on a probe that tells 256 from
every other block width, the grids, the generic path of Ranker.partialDependence on a ranker that needs no device, the refusals a
machine without a device can reach, the two entry points in the header, the library and _native.ABI_SYMBOLS, and the host side of the
call (rl_partial_host.h) through tools/partial_host_check.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import partial_restatement as PD
import permuted_restatement as PR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import partial as P
from ranklib_amd.learning import DataPoint, LambdaMART, Ranker, RankList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, S = TM.L, TM.S
INF = np.float32(np.inf)
TRAP_GRID = np.array([-INF, -1, -0.5, 0, 0.25, 0.5, 1, INF], np.float32)


# ---- 1. by hand -------------------------------------------------------------------------------------------------------------------------
def hand_model():
    # documents (x1, x2): d0 (0, 0), d1 (1, 0), d2 (-1, 1), d3 (0, 1); every weight 1.
    #   T1  x1 <= 0.5 ? 1 : 2      T2  x2 <= 0.5 ? 0 : 4      T3  x1 <= 0.5 ? (x1 <= -0.5 ? 0.25 : 0.5) : 8      (T3 tests x1 twice)
    trees = [TM.flatten(S(1, 0.5, L(1.0), L(2.0))), TM.flatten(S(2, 0.5, L(0.0), L(4.0))),
             TM.flatten(S(1, 0.5, S(1, -0.5, L(0.25), L(0.5)), L(8.0)))]
    rows = np.array([[0, 0, 0], [0, 1, 0], [0, -1, 1], [0, 0, 1]], np.float32)
    return trees, np.ones(3, np.float32), rows


def test_a_table_derived_by_hand():
    # base          d0 1 + 0 + 0.5 = 1.5     d1 2 + 0 + 8 = 10     d2 1 + 4 + 0.25 = 5.25     d3 1 + 4 + 0.5 = 5.5
    # x1 = -1       T1 1, T3 0.25, T2 the document's own:   1.25  1.25  5.25  5.25     mean 13 / 4
    # x1 =  0       T1 1, T3 0.5:                           1.5   1.5   5.5   5.5      mean 14 / 4
    # x1 =  1       T1 2, T3 8:                             10    10    14    14       mean 48 / 4
    # x2 =  0, 0.5  T2 0 (0.5 <= 0.5 goes left):            1.5   10    1.25  1.5      mean 14.25 / 4
    # x2 =  1       T2 4:                                   5.5   14    5.25  5.5      mean 30.25 / 4
    trees, w, rows = hand_model()
    grids = [np.array([-1, 0, 1], np.float32), np.array([0, 0.5, 1], np.float32)]
    for fn in (PD.partial_scores, PD.partial_scores_path_rule):
        base, sc = fn(trees, w, rows, [1, 2], grids)
        assert base.tolist() == [1.5, 10.0, 5.25, 5.5]
        assert sc.tolist() == [[1.25, 1.25, 5.25, 5.25], [1.5, 1.5, 5.5, 5.5], [10.0, 10.0, 14.0, 14.0],
                               [1.5, 10.0, 1.25, 1.5], [1.5, 10.0, 1.25, 1.5], [5.5, 14.0, 5.25, 5.5]]
    mean, shift2 = PD.reduce_cells(base, sc)
    assert mean.tolist() == [3.25, 3.5, 12.0, 3.5625, 3.5625, 7.5625]
    # the moves: x1 = -1 (-0.25, -8.75, 0, -0.25); x1 = 0 (0, -8.5, 0.25, 0); x1 = 1 (8.5, 0, 8.75, 8.5); x2 <= 0.5 (0, 0, -4, -4); x2 = 1 (4, 4, 0, 0)
    assert shift2.tolist() == [76.6875 / 4, 72.3125 / 4, 221.0625 / 4, 8.0, 8.0, 8.0]
    res = P.summarize([1, 2], grids, base, [mean[:3], mean[3:]], [shift2[:3], shift2[3:]])
    assert res.base_mean == 22.25 / 4 and res.centred[0].tolist() == [3.25 - 5.5625, 3.5 - 5.5625, 12.0 - 5.5625]
    assert res.rms[1].tolist() == [np.sqrt(8.0)] * 3
    assert P.table_lines(res)[1] == "1\t0.0\t3.5\t-2.0625\t4.251837837923738" and P.table_lines(res)[5] == "2\t1.0\t7.5625\t2.0\t2.8284271247461903"
    assert float(P.table_lines(res)[1].split("\t")[4]) == np.sqrt(18.078125)                  # Double.toString round-trips
    assert [ln.split("\t")[:2] for ln in P.table_lines(res)] == [["1", "-1.0"], ["1", "0.0"], ["1", "1.0"], ["2", "0.0"], ["2", "0.5"], ["2", "1.0"]]


def test_a_column_beyond_the_rows_is_substituted_all_the_same():
    """the rows count as padded with zeros to any width: a tree on column 5 sees the grid value although the rows are 3 wide"""
    trees, w, rows = hand_model()
    trees = trees + [TM.flatten(S(5, 0.0, L(16.0), L(32.0)))]
    w = np.ones(4, np.float32)
    for fn in (PD.partial_scores, PD.partial_scores_path_rule):
        base, sc = fn(trees, w, rows, [5], [np.array([0.0, 1.0], np.float32)])
        assert base.tolist() == [17.5, 26.0, 21.25, 21.5] and sc.tolist() == [[17.5, 26.0, 21.25, 21.5], [33.5, 42.0, 37.25, 37.5]]


# ---- 2. the two restatements ------------------------------------------------------------------------------------------------------------
def test_the_path_rule_equals_the_materialised_matrix_on_the_main_data():
    trees, w, rows = PR.main_data()[:3]
    base, sc, _, _ = PD.main_partial()
    base2, sc2 = PD.partial_scores_path_rule(trees, w, rows, PR.COLUMNS, PD.main_grids())
    assert np.array_equal(PD.bits32(base2), PD.bits32(base)) and np.array_equal(PD.bits32(sc2), PD.bits32(sc))
    assert np.array_equal(PD.bits32(base), PD.bits32(PR.main_data()[6]))


def test_the_main_data_tells_the_cells_apart():
    """a kernel that returned the base everywhere cannot pass the GPU tests: in every cell of the columns 1 .. 12 at least a quarter of
    the scores differ in bits from the base (the least share over the 152 cells is 0.43); columns 0 (no tree tests it) and 13 (no tree
    tests it, and it lies at the row stride) have no thresholds and a two-value grid whose cells equal the base"""
    base, sc, mean, shift2 = PD.main_partial()
    grids = PD.main_grids()
    sizes = [len(g) for g in grids]
    assert sizes[0] == 2 and sizes[13] == 2 and min(sizes[1:13]) >= 8 and max(sizes[1:13]) <= 17 and sum(sizes[1:13]) == 152
    share = (PD.bits32(sc) != PD.bits32(base)[None, :]).mean(axis=1)
    assert not share[:2].any() and not share[-2:].any()
    assert (share[2:-2] >= 0.25).all(), share
    assert 0.42 <= share[2:-2].min() <= 0.44, share[2:-2].min()
    assert not shift2[:2].any() and not shift2[-2:].any() and (shift2[2:-2] > 0).all()
    assert len(set(PD.bits64(mean[2:-2]).tolist())) > 100


def test_the_path_rule_equals_the_materialised_matrix_on_the_trap_trees():
    trees, w = PR.trap_trees()
    rows = PR.trap_rows(np.random.default_rng(8), 300)
    cols = [3, 5, 2, 7, 1, 13]
    a = PD.partial_scores(trees, w, rows, cols, [TRAP_GRID] * len(cols))
    b = PD.partial_scores_path_rule(trees, w, rows, cols, [TRAP_GRID] * len(cols))
    assert TM.same_scores(b[1].ravel(), a[1].ravel()) is None and TM.same_scores(b[0], a[0]) is None
    assert (PD.bits32(a[1][:8]) != PD.bits32(a[0])[None, :]).mean(axis=1).min() > 0.25          # every cell of column 3
    assert TM.same_scores(a[1][-8:].ravel(), np.tile(a[0], 8)) is None                          # column 13: untested


def test_substituting_only_at_the_first_node_would_be_wrong():
    # x3 <= 0 ? (x3 <= -1 ? 1 : 2) : 3.  A document with x3 = 0.5 under the grid value -2: the root goes left AND the node below must see -2
    # too (1); with its own 0.5 there it would reach 2.
    trees, w = [TM.flatten(S(3, 0.0, S(3, -1.0, L(1.0), L(2.0)), L(3.0)))], np.ones(1, np.float32)
    rows = np.zeros((2, 4), np.float32)
    rows[:, 3] = [0.5, -2.0]
    for fn in (PD.partial_scores, PD.partial_scores_path_rule):
        base, sc = fn(trees, w, rows, [3], [[-2.0, 0.5]])
        assert base.tolist() == [3.0, 1.0] and sc.tolist() == [[1.0, 1.0], [3.0, 3.0]]


# ---- 3. the fixed order -----------------------------------------------------------------------------------------------------------------
def test_the_order_probe():
    """document 0 scores 2^53, the 511 others 1.0.  Adding 1.0 to 2^53 changes nothing (the tie goes to even), so the first partial of
    256 documents is 2^53 and the second 256: S1 = 2^53 + 256 exactly, the mean 2^44 + 0.5.  One serial chain gives 2^53, blocks of 128
    give 2^53 + 384: the block width and the order are pinned."""
    trees, w = [TM.flatten(S(1, 0.5, L(2.0 ** 53), L(1.0)))], np.ones(1, np.float32)
    rows = np.ones((512, 3), np.float32)
    rows[0, 1] = 0.0
    base, sc = PD.partial_scores(trees, w, rows, [2], [[0.0]])
    assert base[0] == 2.0 ** 53 and (base[1:] == 1.0).all() and np.array_equal(sc[0], base)
    assert PD.fixed_sums(sc[0], base) == (2.0 ** 53 + 256, 0.0)
    assert PD.fixed_sums(sc[0], base, block=512)[0] == 2.0 ** 53 and PD.fixed_sums(sc[0], base, block=128)[0] == 2.0 ** 53 + 384
    mean, shift2 = PD.reduce_cells(base, sc)
    assert mean.tolist() == [2.0 ** 44 + 0.5] and shift2.tolist() == [0.0]
    assert P.fixed_order_sums(sc[0].astype(np.float64), base.astype(np.float64)) == (2.0 ** 53 + 256, 0.0)      # the NumPy statement of the generic path


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513, 1611])
def test_the_numpy_statement_of_the_order_equals_the_loop(n):
    rng = np.random.default_rng(n)
    ice = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 8, n)).astype(np.float32)
    base = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 8, n)).astype(np.float32)
    ice[0] = -0.0
    assert PD.bits64(P.fixed_order_sums(ice.astype(np.float64), base.astype(np.float64))).tolist() == PD.bits64(PD.fixed_sums(ice, base)).tolist()
    for special in (np.inf, np.nan):
        ice[n // 2] = base[n // 2] = special                # inf - inf: S2 is NaN, S1 the infinity
        a, b = P.fixed_order_sums(ice.astype(np.float64), base.astype(np.float64)), PD.fixed_sums(ice, base)
        assert np.isnan(a[1]) and np.isnan(b[1]) and (a[0] == b[0] or (np.isnan(a[0]) and np.isnan(b[0])))
    assert P.fixed_order_sums(np.array([-0.0]), np.array([-0.0])) == (0.0, 0.0)
    assert PD.bits64(P.fixed_order_sums(np.array([-0.0]), np.array([-0.0]))[0])[0] == 0          # from +0.0: never -0.0


# ---- 4. the grids -----------------------------------------------------------------------------------------------------------------------
def text_ranker(trees, w):
    r = LambdaMART.__new__(LambdaMART)                       # (the text only: no device)
    r._model_text = TM.model_text(trees, w)
    return r


def lists_of(rows, sizes):
    out, i = [], 0
    for q, s in enumerate(sizes):
        out.append(RankList([DataPoint.from_parsed(0.0, "q%d" % q, "", np.array(rows[i + k], np.float32)) for k in range(s)]))
        i += s
    return out


def test_grid_for_thresholds():
    trees, w = PR.trap_trees()
    r = text_ranker(trees, w)
    g3 = P.grid_for(r, [], 3, "thresholds")
    assert np.array_equal(PD.bits32(g3), PD.bits32(PD.thresholds_grid(trees, 3)))
    assert g3[0] == -np.inf and g3[-1] == np.inf and (np.diff(g3[1:-1]) > 0).all()           # Infinity is last: nothing beyond it
    assert not (PD.bits32(g3) == 0x80000000).any() and (PD.bits32(g3) == 0).any()             # -0.0 and 0.0 are thresholds of column 3: one 0.0
    g7 = P.grid_for(r, [], 7, "Thresholds")
    assert g7.tolist() == [0.25, float(np.nextafter(np.float32(0.25), INF))]                 # the whole curve: the value at and the value beyond
    top = text_ranker([TM.flatten(S(2, TM.F32_MAX, L(1.0), L(2.0)))], np.ones(1, np.float32))
    assert P.grid_for(top, [], 2, "thresholds").tolist() == [float(TM.F32_MAX)]              # nextafter is Infinity: not finite, left out
    for c in range(1, 13):
        assert np.array_equal(PD.bits32(P.grid_for(text_ranker(*PR.main_data()[:2]), [], c, "thresholds")), PD.bits32(PD.main_grids()[c]))
    with pytest.raises(N.RankLibError, match="no threshold on feature 9"):
        P.grid_for(r, [], 9, "thresholds")
    with pytest.raises(N.RankLibError, match="needs a tree model"):
        P.grid_for(FakeLinear(), [], 1, "thresholds")
    with pytest.raises(N.RankLibError, match="a count or 'thresholds'"):
        P.grid_for(r, [], 3, "quantiles")


def test_grid_for_order_statistics():
    rows = np.zeros((100, 4), np.float32)
    rows[:, 1] = np.arange(100) % 50                         # 50 distinct values, each twice
    rows[:, 2] = [-0.0, 0.0, 1.0, np.nan] * 25              # -0.0 folds into 0.0, NaN is no value
    rows[:, 3] = np.nan
    samples = lists_of(rows, [10, 0, 60, 30])
    g = P.grid_for(None, samples, 1, 20)
    assert g.dtype == np.float32 and g.tolist() == [float((j * 49) // 19) for j in range(20)] and g[0] == 0 and g[-1] == 49
    assert P.grid_for(None, samples, 1, 50).tolist() == list(range(50)) and P.grid_for(None, samples, 1, 80).tolist() == list(range(50))      # m <= n: all
    assert P.grid_for(None, samples, 1, 2).tolist() == [0.0, 49.0]
    g2 = P.grid_for(None, samples, 2, 20)
    assert g2.tolist() == [0.0, 1.0] and PD.bits32(g2)[0] == 0
    many = lists_of(np.repeat(np.arange(7, dtype=np.float32), 2).reshape(-1, 1) * np.ones((1, 2), np.float32), [14])
    assert P.grid_for(None, many, 1, 5).tolist() == [0.0, 1.0, 3.0, 4.0, 6.0]               # (j * 6) // 4
    assert P.grid_for(None, many, 1, 6).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 6.0]          # (j * 6) // 5: 0 1 2 3 4 6
    with pytest.raises(N.RankLibError, match="feature 3 has no value"):
        P.grid_for(None, samples, 3, 20)
    with pytest.raises(N.RankLibError, match="feature 9 has no value"):
        P.grid_for(None, samples, 9, 20)
    with pytest.raises(N.RankLibError, match="at least 1"):
        P.grid_for(None, samples, 1, 0)


# ---- 5. the generic path on a ranker that needs no device -------------------------------------------------------------------------------
class FakeLinear(Ranker):
    """2 x1 - x3, a missing or unknown feature reading 0"""

    def __init__(self):
        super().__init__(features=[1, 3])

    def eval(self, dp):               # noqa: A003
        v = lambda f: 0.0 if f >= len(dp.fVals) or np.isnan(dp.fVals[f]) else float(dp.fVals[f])      # noqa: E731
        return 2.0 * v(1) - v(3)

    def name(self):
        return "Fake"


def test_the_generic_path():
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 5, (300, 4)).astype(np.float32)     # features 1 .. 3, each 0 .. 4
    samples = lists_of(rows, [1, 0, 99, 200])
    res = FakeLinear().partialDependence(samples, grid=3, ice=True)
    assert res.features == [1, 3] and res.grids[0].tolist() == [0.0, 2.0, 4.0] and res.grids[1].tolist() == [0.0, 2.0, 4.0]
    base = 2.0 * rows[:, 1].astype(np.float64) - rows[:, 3].astype(np.float64)
    assert np.array_equal(res.base, base) and res.base_mean == PD.fixed_sums(base, base)[0] / 300
    for c, ice_of in enumerate((lambda v: 2.0 * v - rows[:, 3].astype(np.float64), lambda v: 2.0 * rows[:, 1].astype(np.float64) - v)):
        for g, v in enumerate([0.0, 2.0, 4.0]):
            ice = ice_of(v)                                  # (small integers: exact in f32, so the f32 loop of the restatement applies)
            s1, s2 = PD.fixed_sums(ice, base)
            assert np.array_equal(res.ice[c][g], ice) and res.mean[c][g] == s1 / 300 and res.centred[c][g] == s1 / 300 - res.base_mean
            assert res.rms[c][g] == np.sqrt(s2 / 300) and s2 > 0
    two = FakeLinear().partialDependence(samples, features=[3, 1], grid=3)
    assert two.ice is None and two.features == [1, 3] and np.array_equal(two.mean[1], res.mean[1])


def test_the_generic_path_substitutes_a_feature_beyond_the_documents():
    samples = lists_of(np.array([[0, 1.0], [0, 2.0]], np.float32), [2])
    r = FakeLinear()
    with pytest.raises(N.RankLibError, match="feature 3 has no value"):
        r.partialDependence(samples, grid=5)
    wide = lists_of(np.array([[0, 1.0, 0, 7.0]], np.float32), [1]) + samples      # one document has feature 3: a one-value grid, set in all three
    res = r.partialDependence(wide, features=[3], grid=5, ice=True)
    assert res.grids[0].tolist() == [7.0] and res.ice[0].tolist() == [[-5.0, -5.0, -3.0]] and res.base.tolist() == [-5.0, 2.0, 4.0]
    with pytest.raises(N.RankLibError, match="at least one document"):
        r.partialDependence([], grid=5)
    with pytest.raises(N.RankLibError, match="feature ids >= 1"):
        r.partialDependence(samples, features=[0], grid=5)


# ---- 6. refusals and symbols ------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return N.lib()


def test_the_refusals_that_need_no_device():
    """the model is looked at after the other arguments, so a null model reaches every argument check"""
    lib = _lib()
    rows = np.zeros((4, 3), np.float32)
    cols, off, grid = np.array([1, 2], np.int32), np.array([0, 2, 5], np.int32), np.array([0, 1, -np.inf, 0, np.inf], np.float32)
    mean, shift2 = np.zeros(5), np.zeros(5)
    args = dict(m=None, X=rows.ctypes.data, n=4, stride=3, cols=cols.ctypes.data, nc=2, off=off.ctypes.data, grid=grid.ctypes.data, scratch=0,
                mean=mean.ctypes.data, shift2=shift2.ctypes.data)

    def pp(**kw):
        a = dict(args, **kw)
        rc = lib.rl_model_predict_partial(a["m"], a["X"], a["n"], a["stride"], a["cols"], a["nc"], a["off"], a["grid"], a["scratch"], None,
                                          a["mean"], a["shift2"], None)
        return rc, lib.rl_last_error().decode()

    i32, f32 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.float32))
    neg, off1, empty, down = i32(1, -2), i32(1, 2, 5), i32(0, 2, 2), i32(0, 3, 2)
    nan, equal, fall, zeros = f32(0, 1, 0, np.nan, 2), f32(0, 1, 0, 1, 1), f32(0, 1, 0, 1, 0.5), f32(0, 1, -1, -0.0, 0.0)
    for kw, text in ((dict(), "null model"), (dict(X=None), "null X"), (dict(cols=None), "null columns"), (dict(off=None), "null grid_off"),
                     (dict(grid=None), "null grid"), (dict(mean=None), "null out_mean"), (dict(shift2=None), "null out_shift2"),
                     (dict(n=0), "n_docs must be >= 1"), (dict(n=-1), "n_docs must be >= 1"), (dict(stride=0), "row_stride must be >= 1"),
                     (dict(nc=0), "n_columns must be >= 1"), (dict(cols=neg.ctypes.data), "columns[1] = -2 is negative"),
                     (dict(off=off1.ctypes.data), "grid_off[0] = 1 must be 0"),
                     (dict(off=empty.ctypes.data), "grid_off[2] = 2 is not greater than grid_off[1] = 2: a column's grid is empty or grid_off descends"),
                     (dict(off=down.ctypes.data), "grid_off[2] = 2 is not greater than grid_off[1] = 3: a column's grid is empty or grid_off descends"),
                     (dict(grid=nan.ctypes.data), "grid[1][1] = nan is NaN"),
                     (dict(grid=equal.ctypes.data), "grid[1][2] = 1 is not greater than its predecessor 1: a column's grid ascends strictly"),
                     (dict(grid=fall.ctypes.data), "grid[1][2] = 0.5 is not greater than its predecessor 1: a column's grid ascends strictly"),
                     (dict(grid=zeros.ctypes.data), "grid[1][2] = 0 is not greater than its predecessor -0: a column's grid ascends strictly"),
                     (dict(scratch=-1), "scratch_bytes must be >= 0")):
        rc, msg = pp(**kw)
        assert rc == -1 and msg == "rl_model_predict_partial: " + text, (kw, rc, msg)
    rc, msg = pp(n=(1 << 31))
    assert rc == -4 and msg == "rl_model_predict_partial: more than 2^31 documents per call"
    with pytest.raises(N.RankLibError, match="rl_debug_partial_times: null argument"):
        N.check(lib.rl_debug_partial_times(None, None))
    assert min(N.partial_times()) >= 0.0


def test_the_two_entry_points_are_declared_exported_and_named():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = C.CDLL(_lib()._name)
    for n in ("rl_model_predict_partial", "rl_debug_partial_times"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in N.ABI_SYMBOLS
    assert lib.rl_abi_version() == 5 and re.search(r"#define RLHIP_ABI_VERSION 5\b", hdr)          # as the permuted entry points: no bump
    assert re.search(r"#ifndef RL_PARTIAL_BATCH\n#define RL_PARTIAL_BATCH %d\b" % N.PARTIAL_BATCH, hdr) and N.PARTIAL_BATCH == 16
    assert re.search(r"#ifndef RL_PARTIAL_SUM_BLOCK\n#define RL_PARTIAL_SUM_BLOCK %d\b" % N.PARTIAL_SUM_BLOCK, hdr) and N.PARTIAL_SUM_BLOCK == PD.SUM_BLOCK == 256
    assert re.search(r"RL_MODEL_PATH_PARTIAL = %d\b" % N.MODEL_PATH_PARTIAL, hdr) and N.MODEL_PATH_PARTIAL == 7


# ---- 7. the host side of a call ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("partial_host")
    exe, model = str(d / "partial_host_check"), str(d / "model.txt")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "partial_host_check.cpp"),
                           os.path.join(ROOT, "ranklib_amd", "csrc", "rl_model.cpp"), "-o", exe])
    trees, w = PR.trap_trees()
    with open(model, "w", encoding="ascii") as f:
        f.write(TM.model_text(trees, w))
    return exe, model, trees


def run_plan(exe, model, B, chunk, columns, grids):
    fmt = lambda v: "inf" if v == np.inf else "-inf" if v == -np.inf else "nan" if v != v else repr(float(v))      # noqa: E731
    args = ["%d:%s" % (c, ",".join(fmt(v) for v in g)) for c, g in zip(columns, grids)]
    return subprocess.check_output([exe, model, str(B), str(chunk)] + args, text=True).splitlines()


def plan_lines(trees, columns, grids, chunk, B):
    chunks = PD.plan(trees, columns, grids, chunk, B)
    out = ["rc 0 ", "plan %d %d %d %d %d" % (sum(len(g) for g in grids), chunk, B, len(trees), len(chunks))]
    first = cell0 = 0
    for ci, bs in enumerate(chunks):
        cells = sum(b[3] for b in bs if b[0] >= 0)
        out.append("chunk %d %d %d %d %d" % (ci, first, len(bs), cell0, cells))
        first, cell0 = first + len(bs), cell0 + cells
        out += ["batch %d %d %d %d %s %s" % (b[0], b[1], b[2], b[3], ",".join("%08x" % PD.bits32([v])[0] for v in b[4]), b[5]) for b in bs]
    return out


@pytest.mark.parametrize("B, chunk", [(16, 1000), (4, 1000), (4, 5), (4, 1), (3, 7), (1, 2)])
def test_the_plan_of_the_host_header(host_check, B, chunk):
    """batches never straddle a column, the last batch of a column (and of a chunk) is padded with its last value, uses is exact per
    column -- column 3 is tested by six of the nine trap trees, 5 by three, 7 by one, 9 and 40 by none --, chunks cut where they must"""
    exe, model, trees = host_check
    columns = [5, 3, 9, 3, 7, 40]                            # unsorted, 3 repeated, 9 and 40 untested
    grids = [TRAP_GRID, TRAP_GRID[:5], [0.0], np.array([-0.0], np.float32), TRAP_GRID[1:4], [TM.F32_MAX, np.inf]]
    got = run_plan(exe, model, B, chunk, columns, grids)
    assert got == plan_lines(trees, columns, grids, chunk, B)
    batches = [ln.split(" ") for ln in got if ln.startswith("batch ")]
    assert batches[0][1:5] == ["-1", "-1", "0", "1"] and set(batches[0][6]) == {"0"} and sum(b[1] == "-1" for b in batches) == 1      # the base: once, first
    cells = {}
    for b in batches[1:]:
        assert 1 <= int(b[4]) <= B and len(b[5].split(",")) == B and len(b[6]) == len(trees)
        vals = b[5].split(",")
        assert all(v == vals[int(b[4]) - 1] for v in vals[int(b[4]):])                       # the padding repeats the last value
        cells.setdefault(int(b[2]), []).extend(vals[:int(b[4])])
        assert b[6] == "".join("1" if (t["feature"] == int(b[1])).any() else "0" for t in trees)
    assert [cells[p] for p in range(len(columns))] == [["%08x" % PD.bits32([v])[0] for v in g] for g in grids]      # every cell once, in order
    assert {b[1]: b[6].count("1") for b in batches[1:]} == {"5": 3, "3": 6, "9": 0, "7": 1, "40": 0}
    per_chunk = [int(ln.split(" ")[5]) for ln in got if ln.startswith("chunk ")]
    total = sum(len(g) for g in grids)
    assert sum(per_chunk) == total and max(per_chunk) <= chunk and min(per_chunk) >= 1
    if chunk >= B:                                           # a chunk that can hold a whole batch never cuts one: no walk more than one chunk needs
        assert len(batches) == 1 + sum(-(-len(g) // B) for g in grids)
    else:                                                    # smaller chunks are filled to the last cell
        assert per_chunk == [min(chunk, total - c0) for c0 in range(0, total, chunk)]


def test_the_host_check_refuses_by_message(host_check):
    exe, model, _ = host_check
    assert run_plan(exe, model, 4, 5, [3, 5], [[0.0, 1.0], [2.0, 2.0]]) == ["rc -1 who: grid[1][1] = 2 is not greater than its predecessor 2: a column's grid ascends strictly"]
    assert run_plan(exe, model, 4, 5, [3, -5], [[0.0, 1.0], [2.0]]) == ["rc -1 who: columns[1] = -5 is negative"]
    assert run_plan(exe, model, 4, 5, [3], [[0.0, np.nan]]) == ["rc -1 who: grid[0][1] = nan is NaN"]
    assert run_plan(exe, model, 4, 5, [3], [[-0.0, 0.0]])[0].startswith("rc -1 who: grid[0][1] = 0 is not greater than its predecessor -0")
