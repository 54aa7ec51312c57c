"""Two-feature partial dependence without a GPU: the restatements (tests/partial2_restatement.py) against a table written out
by hand and against each other -- so the rectangle descent the kernel follows is pinned here, with its stack bound --, the condition that
keeps a kernel that substitutes one column or none from passing the GPU tests, the host side of a call (rl_partial2_host.h) through
tools/partial2_host_check.cpp, the refusals a machine without a device reaches, h2, and the generic path of Ranker.partialDependence2."""
import os
import re
import subprocess

import numpy as np
import pytest

import partial2_restatement as P2
import partial_restatement as PD
import permuted_restatement as PR
import tree_models as TM
import walk_cases as WC
from ranklib_amd import _native as N
from ranklib_amd import partial as P
from test_partial_cpu import FakeLinear, _lib, lists_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, S = TM.L, TM.S
INF = np.float32(np.inf)
TA, TB = N.PARTIAL2_TILE_A, N.PARTIAL2_TILE_B
TRAP_GRID = np.array([-INF, -1, -0.5, 0, 0.25, 0.5, 1, INF], np.float32)


# ---- 1. by hand -------------------------------------------------------------------------------------------------------------------------
def hand_model():
    # documents (x1, x2, x3): d0 (0, 0, 0), d1 (1, 0, 1), d2 (-1, 1, 0), d3 (0, 1, 1); every weight 1; a = x1, b = x2.
    #   T1  x1 <= 0.5 ? 1 : 2        T2  x2 <= 0.5 ? 0 : 4        T3  x1 <= 0.5 ? (x2 <= 0.5 ? (x1 <= -0.5 ? 0.25 : 0.5) : 8) : 16
    #   T4  x3 <= 0.5 ? 0 : 32       (another column: the document's own value)
    trees = [TM.flatten(S(1, 0.5, L(1.0), L(2.0))), TM.flatten(S(2, 0.5, L(0.0), L(4.0))),
             TM.flatten(S(1, 0.5, S(2, 0.5, S(1, -0.5, L(0.25), L(0.5)), L(8.0)), L(16.0))), TM.flatten(S(3, 0.5, L(0.0), L(32.0)))]
    rows = np.array([[0, 0, 0, 0], [0, 1, 0, 1], [0, -1, 1, 0], [0, 0, 1, 1]], np.float32)
    return trees, np.ones(4, np.float32), rows


def test_a_table_written_out_by_hand():
    # base      d0 1 + 0 + 0.5 + 0 = 1.5      d1 2 + 0 + 16 + 32 = 50      d2 1 + 4 + 8 + 0 = 13      d3 1 + 4 + 8 + 32 = 45
    # T1 + T2 + T3 of a cell, the same for every document; T4 adds 0, 32, 0, 32:
    #   x1 = -1:  x2 = 0, 0.5: 1 + 0 + 0.25 = 1.25     x2 = 1: 1 + 4 + 8 = 13
    #   x1 =  0:  x2 = 0, 0.5: 1 + 0 + 0.5  = 1.5      x2 = 1: 13
    #   x1 =  1:  x2 = 0, 0.5: 2 + 0 + 16   = 18       x2 = 1: 2 + 4 + 16 = 22
    trees, w, rows = hand_model()
    grids = [(np.array([-1, 0, 1], np.float32), np.array([0, 0.5, 1], np.float32))]
    f = [1.25, 1.25, 13.0, 1.5, 1.5, 13.0, 18.0, 18.0, 22.0]
    want = [[v, v + 32, v, v + 32] for v in f]
    base, sc = P2.partial2_scores(trees, w, rows, [(1, 2)], grids)
    assert base.tolist() == [1.5, 50.0, 13.0, 45.0] and sc.tolist() == want
    for ta, tb in ((1, 1), (2, 2), (3, 3), (8, 8)):
        got, deepest = P2.partial2_scores_descent(trees, w, rows, [(1, 2)], grids, ta, tb)
        assert got.tolist() == want and deepest <= max(0, min(ta, 3) + min(tb, 3) - 2)
    got, _ = P2.partial2_scores_descent(trees, w, rows, [(2, 1)], [grids[0][::-1]], 3, 3)      # (b, a): the transposed surface
    assert got.reshape(3, 3, 4).transpose(1, 0, 2).reshape(9, 4).tolist() == want
    mean, shift2 = PD.reduce_cells(base, sc)
    assert mean.tolist() == [v + 16 for v in f]
    # cell (0, 0): scores 1.25, 33.25, 1.25, 33.25; the moves -0.25, -16.75, -11.75, -11.75
    assert shift2[0] == (0.0625 + 280.5625 + 138.0625 + 138.0625) / 4


# ---- 2. the two restatements, the stack bound and the condition on the pairs ------------------------------------------------------------------
def test_the_descent_equals_the_materialised_matrix_on_the_main_data():
    trees, w, rows = PR.main_data()[:3]
    pairs, grids, base, sc, _, _ = P2.main_partial2()
    assert sc.shape == (270, len(rows)) and np.array_equal(PD.bits32(base), PD.bits32(PD.main_partial()[0]))
    at = np.arange(0, len(rows), 47)                          # (a plain Python loop per document: every 47th)
    for ta, tb in ((TA, TB), (4, 3)):
        got, deepest = P2.partial2_scores_descent(trees, w, rows[at], pairs, grids, ta, tb)
        assert np.array_equal(PD.bits32(got), PD.bits32(sc[:, at]))
        assert 1 <= deepest <= ta + tb - 2                    # the pending stack's bound, whatever the depth


def test_a_kernel_that_substitutes_one_column_or_none_cannot_pass():
    """for every pair of the GPU tests, in at least a quarter of its cells some score differs in bits from the base, and in at least a
    quarter some score differs from BOTH one-column substitutions (a alone at u, b alone at v).  The least shares over the three
    pairs are asserted below and stated in DESIGN.md 35.5."""
    trees, w, rows = PR.main_data()[:3]
    pairs, grids, base, sc, _, shift2 = P2.main_partial2()
    both = P2.together(trees)
    least_base, least_both = 1.0, 1.0
    for p, ((a, b), (ga, gb)) in enumerate(zip(pairs, grids)):
        assert len(both[(min(a, b), max(a, b))]) >= 2 and (len(ga), len(gb)) == (9, 10)
        cells = PD.bits32(sc[90 * p:90 * p + 90]).reshape(9, 10, -1)
        one_a = PD.bits32(PD.partial_scores(trees, w, rows, [a], [ga])[1])[:, None, :]
        one_b = PD.bits32(PD.partial_scores(trees, w, rows, [b], [gb])[1])[None, :, :]
        least_base = min(least_base, (cells != PD.bits32(base)).any(axis=2).mean())
        least_both = min(least_both, ((cells != one_a) & (cells != one_b)).any(axis=2).mean())
    assert least_base >= 0.25 and least_both >= 0.25, (least_base, least_both)
    assert least_base == 1.0 and least_both == 1.0, (least_base, least_both)
    assert (shift2 > 0).all()


@pytest.mark.parametrize("name", ["trap", "dup_path", "thresholds_deep"])
def test_the_descent_equals_the_materialised_matrix_on_the_trap_trees(name):
    if name == "trap":
        (trees, w), rows, pairs = PR.trap_trees(), PR.trap_rows(np.random.default_rng(8), 60), [(3, 5), (5, 3), (3, 7), (2, 13)]
        grids = [(TRAP_GRID, TRAP_GRID)] * 4
    else:
        trees, w = WC.trees_of(name)
        rows = WC.rows(name)[:40]
        cols = WC.cell_columns(name)
        pairs = [(cols[0], cols[1]), (cols[2], cols[0])]
        grid_of = dict(zip(cols, WC.cell_grids(name)))
        grids = [(grid_of[a][:9], grid_of[b][-9:]) for a, b in pairs]
    want = P2.partial2_scores(trees, w, rows, pairs, grids)[1]
    got, deepest = P2.partial2_scores_descent(trees, w, rows, pairs, grids, TA, TB)
    assert TM.same_scores(got.ravel(), want.ravel()) is None and deepest <= TA + TB - 2


# ---- 3. the host side of a call ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("partial2_host")
    exe, model = str(d / "partial2_host_check"), str(d / "model.txt")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "partial2_host_check.cpp"),
                           os.path.join(ROOT, "ranklib_amd", "csrc", "rl_model.cpp"), "-o", exe])
    trees, w = PR.trap_trees()
    with open(model, "w", encoding="ascii") as f:
        f.write(TM.model_text(trees, w))
    return exe, model, trees


def run_plan(exe, model, ta, tb, chunk, pairs, grids):
    fmt = lambda v: "inf" if v == np.inf else "-inf" if v == -np.inf else "nan" if v != v else repr(float(v))      # noqa: E731
    axis = lambda c, g: "%d:%s" % (c, ",".join(fmt(v) for v in g))      # noqa: E731
    args = [axis(a, ga) + "/" + axis(b, gb) for (a, b), (ga, gb) in zip(pairs, grids)]
    return subprocess.check_output([exe, model, str(ta), str(tb), str(chunk)] + args, text=True).splitlines()


def plan_lines(trees, pairs, grids, chunk, ta, tb):
    base, chunks = P2.plan(trees, pairs, grids, chunk, ta, tb)
    tile = lambda t: "tile %d %d %d %d %d %d %d %d %s %s" % (t[:8] + (",".join("%08x" % PD.bits32([v])[0] for v in t[8]), t[9]))      # noqa: E731
    out = ["rc 0 ", "plan %d %d %d %d %d %d" % (sum(len(ga) * len(gb) for ga, gb in grids), chunk, ta, tb, len(trees), len(chunks)), tile(base)]
    first = 1
    for ci, ts in enumerate(chunks):
        out.append("chunk %d %d %d %d" % (ci, first, len(ts), sum(t[4] * t[5] for t in ts)))
        first += len(ts)
        out += [tile(t) for t in ts]
    return out


@pytest.mark.parametrize("ta, tb, chunk", [(8, 8, 1000), (4, 4, 1000), (4, 4, 20), (3, 2, 7), (4, 4, 5), (8, 8, 1)])
def test_the_plan_of_the_host_header(host_check, ta, tb, chunk):
    """tiles never straddle a pair, an edge tile is padded with its last value on either axis, uses is exact per pair -- column 3 is tested
    by six of the nine trap trees, 5 by three, 7 by one, 9 and 40 by none --, a chunk ends before a tile it cannot hold, and only a chunk
    smaller than a tile cuts the tiles"""
    exe, model, trees = host_check
    pairs = [(5, 3), (3, 9), (5, 3), (40, 9), (7, 5)]          # a repeated pair, an axis no tree tests, a pair no tree tests
    grids = [(TRAP_GRID, TRAP_GRID[:5]), ([0.0], TRAP_GRID[1:6]), (np.array([-0.0], np.float32), [1.0]), ([TM.F32_MAX, np.inf], [0.5, 1.0, 2.0]),
             (TRAP_GRID[1:7], TRAP_GRID[:7])]
    got = run_plan(exe, model, ta, tb, chunk, pairs, grids)
    assert got == plan_lines(trees, pairs, grids, chunk, ta, tb)
    tiles = [ln.split(" ") for ln in got if ln.startswith("tile ")]
    assert tiles[0][1:9] == ["-1", "-1", "-1", "0", "1", "1", "-1", "1"] and set(tiles[0][10]) == {"0"} and sum(t[1] == "-1" for t in tiles) == 1
    cells = []
    for t in tiles[1:]:
        ca, cb, cell, gb = int(t[5]), int(t[6]), int(t[7]), int(t[8])
        vals = t[9].split(",")
        assert 1 <= ca <= ta and 1 <= cb <= tb and len(vals) == ta + tb and gb == len(grids[int(t[3])][1])
        assert all(v == vals[ca - 1] for v in vals[ca:ta]) and all(v == vals[ta + cb - 1] for v in vals[ta + cb:])      # the padding repeats the last value
        assert (int(t[1]), int(t[2])) == pairs[int(t[3])] and t[10] == P2.uses(trees, int(t[1]), int(t[2]))
        cells += [cell + u * gb + v for u in range(ca) for v in range(cb)]
    total = sum(len(ga) * len(gb) for ga, gb in grids)
    assert sorted(cells) == list(range(total))                 # every cell once
    assert {(t[1], t[2]): t[10].count("1") for t in tiles[1:]} == {("5", "3"): 6, ("3", "9"): 6, ("40", "9"): 0, ("7", "5"): 4}      # (3's six hold 5's three)
    per_chunk = [int(ln.split(" ")[4]) for ln in got if ln.startswith("chunk ")]
    assert sum(per_chunk) == total and max(per_chunk) <= chunk and min(per_chunk) >= 1
    if chunk >= ta * tb:                                       # a chunk that can hold a whole tile never cuts one
        assert len(tiles) == 1 + sum(-(-len(ga) // ta) * -(-len(gb) // tb) for ga, gb in grids)


def test_the_host_check_refuses_by_message(host_check):
    exe, model, _ = host_check
    run = lambda pairs, grids: run_plan(exe, model, 4, 4, 50, pairs, grids)      # noqa: E731
    assert run([(3, 5), (4, 4)], [([0.0], [1.0])] * 2) == ["rc -1 who: pairs[1] = (4, 4) names one column twice"]
    assert run([(3, -5)], [([0.0], [1.0])]) == ["rc -1 who: pairs[0] = (3, -5) has a negative column"]
    assert run([(3, 5)], [([0.0], [2.0, 2.0])]) == ["rc -1 who: grid[1][1] = 2 is not greater than its predecessor 2: a grid ascends strictly"]
    assert run([(3, 5)], [([0.0, np.nan], [2.0])]) == ["rc -1 who: grid[0][1] = nan is NaN"]


# ---- 4. refusals and symbols ------------------------------------------------------------------------------------------------------------
def test_the_refusals_that_need_no_device():
    """the model is looked at after the other arguments, so a null model reaches every argument check"""
    lib = _lib()
    rows = np.zeros((4, 3), np.float32)
    i32, f32 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.float32))
    prs, off, grid = i32(1, 2, 2, 1), i32(0, 2, 3, 4, 6), f32(0, 1, -np.inf, 0, 0, np.inf)
    mean, shift2 = np.zeros(6), np.zeros(6)
    args = dict(m=None, X=rows.ctypes.data, n=4, stride=3, prs=prs.ctypes.data, np_=2, off=off.ctypes.data, grid=grid.ctypes.data, scratch=0,
                mean=mean.ctypes.data, shift2=shift2.ctypes.data)

    def pp(**kw):
        a = dict(args, **kw)
        rc = lib.rl_model_predict_partial2(a["m"], a["X"], a["n"], a["stride"], a["prs"], a["np_"], a["off"], a["grid"], a["scratch"], None,
                                           a["mean"], a["shift2"], None)
        return rc, lib.rl_last_error().decode()

    same, neg, off1, empty = i32(1, 2, 2, 2), i32(1, 2, -1, 2), i32(1, 2, 3, 4, 6), i32(0, 2, 3, 3, 6)
    nan, fall = f32(0, 1, -np.inf, 0, np.nan, 1), f32(0, 1, -np.inf, 0, 1, 0.5)
    for kw, text in ((dict(), "null model"), (dict(X=None), "null X"), (dict(prs=None), "null pairs"), (dict(off=None), "null grid_off"),
                     (dict(grid=None), "null grid"), (dict(mean=None), "null out_mean"), (dict(shift2=None), "null out_shift2"),
                     (dict(n=0), "n_docs must be >= 1"), (dict(stride=0), "row_stride must be >= 1"), (dict(np_=0), "n_pairs must be >= 1"),
                     (dict(prs=same.ctypes.data), "pairs[1] = (2, 2) names one column twice"),
                     (dict(prs=neg.ctypes.data), "pairs[1] = (-1, 2) has a negative column"),
                     (dict(off=off1.ctypes.data), "grid_off[0] = 1 must be 0"),
                     (dict(off=empty.ctypes.data), "grid_off[3] = 3 is not greater than grid_off[2] = 3: a grid is empty or grid_off descends"),
                     (dict(grid=nan.ctypes.data), "grid[3][0] = nan is NaN"),
                     (dict(grid=fall.ctypes.data), "grid[3][1] = 0.5 is not greater than its predecessor 1: a grid ascends strictly"),
                     (dict(scratch=-1), "scratch_bytes must be >= 0")):
        rc, msg = pp(**kw)
        assert rc == -1 and msg == "rl_model_predict_partial2: " + text, (kw, rc, msg)
    rc, msg = pp(n=(1 << 31))
    assert rc == -4 and msg == "rl_model_predict_partial2: more than 2^31 documents per call"
    wide = np.array([0, 50000, 100000], np.int32)              # 50 000 x 50 000 cells; the grid itself is checked first, so it is real
    big = np.tile(np.arange(50000, dtype=np.float32), 2)
    rc, msg = pp(np_=1, off=wide.ctypes.data, grid=big.ctypes.data)
    assert rc == -4 and msg == "rl_model_predict_partial2: more than 2^31 cells per call", (rc, msg)
    with pytest.raises(N.RankLibError, match="rl_debug_partial2_times: null argument"):
        N.check(lib.rl_debug_partial2_times(None, None))
    assert min(N.partial2_times()) >= 0.0
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    assert re.search(r"RL_MODEL_PATH_PARTIAL2 = %d\b" % N.MODEL_PATH_PARTIAL2, hdr) and N.MODEL_PATH_PARTIAL2 == 10 and lib.rl_abi_version() == 5
    assert re.search(r"#ifndef RL_PARTIAL2_TILE_A\n#define RL_PARTIAL2_TILE_A %d\b" % TA, hdr) and re.search(r"#define RL_PARTIAL2_TILE_B %d\b" % TB, hdr)


# ---- 5. h2 and the generic path on a ranker that needs no device -----------------------------------------------------------------------------
class FakeTrees(FakeLinear):
    """a tree model on the host: tree_models.eval_ensemble_np row by row, an unknown feature reading 0"""

    def __init__(self, trees):
        super().__init__()
        self.trees, self.features = trees, [1, 2]

    def eval(self, dp):               # noqa: A003
        row = np.nan_to_num(np.asarray(dp.fVals, np.float32), nan=0.0)[None, :]
        return float(TM.eval_ensemble_np(self.trees, np.ones(len(self.trees), np.float32), np.pad(row, ((0, 0), (0, 4))))[0])


def test_h2_of_an_additive_model_and_of_one_tree_on_both_columns():
    rows = np.zeros((64, 3), np.float32)
    rows[:, 1], rows[:, 2] = np.arange(64) % 8, np.arange(64) // 8
    samples = lists_of(rows, [10, 54])
    additive = FakeTrees([TM.flatten(S(1, 3.0, L(1.0), L(2.0))), TM.flatten(S(2, 2.0, L(0.5), L(4.0))), TM.flatten(S(1, 5.0, L(0.0), L(0.25)))])
    res = additive.partialDependence2(samples, [(1, 2)], grid=8)
    assert res.h2 == [0.0] and res.mean[0].shape == (8, 8) and len({m for m in res.mean[0].ravel()}) == 6
    joint = FakeTrees([TM.flatten(S(1, 3.0, L(1.0), S(2, 2.0, L(0.5), L(4.0))))])
    res = joint.partialDependence2(samples, [(1, 2), (2, 1)], grid=8, ice=True)
    assert res.h2[0] > 0.01 and res.h2[0] == res.h2[1] and np.array_equal(res.mean[0], res.mean[1].T) and res.ice[0].shape == (8, 8, 64)
    assert P.h2_on_grid(np.zeros((2, 2)), np.zeros(2), np.zeros(2)) == 0.0      # a flat surface: the denominator is 0
    lines = P.table2_lines(res)
    assert len(lines) == 2 * 64 + 2 and lines[0].split("\t")[:4] == ["1", "2", "0.0", "0.0"] and lines[64].split("\t")[:4] == ["2", "1", "0.0", "0.0"]
    assert lines[-2].split("\t")[:3] == ["1", "2", "h2"] and float(lines[-1].split("\t")[3]) == res.h2[1]


def test_the_generic_path():
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 5, (300, 4)).astype(np.float32)     # features 1 .. 3, each 0 .. 4
    samples = lists_of(rows, [1, 0, 99, 200])
    res = FakeLinear().partialDependence2(samples, [(3, 1)], grid=3, ice=True)
    assert res.pairs == [(3, 1)] and [g.tolist() for g in res.grids[0]] == [[0.0, 2.0, 4.0]] * 2 and res.h2 == [0.0]
    base = 2.0 * rows[:, 1].astype(np.float64) - rows[:, 3].astype(np.float64)
    assert np.array_equal(res.base, base)
    for u, v3 in enumerate([0.0, 2.0, 4.0]):
        for v, v1 in enumerate([0.0, 2.0, 4.0]):
            assert (res.ice[0][u, v] == 2.0 * v1 - v3).all() and res.mean[0][u, v] == 2.0 * v1 - v3
            s2 = PD.fixed_sums(np.full(300, 2.0 * v1 - v3, np.float32), base)[1]
            assert res.rms[0][u, v] == np.sqrt(s2 / 300) and res.centred[0][u, v] == res.mean[0][u, v] - res.base_mean
    for bad, text in (([(1, 1)], "two different features"), ([(0, 1)], "feature ids >= 1"), ([], "no pair to vary")):
        with pytest.raises(N.RankLibError, match=text):
            FakeLinear().partialDependence2(samples, bad)
