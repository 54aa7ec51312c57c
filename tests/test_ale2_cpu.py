"""Second-order accumulated local effects without a GPU: the refusals a machine without a device reaches, the names, the
host side of a call (rl_ale2_host.h) through tools/ale2_host_check.cpp on hand-made trees, the surface of summarize_ale2 against values
enumerated by hand, the three-level sums against the restatement's loop, the command line's usage errors."""
import os
import subprocess

import numpy as np
import pytest

import ale2_restatement as A2
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import partial as P
from ranklib_amd.learning import DataPoint, Ranker, RankList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_refusals_that_need_no_device_and_the_names():
    lib = N.lib()
    i32, f32 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.float32))
    wide = np.concatenate([np.arange(66), np.arange(65)]).astype(np.float32)      # 65 x 64 intervals: one row above the cap
    keep = [np.zeros((4, 3), np.float32), i32(1, 2), i32(0, 2, 5), f32(0, 1, -np.inf, 0, np.inf), np.zeros(2, np.int64), np.zeros(2)]
    args = dict(m=None, X=keep[0].ctypes.data, n=4, stride=3, pairs=keep[1].ctypes.data, np_=1, off=keep[2].ctypes.data, edges=keep[3].ctypes.data,
                scratch=0, count=keep[4].ctypes.data, total=keep[5].ctypes.data)
    cases = [(dict(), "null model"), (dict(X=None), "null X"), (dict(pairs=None), "null pairs"), (dict(off=None), "null edge_off"),
             (dict(edges=None), "null edges"), (dict(count=None), "null out_count"), (dict(total=None), "null out_sum"),
             (dict(n=0), "n_docs must be >= 1"), (dict(stride=0), "row_stride must be >= 1"), (dict(np_=0), "n_pairs must be >= 1"),
             (dict(pairs=i32(1, -2)), "pairs[0] = (1, -2) has a negative column"), (dict(pairs=i32(2, 2)), "pairs[0] = (2, 2) names one column twice"),
             (dict(off=i32(1, 2, 5)), "edge_off[0] = 1 must be 0"), (dict(off=i32(0, 1, 5)), "edge_off[1] - edge_off[0] = 1: a slice has 2 .. 256 edges"),
             (dict(off=i32(0, 2, 259)), "edge_off[2] - edge_off[1] = 257: a slice has 2 .. 256 edges"),
             (dict(edges=f32(0, 1, 0, np.nan, 2)), "edges[1][1] = nan is NaN"),
             (dict(edges=f32(0, 1, 0, 1, 1)), "edges[1][2] = 1 is not greater than its predecessor 1: a slice's edges ascend strictly"),
             (dict(edges=f32(0, 1, -1, -0.0, 0.0)), "edges[1][2] = 0 is not greater than its predecessor -0: a slice's edges ascend strictly"),
             (dict(off=i32(0, 66, 131), edges=wide), "pairs[0] has 65 x 64 = 4160 cells: a pair has at most 4096"),
             (dict(scratch=-1), "scratch_bytes must be >= 0"), (dict(n=1 << 31), "more than 2^31 documents per call")]
    for kw, text in cases:
        a = dict(args, **{k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
        rc = lib.rl_model_predict_ale2(a["m"], a["X"], a["n"], a["stride"], a["pairs"], a["np_"], a["off"], a["edges"], a["scratch"], None,
                                       a["count"], a["total"], None, None)
        assert rc == (-4 if "2^31" in text else -1) and lib.rl_last_error().decode() == "rl_model_predict_ale2: " + text, (kw, rc, lib.rl_last_error())
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    for name in ("rl_model_predict_ale2", "rl_debug_ale2_times"):
        assert name in N.ABI_SYMBOLS and hasattr(lib, name) and "int  %s(" % name in hdr
    assert "RL_MODEL_PATH_ALE2 = %d }" % N.MODEL_PATH_ALE2 in hdr and N.MODEL_PATH_ALE2 == 12 and lib.rl_abi_version() == 5
    assert all("#define RL_ALE2_%s %d\n" % kv in hdr for kv in (("BATCH", N.ALE2_BATCH), ("MAX_CELLS", N.ALE2_MAX_CELLS), ("SUM_SUPER", N.ALE2_SUM_SUPER)))


@pytest.mark.parametrize("scratch, chunk", [(0, 7), (1, 1), (4000 + 2 * 1000 * 12, 2), (4000 + 5 * 1000 * 12 + 11, 5)])
def test_the_plan_of_the_host_header(scratch, chunk, tmp_path):
    """chunks of `chunk` pairs cut into batches of 2; bit 2u of uses: a tree tests pair u's a, bit 2u + 1: its b.  Tree 0 tests 3 and 5,
    tree 1 only 5, tree 2 is a leaf, tree 3 tests 7"""
    S, L = TM.S, TM.L
    trees = [TM.flatten(t) for t in (S(3, 0.5, S(5, 0.0, L(1.0), L(2.0)), L(3.0)), S(5, 1.0, L(0.5), L(0.25)), L(9.0), S(7, 0.0, L(1.0), L(2.0)))]
    exe, model = str(tmp_path / "ale2_host_check"), str(tmp_path / "model.txt")
    open(model, "w", encoding="ascii").write(TM.model_text(trees, np.ones(4, np.float32)))
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "ale2_host_check.cpp"),
                           os.path.join(ROOT, "ranklib_amd", "csrc", "rl_model.cpp"), "-o", exe])
    pairs = [(3, 5, 10, 10), (5, 3, 4, 2), (3, 9, 1, 1), (9, 40, 64, 64), (7, 5, 3, 255), (3, 5, 10, 10), (5, 7, 2, 2)]
    got = subprocess.check_output([exe, model, "2", str(scratch), "1000", "0"] + ["%d:%d:%d:%d" % p for p in pairs], text=True).splitlines()
    bits = {(3, 5): ["3", "2", "0", "0"], (5, 3): ["3", "1", "0", "0"], (3, 9): ["1", "0", "0", "0"], (9, 40): ["0"] * 4, (7, 5): ["2", "2", "0", "1"],
            (5, 7): ["1", "1", "0", "2"]}                    # per tree, the pair as slot 0 of its batch
    want, nb, cells = [], 0, [ka * kb for _, _, ka, kb in pairs]
    for ci, p0 in enumerate(range(0, 7, chunk)):
        ps = pairs[p0:p0 + chunk]
        want.append("chunk %d %d %d %d %d" % (ci, p0, len(ps), nb, -(-len(ps) // 2)))
        for b0 in range(0, len(ps), 2):
            use = [int(x, 16) | (int(y, 16) << 2) for x, y in zip(bits[ps[b0][:2]], bits[ps[b0 + 1][:2]] if b0 + 1 < len(ps) else ["0"] * 4)]
            want.append("batch %d %s" % (nb, " ".join("%x" % u for u in use)))
            nb += 1
    assert got == ["plan %d %d %d 1 %d" % (sum(cells), chunk, -(-7 // chunk), max(sum(cells[p0:p0 + chunk]) for p0 in range(0, 7, chunk)))] + want


class Surface(Ranker):
    """g(x1) + h(x2) + c x1 x2 on x1, x2 in {0, 1}: with c == 0 additive, so every second difference is 0"""

    def __init__(self, c):
        super().__init__(features=[1, 2])
        self.c = c

    def eval(self, dp):               # noqa: A003
        return 3.0 * dp.fVals[1] - 5.0 * (dp.fVals[2] > 0.5) + self.c * dp.fVals[1] * dp.fVals[2]

    def name(self):
        return "Surface"


def test_the_surface_of_an_additive_model_is_zero_and_of_a_product_the_enumerated_value():
    # one cell [0, 1] x [0, 1] holds all 5 documents; with c = 2 every d = f(1,1) - f(0,1) - f(1,0) + f(0,0) = 2, so the local effect
    # is 2 and the accumulated surface [[0, 0], [0, 2]].  Either main effect is the step (0 + 2) / 2 = 1 across the one interval:
    # minus [0, 1] on either axis gives [[0, -1], [-1, 0]]; the mean of the cell's four corners is -1/2: [[.5, -.5], [-.5, .5]].
    x = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1], [0, 1, 1]], np.float32)
    samples = [RankList([DataPoint.from_parsed(0.0, "q%d" % (i // 3), "", r) for i, r in enumerate(x) if i // 3 == q]) for q in range(2)]
    flat = Surface(0.0).accumulatedEffects2(samples, [(1, 2)], intervals=1, local=True)
    assert flat.pairs == [(1, 2)] and flat.count[0].tolist() == [[5]] and not flat.ale[0].any() and not flat.effect[0].any() and flat.cell[0].tolist() == [0] * 5
    assert flat.corner[0].tolist() == [[0.0] * 5, [-5.0] * 5, [3.0] * 5, [-2.0] * 5]
    res = Surface(2.0).accumulatedEffects2(samples, [(1, 2), (2, 1)], intervals=1)
    assert res.effect[0].tolist() == [[2.0]] and res.ale[0].tolist() == res.ale[1].tolist() == [[0.5, -0.5], [-0.5, 0.5]] and res.centre == [-0.5, -0.5]
    assert P.ale2_lines(res) == ["1\t2\t0.0\t0.0\t0.5\t0.0\t0", "1\t2\t0.0\t1.0\t-0.5\t0.0\t0", "1\t2\t1.0\t0.0\t-0.5\t0.0\t0", "1\t2\t1.0\t1.0\t0.5\t2.0\t5"] + [
        ln.replace("1\t2", "2\t1", 1) for ln in P.ale2_lines(res)[:4]]
    # 2 x 2 cells, one of them empty: effects [[1, 0], [2, 4]] accumulate to [[0, 0, 0], [0, 1, 1], [0, 3, 7]]; a's main effect per row
    # (3 * .5 + 0) / 3 = .5 and (1 * 1 + 2 * 4) / 3 = 3, b's per column (3 * .5 + 1 * 2) / 4 = .875 and (0 + 2 * 2) / 2 = 2
    ale, effect, centre = P.ale2_surface([[3, 0], [1, 2]], [[3.0, 0.0], [2.0, 8.0]])
    surf = np.array([[0, 0, 0], [0, 1, 1], [0, 3, 7]]) - np.array([0, 0.5, 3.5])[:, None] - np.array([0, 0.875, 2.875])[None, :]
    want = (3 * surf[0:2, 0:2].sum() + 1 * surf[1:3, 0:2].sum() + 2 * surf[1:3, 1:3].sum()) / 4 / 6
    assert effect.tolist() == [[1.0, 0.0], [2.0, 4.0]] and centre == want and np.array_equal(ale, surf - want)
    with pytest.raises(N.RankLibError, match="-intervals2 must be 1 .. 64"):
        Surface(0.0).accumulatedEffects2(samples, [(1, 2)], intervals=65)


@pytest.mark.parametrize("n", [1, 257, 16384, 16384 + 257, 2 * 16384 + 1])
def test_the_sums_in_their_three_level_order(n):
    """the NumPy statement of the generic path equals the restatement's loop"""
    rng = np.random.default_rng(n)
    corner = (rng.standard_normal((4, n)) * 10.0 ** rng.integers(-3, 4, (4, n))).astype(np.float32)
    cell = rng.integers(-1, 5, n).astype(np.int32)
    c = corner.astype(np.float64)
    count, total = A2.cell_sums(cell, corner, 6)
    pc, pt = P.ale2_cell_sums((c[3] - c[1]) - (c[2] - c[0]), cell, 6)
    assert np.array_equal(pc, count) and np.array_equal(A2.bits64(pt), A2.bits64(total)) and count[5] == 0 and count.sum() == (cell >= 0).sum()


def test_command_line_usage_errors():
    for argv, text in ((["-intervals2", "5"], "-intervals2 and -local2 need -ale2 tsv"), (["-local2", "x"], "-intervals2 and -local2 need -ale2 tsv"),
                       (["-ale2", "x"], "-ale2 needs -pairs file"), (["-pairs", "p", "-ale2", "x", "-intervals2", "0"], "-intervals2 takes a count 1 .. 64"),
                       (["-pairs", "p", "-ale2", "x", "-intervals2", "65"], "-intervals2 takes a count 1 .. 64")):
        with pytest.raises(N.RankLibError, match=text):
            P.main(["-load", "no-model", "-test", "no-file"] + argv)
