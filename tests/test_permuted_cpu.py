"""Permutation importance without a GPU: the restatements (tests/permuted_restatement.py) against a table derived by hand and
against each other -- so the path rule the kernel follows is pinned here --, the donor generator, the importance arithmetic and the
command line's ordering on a canned result, the refusals a machine without a device can reach, and the three entry points in the
header, the library and _native.ABI_SYMBOLS."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import permuted_restatement as PR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import importance as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, S = TM.L, TM.S


# ---- 1. by hand -------------------------------------------------------------------------------------------------------------------------
def test_a_table_derived_by_hand():
    # documents (x1, x2): d0 (0, 0), d1 (1, 0) | d2 (0, 1), d3 (1, 1); labels 1, 0 | 0, 1; every weight 1.
    #   T1  x1 <= 0.5 ? 1 : 2          T2  x2 <= 0.5 ? 0 : 4          T3  x1 <= 0.5 ? (x2 <= 0.5 ? 0.25 : 0.5) : 8
    # base         d0 1 + 0 + 0.25 = 1.25   d1 2 + 0 + 8 = 10   d2 1 + 4 + 0.5 = 5.5   d3 2 + 4 + 8 = 14
    # donor 3, 2, 1, 0.  Column 1: x1 becomes 1, 0, 1, 0 -> d0 is (1, 0) = 10, d1 (0, 0) = 1.25, d2 (1, 1) = 14, d3 (0, 1) = 5.5
    #                    Column 2: x2 becomes 1, 1, 0, 0 -> d0 is (0, 1) = 5.5, d1 (1, 1) = 14, d2 (0, 0) = 1.25, d3 (1, 0) = 10
    trees = [TM.flatten(S(1, 0.5, L(1.0), L(2.0))), TM.flatten(S(2, 0.5, L(0.0), L(4.0))),
             TM.flatten(S(1, 0.5, S(2, 0.5, L(0.25), L(0.5)), L(8.0)))]
    w = np.ones(3, np.float32)
    rows = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1]], np.float32)
    lab, qoff, donor = np.array([1, 0, 0, 1], np.float32), [0, 2, 4], np.array([[3, 2, 1, 0]])
    for fn in (PR.permuted_scores, PR.permuted_scores_path_rule):
        base, sc = fn(trees, w, rows, [1, 2], donor)
        assert base.tolist() == [1.25, 10.0, 5.5, 14.0]
        assert sc.tolist() == [[[10.0, 1.25, 14.0, 5.5]], [[5.5, 14.0, 1.25, 10.0]]]
    # P@1: base ranks d1 first (label 0) and d3 first (label 1); column 1 turns both lists round, column 2 leaves both orders
    bv, bn, v, nan, _ = PR.eval_permuted(trees, w, rows, lab, qoff, "P", 1, [1, 2], donor)
    assert bv.tolist() == [0.0, 1.0] and v.tolist() == [[[1.0, 0.0]], [[0.0, 1.0]]] and not bn.any() and not nan.any()
    # NDCG@2: the relevant document second is (2^1 - 1) / log2(3) over an ideal DCG of 1
    second = 1.0 / (math.log(3) / math.log(2))
    bv, _, v, _, ideal = PR.eval_permuted(trees, w, rows, lab, qoff, "NDCG", 2, [1, 2], donor)
    assert bv.tolist() == [second, 1.0] and v.tolist() == [[[1.0, second]], [[second, 1.0]]] and ideal.tolist() == [1.0, 1.0]
    res = I.summarize([1, 2], bv, v)
    assert res.base_mean == (second + 1.0) / 2 and res.importance.tolist() == [0.0, 0.0]       # the lists trade places: the file's mean stays


# ---- 2. the two restatements ------------------------------------------------------------------------------------------------------------
def test_the_path_rule_equals_the_materialised_matrix_on_the_main_data():
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    base2, sc2 = PR.permuted_scores_path_rule(trees, w, rows, PR.COLUMNS, donor)
    assert np.array_equal(PR.bits32(base2), PR.bits32(base)) and np.array_equal(PR.bits32(sc2), PR.bits32(sc))


def test_the_main_data_tells_the_columns_apart():
    """a kernel that returned the base everywhere cannot pass the GPU tests: every used column changes at least half of the scores (58 %
    to 84 % of them) and the NDCG@10 of at least 10 of the 12 lists; columns 0 (no tree tests it) and 13 (the row stride) change nothing"""
    trees, w, rows, lab, qoff, donor, base, sc = PR.main_data()
    changed = (PR.bits32(sc) != PR.bits32(base)[None, None, :]).mean(axis=2)
    assert not changed[0].any() and not changed[13].any()
    assert (changed[1:13] >= 0.5).all(), changed
    assert changed[1:13, 0].min() >= 0.58 and changed[1:13, 0].max() <= 0.84, changed[:, 0]     # the first repeat: RandomState(1)
    bv, _, v, nan, _ = PR.eval_permuted(trees, w, rows, lab, qoff, "NDCG", 10, PR.COLUMNS, donor, scores=(base, sc))
    assert not nan.any()
    for c in range(1, 13):
        assert (PR.bits64(v[c, 0]) != PR.bits64(bv)).sum() >= 10, c


def test_the_path_rule_equals_the_materialised_matrix_on_the_trap_trees():
    trees, w = PR.trap_trees()
    rng = np.random.default_rng(8)
    rows = PR.trap_rows(rng, 300)
    donor = np.stack([rng.permutation(300), np.full(300, 7), np.arange(300)])
    a = PR.permuted_scores(trees, w, rows, [3, 5, 2, 7, 1], donor)
    b = PR.permuted_scores_path_rule(trees, w, rows, [3, 5, 2, 7, 1], donor)
    assert TM.same_scores(b[1].ravel(), a[1].ravel()) is None
    assert TM.same_scores(a[1][:, 2].ravel(), np.tile(a[0], 5)) is None                         # the identity donor: every cell is the base
    assert (PR.bits32(a[1][0, 0]) != PR.bits32(a[0])).mean() > 0.5


def test_substituting_only_at_the_first_node_would_be_wrong():
    # x3 <= 0 ? (x3 <= -1 ? 1 : 2) : 3.  Document (x3 = 0.5) with the donated -2: the root goes left AND the node below must see -2 too (1);
    # with its own 0.5 there it would reach 2.
    trees, w = [TM.flatten(S(3, 0.0, S(3, -1.0, L(1.0), L(2.0)), L(3.0)))], np.ones(1, np.float32)
    rows = np.zeros((2, 4), np.float32)
    rows[:, 3] = [0.5, -2.0]
    for fn in (PR.permuted_scores, PR.permuted_scores_path_rule):
        base, sc = fn(trees, w, rows, [3], [[1, 0]])
        assert base.tolist() == [3.0, 1.0] and sc.tolist() == [[[1.0, 3.0]]]


# ---- 3. the donor generator -------------------------------------------------------------------------------------------------------------
def test_donor_maps():
    sizes = [3, 0, 5, 1, 40]
    n = sum(sizes)
    d = I.donor_maps(sizes, 4, seed=1)
    assert d.shape == (4, n) and d.dtype == np.int32
    for r in range(4):
        assert sorted(d[r].tolist()) == list(range(n))
        assert np.array_equal(d[r], np.random.RandomState(1 + r).permutation(n))
    assert np.array_equal(I.donor_maps(sizes, 2, seed=2)[0], d[1])
    win = I.donor_maps(sizes, 4, seed=1, within=True)
    off = np.concatenate([[0], np.cumsum(sizes)])
    moved = 0
    for r in range(4):
        rs = np.random.RandomState(1 + r)
        for q, s in enumerate(sizes):
            part = win[r, off[q]:off[q + 1]]
            assert sorted(part.tolist()) == list(range(off[q], off[q + 1]))                        # every donor stays in its own list
            assert np.array_equal(part, off[q] + rs.permutation(s))
            moved += int((part != np.arange(off[q], off[q + 1])).sum())
    assert moved > 100
    with pytest.raises(N.RankLibError, match="-repeat"):
        I.donor_maps(sizes, 0)


# ---- 4. the arithmetic and the ordering -------------------------------------------------------------------------------------------------
def test_importance_arithmetic_and_table_order():
    base = [0.5, 0.25, 0.75]
    values = np.array([[[0.5, 0.25, 0.75], [0.5, 0.25, 0.75]],          # feature 7: nothing moves
                       [[0.25, 0.25, 0.25], [0.5, 0.0, 0.25]],          # feature 2
                       [[0.5, 0.25, 0.75], [0.5, 0.25, 0.75]],          # feature 4 ties with 7
                       [[1.0, 0.25, 0.75], [0.5, 0.75, 0.75]]])         # feature 9: better without it
    res = I.summarize([7, 2, 4, 9], base, values)
    bm = (0.5 + 0.25 + 0.75) / 3
    assert res.base_mean == bm
    assert res.repeat_means.tolist() == [[bm, bm], [0.75 / 3, 0.75 / 3], [bm, bm], [2.0 / 3, 2.0 / 3]]
    assert res.importance.tolist() == [0.0, bm - 0.25, 0.0, bm - 2.0 / 3] and res.std.tolist() == [0.0, 0.0, 0.0, 0.0]
    two = I.summarize([1], [1.0], [[[0.5], [0.0]]])                      # repeat means 0.5 and 0.0: mean 0.25, population std 0.25
    assert two.importance.tolist() == [0.75] and two.std.tolist() == [0.25]
    lines = I.table_lines(res)
    assert [ln.split("\t")[0] for ln in lines] == ["2", "4", "7", "9"]   # descending importance, the tie by ascending id
    assert lines[0] == "2\t0.25\t0.0\t0.5\t0.25\t0.25" and lines[1] == "4\t0.0\t0.0\t0.5\t0.5\t0.5"
    assert lines[3].split("\t")[1] == "-0.16666666666666663"            # Double.toString


# ---- 5. refusals and symbols ------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return N.lib()


def test_the_refusals_that_need_no_device():
    """the model is looked at after the other arguments, so a null model reaches every argument check"""
    lib = _lib()
    rows = np.zeros((4, 3), np.float32)
    cols, don = np.array([1, 2], np.int32), np.array([[3, 2, 1, 0]], np.int32)
    out, base = np.zeros((2, 1, 4), np.float32), np.zeros(4, np.float32)
    args = dict(m=None, X=rows.ctypes.data, n=4, stride=3, cols=cols.ctypes.data, nc=2, don=don.ctypes.data, nr=1, base=base.ctypes.data,
                out=out.ctypes.data)

    def pr(**kw):
        a = dict(args, **kw)
        rc = lib.rl_model_predict_permuted(a["m"], a["X"], a["n"], a["stride"], a["cols"], a["nc"], a["don"], a["nr"], a["base"], a["out"])
        return rc, lib.rl_last_error().decode()

    neg, far, low = np.array([1, -2], np.int32), np.array([[3, 2, 4, 0]], np.int32), np.array([[3, -1, 1, 0]], np.int32)
    for kw, text in ((dict(), "null model"), (dict(X=None), "null X"), (dict(cols=None), "null columns"), (dict(don=None), "null donor"),
                     (dict(out=None), "null output"), (dict(n=-1), "n_docs must be >= 0"), (dict(stride=0), "row_stride must be >= 1"),
                     (dict(nc=0), "n_columns must be >= 1"), (dict(nr=0), "n_repeats must be >= 1"),
                     (dict(cols=neg.ctypes.data), "columns[1] = -2 is negative"), (dict(don=far.ctypes.data), "donor[0][2] = 4 is outside [0, 4)"),
                     (dict(don=low.ctypes.data), "donor[0][1] = -1 is outside [0, 4)")):
        rc, msg = pr(**kw)
        assert rc == -1 and msg == "rl_model_predict_permuted: " + text, (kw, rc, msg)
    lab, qoff = np.zeros(4, np.float32), np.array([0, 2, 4], np.int32)
    ov, on, bv, bn = np.zeros((2, 1, 2)), np.zeros((2, 1, 2), np.uint8), np.zeros(2), np.zeros(2, np.uint8)
    eargs = dict(args, lab=lab.ctypes.data, qoff=qoff.ctypes.data, nl=2, metric=0, k=10, scratch=0, bv=bv.ctypes.data, bn=bn.ctypes.data,
                 ov=ov.ctypes.data, on=on.ctypes.data)

    def ev(**kw):
        a = dict(eargs, **kw)
        rc = lib.rl_model_eval_permuted(a["m"], a["X"], a["n"], a["stride"], a["lab"], a["qoff"], a["nl"], None, None, None, a["metric"], a["k"],
                                        16.0, a["cols"], a["nc"], a["don"], a["nr"], a["scratch"], a["bv"], a["bn"], a["ov"], a["on"], None)
        return rc, lib.rl_last_error().decode()

    for kw, text in ((dict(), "null model"), (dict(X=None), "null X"), (dict(cols=None), "null columns"), (dict(don=None), "null donor"),
                     (dict(ov=None), "null output"), (dict(nc=-3), "n_columns must be >= 1"), (dict(nr=-1), "n_repeats must be >= 1"),
                     (dict(cols=neg.ctypes.data), "columns[1] = -2 is negative"), (dict(don=far.ctypes.data), "donor[0][2] = 4 is outside [0, 4)"),
                     (dict(stride=-1), "row_stride must be >= 1")):
        rc, msg = ev(**kw)
        assert rc == -1 and msg == "rl_model_eval_permuted: " + text, (kw, rc, msg)
    with pytest.raises(N.RankLibError, match="rl_debug_permuted_times: null argument"):
        N.check(lib.rl_debug_permuted_times(None, None))
    assert N.permuted_times() == (0.0, 0.0) or min(N.permuted_times()) >= 0.0


def test_the_three_entry_points_are_declared_exported_and_named():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = C.CDLL(_lib()._name)
    for n in ("rl_model_predict_permuted", "rl_model_eval_permuted", "rl_debug_permuted_times"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in N.ABI_SYMBOLS
    assert lib.rl_abi_version() == 5 and re.search(r"#define RLHIP_ABI_VERSION 5\b", hdr)          # as the staged entry points: no bump
    assert re.search(r"#define RL_PERMUTED_BATCH %d\b" % N.PERMUTED_BATCH, hdr)
    assert re.search(r"RL_MODEL_PATH_PERMUTED = %d\b" % N.MODEL_PATH_PERMUTED, hdr)
