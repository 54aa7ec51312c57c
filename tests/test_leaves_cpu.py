"""Leaf indices without a device (rl_model_predict_leaves): the names, the refusals that need no model, the reference's
leaf numbering on a hand-written tree, the command line's argument errors and the rankers that have no leaves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import leaves_reference as LR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import leaves as LV
from ranklib_amd import learning as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rl_model_leaf_counts", "rl_model_predict_leaves", "rl_debug_leaves_times")
L, S = TM.L, TM.S


def test_the_names_are_in_the_header_the_library_and_the_symbol_list():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = N.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in N.ABI_SYMBOLS
    assert re.search(r"RL_LEAVES_BY_ROW = 0, RL_LEAVES_BY_TREE = 1\b", hdr) and lib.rl_abi_version() == 5


def test_the_refusals_that_need_no_device(gpu_available):
    """the model is looked at after the arguments that need none, so a null model reaches every one of them"""
    lib = N.lib()
    rows, out = np.zeros((4, 3), np.float32), np.zeros(8, np.uint16)
    args = dict(X=rows.ctypes.data, n=4, stride=3, first=0, cnt=0, layout=0, out=out.ctypes.data)
    for kw, rc, text in ((dict(), -1, "null model"), (dict(X=None), -1, "null X"), (dict(out=None), -1, "null output"),
                         (dict(n=-1), -1, "n_docs must be >= 0"), (dict(n=1 << 31), -4, "more than 2^31 documents per call"),
                         (dict(stride=0), -1, "row_stride must be >= 1"), (dict(layout=2), -1, "layout = 2 is neither RL_LEAVES_BY_ROW nor RL_LEAVES_BY_TREE"),
                         (dict(first=-1), -1, "first_tree must be >= 0"), (dict(cnt=-1), -1, "n_trees must be >= 0")):
        a = dict(args, **kw)
        got = lib.rl_model_predict_leaves(None, a["X"], a["n"], a["stride"], a["first"], a["cnt"], a["layout"], a["out"])
        assert (got, lib.rl_last_error().decode()) == (rc, "rl_model_predict_leaves: " + text), kw
    assert lib.rl_model_leaf_counts(None, None, 0, None) == -1 and lib.rl_last_error().decode() == "rl_model_leaf_counts: null model"
    with pytest.raises(N.RankLibError, match="rl_debug_leaves_times: null argument"):
        N.check(lib.rl_debug_leaves_times(None))
    assert N.leaves_times() >= 0.0
    if not gpu_available:                                      # no handle without a device, so no leaves: nothing falls back to the host
        with pytest.raises(N.RankLibError, match="no CPU fallback"):
            N.Model(TM.model_text([TM.flatten(S(1, 0.5, L(1.0), L(2.0)))], np.ones(1, np.float32))).predict_leaves(rows)


def test_the_reference_numbers_leaves_in_pre_order_left_first():
    """nodes in pre-order: 0 S, 1 S, 2 leaf, 3 leaf, 4 S, 5 leaf, 6 S, 7 leaf, 8 leaf -- the leaves are 0 .. 4 from left to right"""
    t = TM.flatten(S(1, 0.5, S(2, 0.5, L(10.0), L(11.0)), S(3, 0.5, L(12.0), S(1, 2.0, L(13.0), L(14.0)))))
    assert LR.numbers(t).tolist() == [-1, -1, 0, 1, -1, 2, -1, 3, 4] and LR.counts([t, TM.flatten(L(1.0))]).tolist() == [5, 1]
    rows = [[0, 0, 0, 0], [0, 0.5, 1, 0], [0, 1, 0, 0.5], [0, 2, 0, 1], [0, 3, 0, 1], [0, np.nan, 0, np.nan], [0, 0.5]]
    got = [int(LR.leaves([t], np.array([r], np.float32))[0, 0]) for r in rows]
    assert got == [0, 1, 2, 3, 4, 4, 0]                         # NaN goes right at every node; the two-column row reads 0 in column 2
    assert t["output"][t["feature"] == -1][got].tolist() == [10.0, 11.0, 12.0, 13.0, 14.0, 14.0, 10.0]
    assert LV.column_bases([5, 1, 3]).tolist() == [1, 6, 7]
    dp = RL.DataPoint("2 qid:q7 1:0.5 # doc-3")
    assert LV.out_line(dp, np.array([4, 0], np.uint16)) == "q7\t# doc-3\t4\t0"
    assert LV.letor_line(dp, np.array([4, 0], np.uint16), LV.column_bases([5, 1])) == "2 qid:q7 5:1 6:1"


@pytest.mark.parametrize("argv,text", [
    (["-test", "f", "-out", "o"], "ranklib_amd.leaves takes exactly one -load model (got 0)"),
    (["-load", "a", "-load", "b", "-test", "f", "-out", "o"], "ranklib_amd.leaves takes exactly one -load model (got 2)"),
    (["-load", "a", "-out", "o"], "ranklib_amd.leaves takes exactly one -test file (got 0)"),
    (["-load", "a", "-test", "f"], "ranklib_amd.leaves needs -out tsv"),
    (["-load", "a", "-test", "f", "-out", "o", "-from", "-1"], "-from must be at least 0 (got -1)"),
    (["-load", "a", "-test", "f", "-out", "o", "-count", "0"], "-count must be at least 1 (got 0)"),
    (["-load", "a", "-test", "f", "-out", "o", "-from", "x"], "-from takes a number of trees (got x)"),
    (["-load", "a", "-test", "f", "-out"], "Missing value for -out"),
    (["-load", "a", "-test", "f", "-out", "o", "-gmax", "2"], "Unknown command-line parameter: -gmax")])
def test_the_command_line_refuses_by_message(argv, text):
    with pytest.raises(N.RankLibError) as e:
        LV.main(argv)
    assert str(e.value) == text
    assert LV.main([]) == 0                                    # the usage line


@pytest.mark.parametrize("cls,text", [
    (RL.RFRanker, RL.LEAVES_NOT_BAGS),
    (RL.CoorAscent, "rlhip: leaves needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"),
    (RL.LinearRegRank, "rlhip: leaves needs a LambdaMART or MART model: a Linear Regression model has no trees"),
    (RL.RankNet, "rlhip: leaves needs a LambdaMART or MART model: a RankNet model has no trees"),
    (RL.ListNet, "rlhip: leaves needs a LambdaMART or MART model: a ListNet model has no trees")])
def test_rankers_without_one_ensemble_of_trees_are_refused(cls, text):
    with pytest.raises(N.RankLibError) as e:
        cls().leaves([])
    assert str(e.value) == text and "\n" not in text and "Random Forests" in RL.LEAVES_NOT_BAGS
