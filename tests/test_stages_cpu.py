"""Staged evaluation without a GPU: the restatement (tests/stages_restatement.py) against hand-derived stage tables, the -step stage
lists, truncated()'s text, the refusals for models without stages, and the three entry points in the header, the library and
_native.ABI_SYMBOLS."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import stages_restatement as SR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import learning, stages
from ranklib_amd.learning import RankerFactory, truncate_model_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, S = TM.L, TM.S


def rows_of(x):
    r = np.zeros((len(x), 2), np.float32)
    r[:, 1] = x
    return r


def test_a_tie_is_broken_by_the_given_order():
    # stage 1: scores [1, 2] -> document 1 first, ranked labels [0, 1].  Stage 2: [2, 2], a tie -> the given order, ranked labels [1, 0].
    trees = [TM.flatten(S(1, 0.5, L(1.0), L(2.0))), TM.flatten(S(1, 0.5, L(1.0), L(0.0)))]
    w = np.array([1.0, 1.0], np.float32)
    rows, lab, qoff = rows_of([0.0, 1.0]), np.array([1, 0], np.float32), [0, 2]
    assert SR.stage_scores(trees, w, rows, [1, 2]).tolist() == [[1.0, 2.0], [2.0, 2.0]]
    for metric, k, want in (("P", 1, [0.0, 1.0]), ("RR", 2, [0.5, 1.0]), ("DCG", 2, [1.0 / (math.log(3) / math.log(2)), 1.0]),
                            ("BEST", 1, [0.0, 1.0]), ("MAP", 0, [0.5, 1.0])):
        v, nan, _ = SR.eval_stages(trees, w, rows, lab, qoff, metric, k, [1, 2])
        assert v[:, 0].tolist() == want and not nan.any(), metric


def test_negative_zero_ties_with_zero():
    # -Float.MIN_VALUE * 0.25 rounds to -0.0f: scores [-0.0, +0.0].  They tie, so the relevant document 0 stays first (by their bits
    # +0.0 would pass it).  Tree 2 keeps the -0.0 (-0.0 + -0.0) and lifts document 1 to 1.0.
    trees = [TM.flatten(S(1, 0.5, L(-TM.F32_MIN), L(0.0))), TM.flatten(S(1, 0.5, L(-0.0), L(4.0)))]
    w = np.array([0.25, 0.25], np.float32)
    rows, lab, qoff = rows_of([0.0, 1.0]), np.array([1, 0], np.float32), [0, 2]
    sc = SR.stage_scores(trees, w, rows, [1, 2])
    assert sc.view(np.uint32).tolist() == [[0x80000000, 0], [0x80000000, 0x3f800000]]
    v, nan, _ = SR.eval_stages(trees, w, rows, lab, qoff, "P", 1, [1, 2])
    assert v[:, 0].tolist() == [1.0, 0.0] and not nan.any()


def test_a_nan_from_stage_2_on_is_flagged_in_its_list_only():
    # two lists of two documents; tree 2 gives NaN to x > 0.5, which only list 0 holds
    trees = [TM.flatten(S(1, 0.5, L(1.0), L(2.0))), TM.flatten(S(1, 0.5, L(0.5), L(np.nan))), TM.flatten(L(1.0))]
    w = np.ones(3, np.float32)
    rows, lab, qoff = rows_of([0.0, 1.0, 0.0, 0.25]), np.array([1, 0, 0, 1], np.float32), [0, 2, 4]
    v, nan, _ = SR.eval_stages(trees, w, rows, lab, qoff, "RR", 2, [1, 2, 3])
    assert nan.tolist() == [[0, 0], [1, 0], [1, 0]]
    assert v.tolist() == [[0.5, 0.5], [0.0, 0.5], [0.0, 0.5]]
    v, nan, _ = SR.eval_stages(trees, w, rows, lab, qoff, "RR", 2, [3])
    assert nan.tolist() == [[1, 0]] and v.tolist() == [[0.0, 0.5]]


@pytest.mark.parametrize("T, n, want", [(5, 1, [1, 2, 3, 4, 5]), (5, 5, [5]), (5, 9, [5]), (7, 3, [3, 6, 7]), (37, 7, [7, 14, 21, 28, 35, 37]),
                                        (1, 1, [1])])
def test_step_stage_lists(T, n, want):
    assert stages.stage_list(T, n) == want


def test_step_below_one_is_refused():
    with pytest.raises(N.RankLibError, match="-step"):
        stages.stage_list(5, 0)


def test_pick_is_the_earliest_highest_mean():
    assert stages.pick_stage([0.1, 0.3, 0.3, 0.2]) == 1 and stages.pick_stage([0.5]) == 0 and stages.pick_stage([0.2, 0.1, 0.4]) == 2
    assert stages.file_means([[0.1, 0.2, 0.3], [1.0, 0.0, 0.0]]) == [(0.1 + 0.2 + 0.3) / 3, 1.0 / 3]


TWO = ("## LambdaMART\n## No. of trees = 2\n## No. of leaves = 10\n## No. of threshold candidates = 256\n## Learning rate = 0.1\n## Stop early = 100\n"
       "\n<ensemble>\n"
       "\t<tree id=\"1\" weight=\"0.1\">\n\t\t<split>\n\t\t\t<output>1.5 </output>\n\t\t</split>\n\t</tree>\n"
       "\t<tree id=\"2\" weight=\"0.5\">\n\t\t<split>\n\t\t\t<output>-2.0 </output>\n\t\t</split>\n\t</tree>\n"
       "</ensemble>\n")


def test_truncated_text_of_a_two_tree_model():
    assert TM.model_text([TM.flatten(L(1.5)), TM.flatten(L(-2.0))], np.array([0.1, 0.5], np.float32)) == TWO
    head = ("## LambdaMART\n## No. of trees = 2\n## No. of leaves = 10\n## No. of threshold candidates = 256\n## Learning rate = 0.1\n"
            "## Stop early = 100\n")
    one = "\t<tree id=\"1\" weight=\"0.1\">\n\t\t<split>\n\t\t\t<output>1.5 </output>\n\t\t</split>\n\t</tree>\n"
    two = "\t<tree id=\"2\" weight=\"0.5\">\n\t\t<split>\n\t\t\t<output>-2.0 </output>\n\t\t</split>\n\t</tree>\n"
    assert truncate_model_text(TWO, 1) == head + "## rlhip: first 1 of 2 trees\n\n<ensemble>\n" + one + "</ensemble>\n"
    assert truncate_model_text(TWO, 2) == head + "## rlhip: first 2 of 2 trees\n\n<ensemble>\n" + one + two + "</ensemble>\n"


@pytest.mark.parametrize("t", [0, 3, -1, 1.0, None, True])
def test_truncated_out_of_range(t):
    with pytest.raises(N.RankLibError, match="truncated"):
        truncate_model_text(TWO, t)


class _NoDeviceModel:
    """stands where _native.Model stands while a tree model's text is loaded on a machine without a GPU"""

    def __init__(self, text, device=0):
        self.text = text

    def features(self):
        return np.array([1], np.int32)


FOREST = "## Random Forests\n## No. of bags = 1\n\n" + TWO.split("\n\n", 1)[1]
LINEAR = "## Coordinate Ascent\n## Restart = 5\n## MaxIteration = 25\n## StepBase = 0.05\n## StepScale = 2.0\n## Tolerance = 0.001\n## Regularized = false\n## Slack = 0.001\n1:0.5 2:0.5\n"


@pytest.mark.parametrize("text, name", [(FOREST, "Random Forests"), (LINEAR, "Coordinate Ascent")])
def test_models_without_stages_refuse(text, name, monkeypatch):
    monkeypatch.setattr(learning.N, "Model", _NoDeviceModel)
    r = RankerFactory().loadRankerFromString(text)
    assert r.name() == name
    with pytest.raises(N.RankLibError, match="stagedScores.*%s" % name):
        r.stagedScores([], None)
    with pytest.raises(N.RankLibError, match="truncated.*%s" % name):
        r.truncated(1)


def test_the_three_entry_points_are_declared_exported_and_named():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    names = ("rl_model_predict_stages", "rl_model_eval_stages", "rl_debug_stage_times")
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(N.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in N.ABI_SYMBOLS
    assert lib.rl_abi_version() == 5 and re.search(r"#define RLHIP_ABI_VERSION 5\b", hdr)
