"""-m gpu: the lambdas of P@k and RR@k branch by branch.  The data of tests/pr_cases.py puts chosen labels at chosen ranked positions (round 0
ranks in the file's order), so that every written case of the two swapChange matrices is reached in every compared round, in lists of every
length class of the lambda kernels and in one list only k_rank_huge can rank.  The comparison is tests/test_gpu_tree_pr.py's: lambdas, weights,
scores, trees, the float train metric of every round and the finish() figure against the literal restatement, as bit patterns.

Where the restatement's rounds are recorded, every round has to reach the cases named there, give a non-zero lambda to a quarter of the
documents and split.  Round 0 is checked once more against a direct evaluation that ranks nothing (pr_cases.direct_round0): a wrong swap
change and a wrong ranking fail differently."""
import functools

import numpy as np
import pytest

import pr_cases as C
import test_gpu_tree_pr as TP
from ranklib_amd import _native as N

pytestmark = pytest.mark.gpu

ARM = N.ARM
LEAVES = 6
DATA = {"enumerated": C.enumerated, "structured": C.structured, "huge": lambda k: C.huge()}
ROUNDS = {"enumerated": 3, "structured": 3, "huge": 2}


@functools.lru_cache(maxsize=None)
def reference(name, data_k, metric, k):
    """the restatement's rounds on DATA[name](data_k) for metric@k, recorded once"""
    train = DATA[name](data_k)
    X, lab, qoff = train
    cases = C.reached(metric, k, lab, qoff)
    if name == "enumerated":
        assert cases == C.reachable(metric, k)
    elif name == "structured":
        assert cases == C.NAMES[metric]
    # (huge: a handful of lists, which a trained model ranks out of some cases: what its rounds reach is not asserted)
    ref = TP._restatement("LAMBDAMART", metric, k, ROUNDS[name], LEAVES, 100, train, None, cases=None if name == "huge" else cases)
    lam, w = C.direct_round0(TP.SCORERS[metric](k), lab, qoff)
    assert np.array_equal(TP.bits(lam, np.int64), TP.bits(ref["rounds"][0]["lam"], np.int64)), (name, metric, k)
    assert np.array_equal(TP.bits(w, np.int64), TP.bits(ref["rounds"][0]["w"], np.int64)), (name, metric, k)
    return ref


def run(name, data_k, metric, k, monkeypatch, env=None):
    for knob, v in (env or {}).items():
        monkeypatch.setenv("RLHIP_" + knob, str(v))
    ref = reference(name, data_k, metric, k)
    g = N.Trainer(n_trees=ROUNDS[name], n_leaves=LEAVES, metric=metric, metric_k=k, ranker="LAMBDAMART", early_stop_rounds=100)
    g.set_train(*DATA[name](data_k))
    g.init()
    return TP.compare(g, ref, (name, data_k, metric, k, env))


def _unfused(arms, rounds):
    assert arms[ARM["LAM_UNFUSED"]] == rounds and arms[ARM["LAM_ON_MAIN"]] + arms[ARM["LAM_ON_SIDE"]] == 0, [int(arms[ARM[a]]) for a in ("LAM_UNFUSED", "LAM_ON_MAIN", "LAM_ON_SIDE")]


# ---- every label string of up to k + 2 documents -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "TINY_MIN", "LAMBDA_UNFUSED"])
@pytest.mark.parametrize("metric", ["P", "RR"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_label_string(k, metric, mode, monkeypatch):
    arms = run("enumerated", k, metric, k, monkeypatch, {} if mode == "default" else {mode: 1})
    if mode == "LAMBDA_UNFUSED":
        _unfused(arms, 3)
        return
    TP._fused_only(arms, 3)
    # (k = 4: 5 460 lists of at most 16 documents, past the 4 096 from which they are ranked by k_rank_tiny without the knob)
    assert (arms[ARM["RANK_TINY"]] > 0) == (mode == "TINY_MIN" or k == 4)


# ---- first / second at chosen positions of lists of every length class ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["P", "RR"])
@pytest.mark.parametrize("k", [10, 16, 17, 20])
def test_first_and_second_at_chosen_positions(k, metric, monkeypatch):
    arms = run("structured", k, metric, k, monkeypatch)
    if k <= 16:
        TP._fused_only(arms, 3)
        assert arms[ARM["LAM_ON_MAIN"]] + arms[ARM["LAM_ON_SIDE"]] == 4 * 3      # the four length classes hold lists
    else:                                                                # past kLambdaFusedMaxK
        _unfused(arms, 3)


# ---- a list past the block rank kernel's cap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,k", [("P", 10), ("RR", 10), ("RR", 20)])
def test_a_list_only_k_rank_huge_can_rank(metric, k, monkeypatch):
    """RR@20: unfused, so firstRank / secondRank of the list of 5 001 documents are read from the table k_rank_huge wrote"""
    arms = run("huge", 10, metric, k, monkeypatch)
    if k <= 16:
        TP._fused_only(arms, 2)
    else:
        _unfused(arms, 2)
    assert arms[ARM["RANK_HUGE"]] > 0 and arms[ARM["RANK_MIXED"]] > 0, TP._rank_arms(arms)


@pytest.mark.parametrize("k", [10, 20])
def test_a_huge_list_beside_split_rank_kernels(k, monkeypatch):
    arms = run("huge", 10, "RR", k, monkeypatch, {"RANK_SPLIT": 1})
    if k <= 16:
        TP._fused_only(arms, 2)
    else:
        _unfused(arms, 2)
    assert arms[ARM["RANK_WAVE_SHORT"]] > 0 and arms[ARM["RANK_BLOCK"]] > 0 and arms[ARM["RANK_HUGE"]] > 0 and arms[ARM["RANK_MIXED"]] == 0, TP._rank_arms(arms)
