"""P@k and RR@k as train metrics of the tree trainers, without a GPU: the transcribed scorers (tests/pr_restatement.py) on hand-derived
swap changes, their scores against the host scorers of ranklib_amd.metric, the metric ids of the Python side against include/rlhip.h,
LambdaMART.init reaching the library with them, and LambdaRank's refusal, which stays."""
import os
import re

import numpy as np
import pytest

from pr_restatement import P, RR
from ranklib_amd import _native as N
from ranklib_amd import learning, metric
from ranklib_amd._native import RankLibError
from ranklib_amd.learning import DataPoint, LambdaMART, LambdaRank, MART, RankerFactory, RankerType, RankList
from ranklib_amd.metric import MetricScorerFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix(n, entries):
    """the symmetric n x n matrix that holds `entries` {(i, j): value} and 0.0 elsewhere"""
    m = [[0.0] * n for _ in range(n)]
    for (i, j), v in entries.items():
        m[i][j] = m[j][i] = v
    return m


# ---- 1. known answers, derived by hand from the two Java files -----------------------------------------------------------------------------
def test_p_swap_change_known_answers():
    lab = [1.0, 0.0, 2.0, 0.5, 0.0, 3.0, 0.0, 1.0]
    assert P(10).swap_change(lab, "q") == _matrix(8, {})                # n <= k: size == n, no j >= size
    assert P(8).swap_change(lab, "q") == _matrix(8, {})
    u = float(np.float32(1.0) / np.float32(3.0))                        # ((float) 1) / 3, widened
    assert u != 1.0 / 3.0
    # size 3; binary relevances 1 0 1 | 1 0 1 0 1: rows 0 and 2 lose against the non-relevant columns 4 and 6, row 1 gains against 3, 5, 7
    want = {(0, 4): -u, (0, 6): -u, (2, 4): -u, (2, 6): -u, (1, 3): u, (1, 5): u, (1, 7): u}
    assert P(3).swap_change(lab, "q") == _matrix(8, want)
    # labels 2 and 1 differ, their binary relevances do not: change 0
    assert P(1).swap_change([2.0, 1.0, 0.0], "q") == _matrix(3, {(0, 2): -1.0})


def test_rr_swap_change_known_answers():
    # no relevant document in the top `size`: firstRank := size, rr = 0; rows 0 .. 2 against the relevant columns 3 and 5
    got = RR(3).swap_change([0.0, 0.0, 0.0, 2.0, 0.0, 1.0, 0.0, 0.0], "q")
    assert got == _matrix(8, {(0, 3): 1.0, (0, 5): 1.0, (1, 3): 0.5, (1, 5): 0.5, (2, 3): 1.0 / 3, (2, 5): 1.0 / 3})
    # secondRank == -1: size 4, firstRank 1, rr 0.5
    got = RR(4).swap_change([0.0, 2.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0], "q")
    want = {(1, 2): 1.0 / 3 - 0.5, (1, 3): 1.0 / 4 - 0.5,               # j < size, non-relevant: 1 / (j + 1) - rr
            (1, 4): -0.5, (1, 6): -0.5, (1, 7): -0.5,                   # j >= size, non-relevant: -rr (column 5 is relevant: untouched by this loop)
            (0, 1): 0.5, (0, 5): 0.5}                                   # rows above firstRank against the relevant columns from firstRank on
    assert got == _matrix(8, want)
    # j < secondRank, j >= secondRank and j >= size: size 6, firstRank 1, secondRank 3, rr 0.5
    got = RR(6).swap_change([0.0, 1.0, 0.0, 2.0, 0.0, 0.0, 3.0, 0.0], "q")
    want = {(1, 2): 1.0 / 3 - 0.5,                                      # j < secondRank
            (1, 4): 1.0 / 4 - 0.5, (1, 5): 1.0 / 4 - 0.5,               # secondRank <= j < size: 1 / (secondRank + 1) - rr
            (1, 7): 1.0 / 4 - 0.5,                                      # j >= size
            (0, 1): 0.5, (0, 3): 0.5, (0, 6): 0.5}
    assert got == _matrix(8, want)
    # a label 0.5 is relevant (> 0.0: it is secondRank) AND non-relevant ((int) 0.5 == 0): position 2 is written by the first loop, against
    # firstRank, and by the third, against row 0
    got = RR(5).swap_change([0.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0], "q")
    s = 1.0 / 3 - 0.5                                                   # secondRank == 2: every non-relevant j >= 2 takes 1 / (2 + 1) - rr
    want = {(1, 2): s, (1, 3): s, (1, 4): s, (1, 5): s, (1, 6): s, (1, 7): s, (0, 1): 0.5, (0, 2): 0.5}
    assert got == _matrix(8, want)
    # ... and past `size` as well: a 0.5 there takes a value from the second loop and from the third
    got = RR(2).swap_change([0.0, 3.0, 0.5, 0.0], "q")
    assert got == _matrix(4, {(1, 2): -0.5, (1, 3): -0.5, (0, 1): 0.5, (0, 2): 0.5})
    # plain RR has k = 0: size 0, nothing
    assert RR().k == 0 and RR().swap_change([1.0, 0.0], "q") == _matrix(2, {}) and RR().score([1.0, 0.0], "q") == 0.0


# ---- 2. score against the host scorers ------------------------------------------------------------------------------------------------------
def test_scores_equal_the_host_scorers_on_random_lists():
    rng = np.random.default_rng(11)
    f = MetricScorerFactory()
    for t in range(200):
        n = int(rng.integers(1, 31))
        lab = rng.integers(0, 5, n).astype(np.float64)
        lab[rng.random(n) < 0.15] = 0.5
        if t % 7 == 0:
            lab[: n // 2] = 0.0
        rl = RankList([DataPoint("%r qid:q 1:0" % float(v)) for v in lab])
        for k in (1, 3, 10):
            assert P(k).score(list(lab), "q") == f.createScorer("P@%d" % k).score(rl), (t, k)
            assert RR(k).score(list(lab), "q") == f.createScorer("RR@%d" % k).score(rl), (t, k)


# ---- 3. metric ids --------------------------------------------------------------------------------------------------------------------------
def test_metric_ids_of_the_tree_trainer_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bRL_METRIC_([A-Z]+) = (\d+)", hdr)}
    assert N.RL_METRIC["P"] == 4 == ids["P"] and N.RL_METRIC["RR"] == 5 == ids["RR"]
    assert N.RL_METRIC == {k: v for k, v in ids.items() if k != "BEST"}
    assert N.RL_CA_METRIC == N.RL_METRIC and N.RL_EVAL_METRIC == dict(N.RL_METRIC, BEST=6) and ids["BEST"] == 6
    assert "BEST" not in N.RL_METRIC


# ---- 4. LambdaMART.init reaches the library -------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


@pytest.mark.parametrize("cls,ranker", [(LambdaMART, "LAMBDAMART"), (MART, "MART")])
@pytest.mark.parametrize("name", ["P@5", "RR@5"])
def test_init_passes_the_metric_to_the_trainer(monkeypatch, cls, ranker, name):
    seen = {}

    def trainer(**kw):
        seen.update(kw)
        raise _Stop()
    monkeypatch.setattr(N, "Trainer", trainer)
    monkeypatch.setattr(N, "set_err_max", lambda v: None)
    dp = [DataPoint("1 qid:1 1:1 2:0"), DataPoint("0 qid:1 1:0 2:1")]
    r = cls([RankList(dp)], [1, 2], MetricScorerFactory().createScorer(name))
    with pytest.raises(_Stop):
        r.init()
    assert seen["metric"] == name.split("@")[0] and seen["metric_k"] == 5 and seen["ranker"] == ranker


def test_init_still_refuses_best(monkeypatch):
    monkeypatch.setattr(N, "Trainer", lambda **kw: pytest.fail("reached the library"))
    dp = [DataPoint("1 qid:1 1:1 2:0"), DataPoint("0 qid:1 1:0 2:1")]
    r = LambdaMART([RankList(dp)], [1, 2], MetricScorerFactory().createScorer("Best@3"))
    with pytest.raises(RankLibError) as e:
        r.init()
    assert "train metric must be one of NDCG, DCG, MAP, ERR, P, RR (got Best@3)" in str(e.value)


# ---- 5. LambdaRank keeps its four metrics ---------------------------------------------------------------------------------------------------
def test_lambdarank_still_refuses_both(monkeypatch):
    monkeypatch.setattr(LambdaRank, "lamseed", 3)
    assert LambdaRank._METRICS == ("NDCG", "DCG", "MAP", "ERR") == metric.TRAINABLE
    assert metric.TREE_TRAINABLE == metric.TRAINABLE + ("P", "RR")
    dp = [DataPoint("1 qid:1 1:1 2:0"), DataPoint("0 qid:1 1:0 2:1")]
    for name in ("P@10", "RR@10"):
        r = RankerFactory().createRanker(RankerType.LAMBDARANK, [RankList(dp)], [1, 2], MetricScorerFactory().createScorer(name))
        with pytest.raises(RankLibError) as e:
            r.init()
        assert "LambdaRank train metric must be one of NDCG, DCG, MAP, ERR (got %s)" % name in str(e.value)
    assert learning.LambdaMART is LambdaMART
