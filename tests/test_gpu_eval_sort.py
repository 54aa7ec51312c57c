"""rl_eval_lists' sort classes (rl_eval_sort.inc) on the GPU against the flat restatement (tests/eval_lists_restatement.py): every edge of the
in-LDS and the multi-block class under every score and label pattern, metric and k, the class each list was ranked in
(rl_debug_eval_path), long and short lists in one call, metric.score_lists and one Evaluator flow.  The edges are read from the built
library inside the tests.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import eval_lists_restatement as ER
import tree_models as T
from ranklib_amd import _native as N
from ranklib_amd import metric as M
from ranklib_amd.evaluator import Evaluator
from ranklib_amd.learning import DataPoint, RankList, RankerType, stable_desc_order

pytestmark = pytest.mark.gpu

GROUPS = ("sort", "pow2", "lds", "two_tiles", "odd_runs", "three_passes")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def lengths_of(group):
    e = N.eval_classes()
    S, L, tile = e["block"], e["sort_lds"], e["tile"]
    p2 = 1 << S.bit_length()                                # the first power of two past S + 1: its neighbours lie inside (S, L]
    assert S + 1 < p2 - 1 and p2 + 1 <= L < 2 * tile - 1
    return {"sort": [S - 1, S, S + 1], "pow2": [p2 - 1, p2, p2 + 1], "lds": [L - 1, L, L + 1], "two_tiles": [2 * tile - 1, 2 * tile, 2 * tile + 1],
            "odd_runs": [3 * tile + 1], "three_passes": [5 * tile + 7]}[group]


def path_of(lens):
    """the lists of each class, as the lengths imply"""
    e = N.eval_classes()
    edges = [e[c] for c in N.EVAL_CLASSES[:4]]
    count = dict.fromkeys(N.EVAL_CLASSES, 0)
    for n in lens:
        count[N.EVAL_CLASSES[sum(n > v for v in edges)]] += 1
    return count


@functools.lru_cache(maxsize=None)
def group_file(group):
    """one file per group and its ranking by the restatement, made once"""
    sc, lab, qoff, what = ER.make_file(lengths_of(group), seed=len(group))
    _, pos, _ = ER.eval_lists(sc, lab, qoff, "DCG", 1, want_pos=True)
    for a in (sc, lab, qoff, pos):
        a.setflags(write=False)
    return sc, lab, qoff, what, pos


@pytest.mark.parametrize("metric", ER.METRICS)
@pytest.mark.parametrize("group", GROUPS)
def test_every_edge_of_the_sort_classes_pattern_metric_and_k(group, metric):
    sc, lab, qoff, what, pos = group_file(group)
    want_path = path_of(np.diff(qoff))
    for k in ER.ks_of(lengths_of(group)):
        got, gpos, gideal = N.eval_lists(sc, lab, qoff, metric, k, want_pos=True)
        assert N.eval_path() == want_path, (k, N.eval_path(), want_path)
        want, _, ideal = ER.eval_lists(sc, lab, qoff, metric, k, pos=pos)
        assert np.array_equal(gpos, pos), (metric, k, what[int(np.searchsorted(qoff, np.flatnonzero(gpos != pos)[0], "right")) - 1])
        bad = np.flatnonzero(bits(got) != bits(want))
        assert not bad.size, (metric, k, [what[q] for q in bad[:3]], got[bad[:3]], want[bad[:3]])
        assert np.array_equal(bits(gideal), bits(ideal))
    for q, (n, sp, _) in enumerate(what):
        if sp == "equal":
            assert np.array_equal(gpos[qoff[q]:qoff[q + 1]], np.arange(n))


def test_long_and_short_lists_share_one_call():
    e = N.eval_classes()
    S, L, tile = e["block"], e["sort_lds"], e["tile"]
    rng = np.random.default_rng(31)
    short = [int(v) for v in rng.integers(1, e["wave"] + 1, 100)]
    lens = short[:30] + [L + 1] + short[30:50] + [S + 1, 2 * S + 1] + short[50:80] + [5 * tile + 7, L] + short[80:]
    assert (L + 1 - 1) // tile != (5 * tile + 7 - 1) // tile    # two multi-block lists of different tile counts
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    sc = rng.integers(-40, 41, qoff[-1]) * 0.25              # ties in every long list
    lab = rng.integers(0, 5, qoff[-1]).astype(np.float32)
    _, pos, _ = ER.eval_lists(sc, lab, qoff, "DCG", 1, want_pos=True)
    for metric, k in (("NDCG", 10), ("MAP", 0)):
        got, gpos, gideal = N.eval_lists(sc, lab, qoff, metric, k, want_pos=True)
        path = N.eval_path()
        want, _, ideal = ER.eval_lists(sc, lab, qoff, metric, k, pos=pos)
        assert path == path_of(lens) and path["sort_multi"] == 2 and path["sort_lds"] == 3 and path["tiny"] + path["wave"] == 100
        assert np.array_equal(gpos, pos) and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(gideal), bits(ideal)), metric


def test_score_lists_ranks_long_lists_on_the_device(monkeypatch):
    e = N.eval_classes()
    lens = [e["block"] + 1, e["sort_lds"] + 1]
    rng = np.random.default_rng(32)
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    sc = rng.standard_normal(qoff[-1]).round(2)
    lab = rng.integers(0, 5, qoff[-1]).astype(np.float32)
    samples = [RankList([DataPoint.from_parsed(float(l), str(q + 1), "", np.zeros(1, np.float32)) for l in lab[qoff[q]:qoff[q + 1]]])
               for q in range(2)]
    want, wpos, _ = ER.eval_lists(sc, lab, qoff, "NDCG", 10, want_pos=True)
    by_list = M.NDCGScorer(10)
    for q, rl in enumerate(samples):
        by_list.score(RankList(rl, list(stable_desc_order(sc[qoff[q]:qoff[q + 1]]))))
    assert max(lens) <= M.EVAL_HOST_LEN
    scorer = M.NDCGScorer(10)
    got, pos = M.score_lists(scorer, samples, sc, want_pos=True)
    assert N.eval_path() == path_of(lens) and sum(N.eval_path().values()) == 2           # none went to the host
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(pos, wpos) and scorer.idealGains == by_list.idealGains
    monkeypatch.setattr(M, "EVAL_HOST_LEN", 6)              # the host path stays reachable, and gives the same bits
    calls = []
    monkeypatch.setattr(N, "eval_lists", lambda *a, **kw: calls.append(a))
    scorer = M.NDCGScorer(10)
    got, pos = M.score_lists(scorer, samples, sc, want_pos=True)
    assert not calls and np.array_equal(bits(got), bits(want)) and np.array_equal(pos, wpos) and scorer.idealGains == by_list.idealGains


def test_the_test_flow_writes_the_same_idv_file_batch_and_list_by_list(tmp_path, monkeypatch):
    n = N.eval_classes()["sort_lds"] + 1
    rng = np.random.default_rng(33)
    data, model = str(tmp_path / "long.txt"), str(tmp_path / "model.txt")
    with open(data, "w", encoding="ascii") as f:
        for q, m in (("1", 9), ("2", n), ("3", 40)):
            for _ in range(m):
                f.write("%d qid:%s 1:%.1f 2:%.1f\n" % (rng.integers(0, 5), q, rng.integers(0, 9) * 0.5, rng.integers(0, 9) * 0.5))
    trees = [T.flatten(T.S(1, 2.0, T.S(2, 1.0, T.L(0.5), T.L(-0.25)), T.S(2, 3.0, T.L(0.125), T.L(1.0)))), T.flatten(T.S(1, 0.5, T.L(0.25), T.L(-0.5)))]
    with open(model, "w", encoding="ascii") as f:
        f.write(T.model_text(trees, np.ones(2, np.float32)))
    idv = {}
    for batch in (True, False):
        monkeypatch.setattr(Evaluator, "batch", batch)
        for m in ("NDCG@10", "MAP"):
            path = str(tmp_path / ("%s.%s.idv" % (m[:3], batch)))
            Evaluator(RankerType.LAMBDAMART, m, m).test(model, data, path)
            idv[m, batch] = open(path, "rb").read()
        if batch:
            assert N.eval_path()["sort_multi"] == 1 and sum(N.eval_path().values()) == 3
    for m in ("NDCG@10", "MAP"):
        assert idv[m, True] == idv[m, False] and idv[m, True].count(b"\n") == 4
