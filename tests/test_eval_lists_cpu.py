"""Test-time evaluation without a GPU: the flat restatement of rl_eval_lists (tests/eval_lists_restatement.py) against the scorer classes
and stable_desc_order, the ABI entry and the refusals it makes before it looks for a device, and metric.score_lists' resolution of what a
scorer object holds, with the restatement in _native.eval_lists' place.  Every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import eval_lists_restatement as ER
from ranklib_amd import _native as N
from ranklib_amd import metric as M
from ranklib_amd.learning import DataPoint, RankList, stable_desc_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ([1, 2, 3], [15, 16, 17], [63, 64, 65], [255, 256, 257])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def scorer_of(metric, k):
    s = M.MetricScorerFactory().createScorer(metric)
    s.setK(k)
    return s


def lists_of(labels, qoff, ids=None):
    out = []
    for q in range(len(qoff) - 1):
        qid = str(ids[q]) if ids is not None else "q%d" % q
        out.append(RankList([DataPoint.from_parsed(float(l), qid, "# d%d" % i, np.zeros(2, np.float32))
                             for i, l in enumerate(labels[qoff[q]:qoff[q + 1]])]))
    return out


def by_scorers(scorer, samples, sc, qoff):
    """the per-list host path: (values, positions)"""
    vals, pos = [], np.zeros(len(sc), np.int32)
    for q, rl in enumerate(samples):
        order = stable_desc_order(sc[qoff[q]:qoff[q + 1]])
        pos[qoff[q] + order] = np.arange(len(order), dtype=np.int32)
        vals.append(scorer.score(RankList(rl, list(order))))
    return np.array(vals, np.float64), pos


@pytest.mark.parametrize("lengths", GROUPS, ids=lambda g: "n%d" % g[1])
def test_restatement_equals_the_scorer_classes(lengths):
    sc, lab, qoff, what = ER.make_file(lengths, seed=lengths[1])
    samples = lists_of(lab, qoff)
    pos = None
    for metric in ER.METRICS:
        for k in ER.ks_of(lengths):
            scorer = scorer_of(metric, k)
            want, wpos = by_scorers(scorer, samples, sc, qoff)
            got, gpos, ideal = ER.eval_lists(sc, lab, qoff, metric, k, want_pos=True, pos=pos)
            pos = gpos
            assert np.array_equal(gpos, wpos), (metric, k)
            bad = np.flatnonzero(bits(got) != bits(want))
            assert not bad.size, (metric, k, [what[q] for q in bad[:3]], got[bad[:3]], want[bad[:3]])
            if metric == "NDCG":
                assert np.array_equal(bits(ideal), bits([scorer.idealGains["q%d" % q] for q in range(len(samples))]))
            else:
                assert np.isnan(ideal).all()
    for q, (n, sp, _) in enumerate(what):
        if sp == "equal":
            assert np.array_equal(pos[qoff[q]:qoff[q + 1]], np.arange(n))
    # plain RR is k = 0: always 0, as written
    assert not ER.eval_lists(sc, lab, qoff, "RR", M.ReciprocalRankScorer().k)[0].any()


def test_counting_rank_equals_the_stable_sort():
    rng = np.random.default_rng(5)
    for n in (1, 2, 64, 65, 300, ER.COUNT_MAX + 476):
        for sp in ER.SCORE_PATTERNS:
            s = ER.scores_of(sp, n, rng)
            counted, sorted_ = ER.positions(s, count=True), ER.positions(s, count=False)
            assert np.array_equal(counted, sorted_), (n, sp)
            order = stable_desc_order(s)
            assert np.array_equal(order[counted], np.arange(n)), (n, sp)


def test_restatement_keeps_the_ideal_of_the_first_list_of_an_id():
    rng = np.random.default_rng(9)
    lab = np.concatenate([[3, 0, 1, 0], [0, 0, 1, 0, 0], [2, 2, 0]]).astype(np.float32)
    qoff = np.array([0, 4, 9, 12], np.int32)
    sc = rng.standard_normal(12)
    ids, qkey = ["7", "7", "8"], np.array([0, 0, 1], np.int32)
    scorer = scorer_of("NDCG", 10)
    want, _ = by_scorers(scorer, lists_of(lab, qoff, ids), sc, qoff)
    got, _, ideal = ER.eval_lists(sc, lab, qoff, "NDCG", 10, qkey=qkey)
    assert np.array_equal(bits(got), bits(want))
    assert ideal[1] == ideal[0] == scorer.idealGains["7"] and ideal[1] != ER.ideal_dcg_of(lab[4:9], 5)
    # given entries with NaN holes, relevant-document counts with zeros
    given = np.array([np.nan, np.nan, 2.5])
    scorer = scorer_of("NDCG", 2)
    scorer.idealGains["8"] = 2.5
    want, _ = by_scorers(scorer, lists_of(lab, qoff, ids), sc, qoff)
    got, _, ideal = ER.eval_lists(sc, lab, qoff, "NDCG", 2, qkey=qkey, ideal_dcg=given)
    assert np.array_equal(bits(got), bits(want)) and ideal[2] == 2.5
    ap = M.APScorer()
    ap.relDocCount = {"7": 3}
    want, _ = by_scorers(ap, lists_of(lab, qoff, ids), sc, qoff)
    got, _, _ = ER.eval_lists(sc, lab, qoff, "MAP", 0, rel_doc_count=np.array([3, 3, 0], np.int32))
    assert np.array_equal(bits(got), bits(want)) and got[2] == 0.0


# ---- the ABI entry ----------------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return N.lib()


def test_library_exports_rl_eval_lists_and_the_abi_version_stays():
    L = _lib()
    assert hasattr(L, "rl_eval_lists")
    assert L.rl_abi_version() == 5
    assert N.RL_EVAL_METRIC["BEST"] == 6 and "BEST" not in N.RL_CA_METRIC
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    assert "RL_METRIC_BEST = 6" in hdr


def _call(sc, lab, qoff, metric=0, k=10, n_docs=None, n_lists=None, out=True, rdc=None):
    L = _lib()
    sc = None if sc is None else np.ascontiguousarray(sc, np.float64)
    lab = None if lab is None else np.ascontiguousarray(lab, np.float32)
    qoff = None if qoff is None else np.ascontiguousarray(qoff, np.int32)
    rdc = None if rdc is None else np.ascontiguousarray(rdc, np.int32)
    nl = n_lists if n_lists is not None else len(qoff) - 1
    o = np.zeros(max(1, nl), np.float64)
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    rc = L.rl_eval_lists(0, metric, k, 16.0, p(sc), p(lab), n_docs if n_docs is not None else len(sc), p(qoff), nl, None, None, p(rdc),
                         o.ctypes.data if out else None, None, None)
    return rc, L.rl_last_error().decode()


def test_refusals_come_before_any_device_call():
    """every one of these returns RL_ERR_INVALID (-1) or RL_ERR_UNSUPPORTED (-4) with its own message, on a machine with a GPU and on one
    without: a call that got as far as the device would answer RL_ERR_NO_DEVICE (-5) here"""
    sc, lab, qoff = np.array([0.5, 0.25, 1.0]), np.array([1, 0, 2], np.float32), np.array([0, 2, 3], np.int32)
    for kw in (dict(sc=None), dict(lab=None), dict(qoff=None), dict(out=False)):
        a = dict(sc=sc, lab=lab, qoff=qoff)
        a.update(kw)
        rc, msg = _call(a.pop("sc"), a.pop("lab"), a.pop("qoff"), n_docs=3, n_lists=2, **a)
        assert rc == -1 and "null argument" in msg, (kw, rc, msg)
    for bad in ([1, 2, 3], [0, 2, 2], [0, 2, 4], [0, 3, 2], [0, 1, 2]):
        rc, msg = _call(sc, lab, np.array(bad, np.int32))
        assert rc == -1 and "qoff" in msg, (bad, rc, msg)
    for m in (-1, 7, 100):
        rc, msg = _call(sc, lab, qoff, metric=m)
        assert rc == -1 and "unknown metric" in msg
    rc, msg = _call(sc, np.array([1, -1, 2], np.float32), qoff)
    assert rc == -1 and "Relevance label cannot be negative" in msg
    rc, msg = _call(sc, np.array([1, 0, 2.0 ** 24], np.float32), qoff)
    assert rc == -4 and "2^24" in msg
    rc, msg = _call(sc, np.array([1, 0, 2.0 ** 24 - 1], np.float32), qoff, rdc=[1, -1])
    assert rc == -1 and "relevant-document count" in msg
    rc, msg = _call(np.array([0.5, 0.25, np.nan]), lab, qoff)
    assert rc == -1 and "NaN score in list 1" in msg
    rc, msg = _call(np.array([0.5, np.nan, 1.0]), lab, qoff)
    assert rc == -1 and "NaN score in list 0 (document 1)" in msg


def test_native_eval_lists_checks_its_arrays():
    _lib()
    with pytest.raises(N.RankLibError, match="metric must be one of"):
        N.eval_lists([1.0], [0.0], [0, 1], "F1", 10)
    with pytest.raises(N.RankLibError, match="scores \\[n_docs\\]"):
        N.eval_lists([1.0, 2.0], [0.0], [0, 2], "NDCG", 10)
    with pytest.raises(N.RankLibError, match="qkey \\[n_lists\\]"):
        N.eval_lists([1.0, 2.0], [0.0, 1.0], [0, 2], "NDCG", 10, qkey=[0, 1])


# ---- metric.score_lists, the restatement in the kernel's place --------------------------------------------------------------------------
@pytest.fixture
def restated(monkeypatch):
    calls = []

    def fake(*a, **kw):
        calls.append((a, kw))
        return ER.eval_lists(*a, **kw)
    monkeypatch.setattr(N, "eval_lists", fake)
    return calls


def _file(seed=3, ids=("1", "2", "2", "3", "1", "4")):
    rng = np.random.default_rng(seed)
    lens = [5, 3, 7, 1, 4, 6][:len(ids)]
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    lab = rng.integers(0, 4, qoff[-1]).astype(np.float32)
    return rng.standard_normal(qoff[-1]).round(1), lab, qoff, list(ids)


@pytest.mark.parametrize("metric", ["NDCG@3", "NDCG@10", "DCG@2", "MAP", "ERR@10", "P@5", "RR@3", "RR", "Best@3"])
def test_score_lists_equals_the_per_list_path(restated, metric):
    sc, lab, qoff, ids = _file()
    a, b = M.MetricScorerFactory().createScorer(metric), M.MetricScorerFactory().createScorer(metric)
    want, wpos = by_scorers(a, lists_of(lab, qoff, ids), sc, qoff)
    got, pos = M.score_lists(b, lists_of(lab, qoff, ids), sc, want_pos=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(pos, wpos)
    assert len(restated) == 1 and restated[0][1]["err_max"] == M.ERRScorer.MAX
    if metric.startswith("NDCG"):
        assert a.idealGains == b.idealGains and sorted(b.idealGains) == ["1", "2", "3", "4"]      # written back, the first list of an id deciding


def test_score_lists_resolves_what_the_scorer_holds(restated, monkeypatch):
    sc, lab, qoff, ids = _file()
    # -qrel entries: ids "2" and "4" have an ideal DCG, "9" is not in the file
    a, b = M.NDCGScorer(3), M.NDCGScorer(3)
    for s in (a, b):
        s.idealGains.update({"2": 7.5, "4": 0.0, "9": 1.0})
    want, _ = by_scorers(a, lists_of(lab, qoff, ids), sc, qoff)
    got, _ = M.score_lists(b, lists_of(lab, qoff, ids), sc)
    assert np.array_equal(bits(got), bits(want)) and a.idealGains == b.idealGains and got[5] == 0.0
    kw = restated[-1][1]
    assert np.array_equal(kw["qkey"], [0, 1, 1, 2, 0, 3]) and np.isnan(kw["ideal_dcg"][[0, 3, 4]]).all() and kw["ideal_dcg"][1] == 7.5
    # a scorer used again (k-fold: the next fold's lists share ids with this one's) sees the ideals it cached
    sc2, lab2, qoff2, ids2 = _file(seed=4, ids=("3", "5", "1"))
    want, _ = by_scorers(a, lists_of(lab2, qoff2, ids2), sc2, qoff2)
    got, _ = M.score_lists(b, lists_of(lab2, qoff2, ids2), sc2)
    assert np.array_equal(bits(got), bits(want)) and a.idealGains == b.idealGains
    # MAP: the external count, 0 for an id the judgments do not have
    a, b = M.APScorer(), M.APScorer()
    a.relDocCount = b.relDocCount = {"1": 4, "2": 1}
    want, _ = by_scorers(a, lists_of(lab, qoff, ids), sc, qoff)
    got, _ = M.score_lists(b, lists_of(lab, qoff, ids), sc)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(restated[-1][1]["rel_doc_count"], [4, 1, 1, 0, 4, 0])
    assert restated[-1][1]["qkey"] is None and restated[-1][1]["ideal_dcg"] is None
    # -gmax reaches the call
    monkeypatch.setattr(M.ERRScorer, "MAX", 4.0)
    want, _ = by_scorers(M.ERRScorer(10), lists_of(lab, qoff, ids), sc, qoff)
    got, _ = M.score_lists(M.ERRScorer(10), lists_of(lab, qoff, ids), sc)
    assert np.array_equal(bits(got), bits(want)) and restated[-1][1]["err_max"] == 4.0


@pytest.mark.parametrize("nan_list", [0, 1, 2, 4])
def test_score_lists_sends_a_list_with_a_nan_score_down_the_host_path(restated, nan_list):
    """only that list; and where it is the first list of its id (0 and 1 are, 2 and 4 are not) it still decides the id's ideal DCG"""
    sc, lab, qoff, ids = _file()
    sc = sc.copy()
    sc[qoff[nan_list]] = np.nan
    for metric in ("NDCG@3", "MAP", "Best@2"):
        a, b = M.MetricScorerFactory().createScorer(metric), M.MetricScorerFactory().createScorer(metric)
        want, wpos = by_scorers(a, lists_of(lab, qoff, ids), sc, qoff)
        got, pos = M.score_lists(b, lists_of(lab, qoff, ids), sc, want_pos=True)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(pos, wpos)
        assert len(restated[-1][0][0]) == len(sc) - (qoff[nan_list + 1] - qoff[nan_list])       # the call never saw the list
        if metric == "NDCG@3":
            assert a.idealGains == b.idealGains


def test_score_lists_sends_a_long_list_down_the_host_path(restated, monkeypatch):
    monkeypatch.setattr(M, "EVAL_HOST_LEN", 6)
    sc, lab, qoff, ids = _file()
    a, b = M.NDCGScorer(3), M.NDCGScorer(3)
    want, wpos = by_scorers(a, lists_of(lab, qoff, ids), sc, qoff)
    got, pos = M.score_lists(b, lists_of(lab, qoff, ids), sc, want_pos=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(pos, wpos) and a.idealGains == b.idealGains
    assert len(restated[-1][0][0]) == len(sc) - 7
    with pytest.raises(N.RankLibError, match="one score per document"):
        M.score_lists(b, lists_of(lab, qoff, ids), sc[:-1])
