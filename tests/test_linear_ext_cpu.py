"""The checker of the linear rankers (tests/{np,ca,ada,rb,lr}_restatement.py) on what -qrel, labels of 31 and above and fractional labels
ask of it, without a GPU: the gain in Java int arithmetic against known answers and the C oracle, the literal scorer against the
vectorised one on external ideal DCGs / relevant-document counts / wrapped and fractional labels, and both against the host scorers
(ranklib_amd.metric, pinned by test_host_mirror.py) that loaded a judgment file.  Every comparison is bit for bit."""
import numpy as np
import pytest

import ada_restatement as AR
import ca_restatement as CR
import linear_ext as E
import lr_restatement as LR
import np_restatement as R
import oracle_ffi as O
import rb_restatement as RB
from ranklib_amd.learning import DataPoint, RankList
from ranklib_amd.metric import APScorer, NDCGScorer


def _bits(v):
    return np.float64(v).tobytes()


def test_gain_known_answers():
    """metric/DCGScorer.java:28-31,137-139 and ERRScorer.java:71-73: (1 << rel) - 1 on ints"""
    assert [R.gain(r) for r in (0, 1, 4, 30, 31, 32, 33, 63)] == [0.0, 1.0, 15.0, 1073741823.0, 2147483647.0, 0.0, 1.0, 2147483647.0]
    assert [R.gain(np.int64(r)) for r in (31, 32, 40)] == [2147483647.0, 0.0, 255.0]
    assert list(CR._GAIN[[30, 31, 0, 1]]) == [1073741823.0, 2147483647.0, 0.0, 1.0] and len(CR._GAIN) == 32
    assert R.ERR(10).R(31) == 2147483647.0 / 16.0 and R.ERR(10).R(32) == 0.0 and R.ERR(10).R(33) == 1.0 / 16.0


@pytest.mark.parametrize("k", [3, 10])
def test_wrapped_gains_against_the_oracle(k):
    rng = np.random.default_rng(40 + k)
    wild = np.array([0, 1, 2, 30, 31, 32, 33, 40], np.float32)
    seen = set()
    for n in (1, 2, 5, 9, 10, 11, 24):
        for _ in range(6):
            lab = rng.choice(wild, n)
            scores = rng.permutation(n).astype(np.float64)               # distinct: no tie for two sorts to resolve differently
            qoff = np.array([0, n], np.int32)
            for cls in (CR.LiteralScorer, CR.VectorScorer):
                cache = list(scores) if cls is CR.LiteralScorer else scores
                assert _bits(cls("NDCG", k).score(cache, lab, qoff, ["a"])) == _bits(O.query_ndcg(scores, lab, k)), (n, lab)
                assert _bits(cls("DCG", k).score(cache, lab, qoff, ["a"])) == _bits(O.query_score("DCG", scores, lab, k)), (n, lab)
            seen |= set(lab.tolist())
    assert seen == set(wild.tolist())


def _mixed(rng, labels, Q=40, hi=31):
    tr = E.data(rng, rng.integers(1, hi, Q), 3, labels, qid=["q%d" % (i % (Q - 7)) for i in range(Q)])
    cache = rng.integers(0, 6, int(tr[2][-1])).astype(np.float64) * 0.25         # heavy ties: the stable order matters
    return tr, cache


@pytest.mark.parametrize("labels", [(0, 1, 2), E.WRAPPED, E.FRACTIONAL, (0, 1, 2, 30, 31, 32, 33, 40)], ids=["plain", "wrapped", "fractional", "wild"])
def test_literal_against_vectorised_with_external_judgments(labels):
    rng = np.random.default_rng(7)
    (X, lab, qoff, qid), cache = _mixed(rng, labels)
    ideal = E.ideal_map([(X, lab, qoff, qid)], 10, rng)
    own = {q: max(R.ideal_dcg([int(v) for v in l], min(10, len(l))) for l in labs) for q, labs in E._by_qid([(X, lab, qoff, qid)]).items()}
    assert any(v < own[q] for q, v in ideal.items() if own[q] > 0) and any(v > own[q] for q, v in ideal.items() if own[q] > 0)
    assert 0 < len(ideal) < len(set(qid))
    counts = E.count_map([(X, lab, qoff, qid)], rng)
    assert 0 in counts.values() and any(v > 0 for v in counts.values()) and len(counts) < len(set(qid))
    cases = [("NDCG", 10, dict(ideal=ideal)), ("NDCG", 10, {}), ("NDCG", 3, dict(ideal=ideal)), ("MAP", 0, dict(rel_doc_count=counts)),
             ("MAP", 0, {}), ("MAP", 0, dict(rel_doc_count={})), ("DCG", 5, {}), ("ERR", 10, {}), ("P", 3, {}), ("RR", 10, {})]
    values = {}
    for i, (metric, k, ext) in enumerate(cases):
        a = CR.LiteralScorer(metric, k, **ext).score(list(cache), lab, qoff, qid)
        b = CR.VectorScorer(metric, k, **ext).score(cache, lab, qoff, qid)
        assert _bits(a) == _bits(b), (metric, k, ext.keys())
        values[i] = a
    assert values[0] != values[1] and values[3] != values[4] and values[5] == 0.0
    # the validation set scored with another map, or with its own counts
    for cls, c in ((CR.LiteralScorer, list(cache)), (CR.VectorScorer, cache)):
        sc = cls("MAP", 0, rel_doc_count=counts, valid_rel_doc_count=None)
        assert _bits(sc.score(c, lab, qoff, qid, valid=True)) == _bits(values[4])
        assert _bits(sc.score(c, lab, qoff, qid)) == _bits(values[3])
        sc = cls("MAP", 0, rel_doc_count=None, valid_rel_doc_count=counts)
        assert _bits(sc.score(c, lab, qoff, qid, valid=True)) == _bits(values[3]) and _bits(sc.score(c, lab, qoff, qid)) == _bits(values[4])


def test_literal_against_vectorised_on_long_lists():
    """the vectorised MAP takes few long lists one by one: the same serial sums"""
    rng = np.random.default_rng(8)
    X, lab, qoff, qid = E.data(rng, [3, 700, 17, 1, 385], 2, E.FRACTIONAL)
    cache = rng.integers(0, 9, int(qoff[-1])).astype(np.float64) * 0.25
    counts = {"q0": 0, "q1": 900, "q4": int(np.sum(lab[qoff[4]:qoff[5]] > 0))}
    for ext in ({}, dict(rel_doc_count=counts)):
        a = CR.LiteralScorer("MAP", 0, **ext).score(list(cache), lab, qoff, qid)
        assert _bits(a) == _bits(CR.VectorScorer("MAP", 0, **ext).score(cache, lab, qoff, qid)) and a > 0.0


def test_fractional_labels_split_the_two_families():
    """a 0.5 is relevant for MAP / P / RR (label > 0) and gain 0 for NDCG / DCG / ERR ((int) label)"""
    lab = np.array([0.5, 0.0, 2.99, 1.5], np.float32)
    qoff = np.array([0, 4], np.int32)
    cache = [4.0, 3.0, 2.0, 1.0]
    for cls, c in ((CR.LiteralScorer, cache), (CR.VectorScorer, np.array(cache))):
        s = lambda m, k: cls(m, k).score(c, lab, qoff, ["a"])      # noqa: E731
        assert s("MAP", 0) == (1 / 1 + 2 / 3 + 3 / 4) / 3 and s("P", 3) == 2 / 3 and s("RR", 10) == 1.0
        assert s("DCG", 10) == 3.0 * R.discount(2) + 1.0 * R.discount(3)
        assert s("NDCG", 10) == (3.0 * R.discount(2) + R.discount(3)) / (3.0 + R.discount(1))
        assert s("ERR", 10) == (3 / 16) / 3 + (1 - 3 / 16) * (1 / 16) / 4


def _rank_lists(rng, labels, names):
    lists = []
    for name in names:
        n = int(rng.integers(1, 15))
        lab = rng.choice(np.array(labels, np.float32), n)
        lists.append(RankList([DataPoint("%s qid:%s 1:%d.0 # d%d" % (repr(float(v)), name, i, i)) for i, v in enumerate(lab)]))
    return lists


@pytest.mark.parametrize("labels", [(0, 1, 2, 3), E.WRAPPED, E.FRACTIONAL], ids=["plain", "wrapped", "fractional"])
def test_restated_scorers_against_the_host_scorers_on_a_judgment_file(tmp_path, labels):
    """NDCGScorer / APScorer.loadExternalRelevanceJudgment (metric/NDCGScorer.java:50-96, APScorer.java:45-66) give the maps; score() of the
    host classes on hand-ranked lists equals the restated scorers fed the same maps -- a second implementation, not the kernels under test"""
    rng = np.random.default_rng(12)
    names = ["7", "3", "11", "3", "20", "8", "9", "5", "8", "30", "31", "32"]                 # 3 and 8 twice
    qrel = str(tmp_path / "qrel.txt")
    with open(qrel, "w") as f:
        for name in ("3", "7", "9", "20", "77", "31"):                                          # 77 names no list; 11, 8, 5, 30, 32 are not judged
            for d in range(int(rng.integers(2, 25))):
                f.write("%s 0 doc%d %d\n" % (name, d, 0 if name == "31" else int(rng.integers(0, 4))))     # 31: no relevant document
    lists = _rank_lists(rng, labels, names)
    lab = np.concatenate([[dp.getLabel() for dp in rl.rl] for rl in lists]).astype(np.float32)
    qoff = np.concatenate([[0], np.cumsum([rl.size() for rl in lists])]).astype(np.int32)
    cache = np.concatenate([-np.arange(rl.size(), dtype=np.float64) for rl in lists])           # the lists as they stand
    for k in (10, 3):
        host = NDCGScorer(k)
        host.loadExternalRelevanceJudgment(qrel)
        gains = dict(host.idealGains)
        assert set(gains) == {"3", "7", "9", "20", "77", "31"} and gains["31"] == 0.0
        lit, vec = CR.LiteralScorer("NDCG", k, ideal=gains), CR.VectorScorer("NDCG", k, ideal=gains)
        plain = CR.LiteralScorer("NDCG", k)
        per = [host.score(rl) for rl in lists]
        for q, rl in enumerate(lists):
            assert _bits(per[q]) == _bits(lit.m.score([float(v) for v in lab[qoff[q]:qoff[q + 1]]], names[q])), (k, q)
        assert _bits(NDCGScorer(k).score(lists)) == _bits(plain.score(list(cache), lab, qoff, names))
        h2 = NDCGScorer(k)
        h2.loadExternalRelevanceJudgment(qrel)
        want = h2.score(lists)
        assert _bits(want) == _bits(CR.LiteralScorer("NDCG", k, ideal=gains).score(list(cache), lab, qoff, names))
        assert _bits(want) == _bits(vec.score(cache, lab, qoff, names))
        assert want != plain.score(list(cache), lab, qoff, names)
    host = APScorer()
    host.loadExternalRelevanceJudgment(qrel)
    counts = dict(host.relDocCount)
    assert "31" not in counts and "77" in counts
    want = host.score(lists)
    assert _bits(want) == _bits(CR.LiteralScorer("MAP", 0, rel_doc_count=counts).score(list(cache), lab, qoff, names))
    assert _bits(want) == _bits(CR.VectorScorer("MAP", 0, rel_doc_count=counts).score(cache, lab, qoff, names))
    assert _bits(APScorer().score(lists)) == _bits(CR.VectorScorer("MAP", 0).score(cache, lab, qoff, names)) and APScorer().score(lists) != want
    for q, rl in enumerate(lists):
        if names[q] not in counts:
            assert host.score(rl) == 0.0


def _judged(metric, rng, tr, va, factors=(0.5, 1.0, 2.0)):
    if metric == "NDCG":
        return dict(ideal=E.ideal_map([tr, va], 10, rng, factors))
    return dict(rel_doc_count=E.count_map([tr, va], rng))


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_learn_functions_pass_the_judgments_through(metric, k):
    """each restatement's learn() with the maps differs from the run without, and Coordinate Ascent's two scorers still agree"""
    rng = np.random.default_rng(21)
    tr, va = E.shared_sets(rng, 4, n_train=20, n_valid=8, hi=12)
    ext = _judged(metric, rng, tr, va, (1.0, 2.0))
    p = dict(nRestart=1, nMaxIteration=6, seed=2)
    a, b = CR.learn(tr, va, metric, k, literal=True, **p, **ext), CR.learn(tr, va, metric, k, **p, **ext)
    assert a["trace"] == b["trace"] and a["weight"] == b["weight"] and a["train"] == b["train"] and a["valid"] == b["valid"]
    assert a["train"] != CR.learn(tr, va, metric, k, **p)["train"]
    assert AR.learn(tr, va, metric, k, nIteration=8, **ext)["trace"] != AR.learn(tr, va, metric, k, nIteration=8)["trace"]
    sc = CR.LiteralScorer(metric, k, **ext)
    assert not np.array_equal(AR.weak_table(tr[0], tr[1], tr[2], tr[3], sc, metric, k),
                              AR.weak_table(tr[0], tr[1], tr[2], tr[3], CR.LiteralScorer(metric, k), metric, k))
    assert RB.learn(tr, va, metric, k, nIteration=5, **ext)["trace"] != RB.learn(tr, va, metric, k, nIteration=5)["trace"]
    x, y = LR.learn(tr, va, metric, k, **ext), LR.learn(tr, va, metric, k)
    assert x["weight"] == y["weight"] and x["train"] != y["train"] and x["valid"] != y["valid"]
    if metric == "MAP":                                       # the validation set alone keeps its own counts
        z = LR.learn(tr, va, metric, k, rel_doc_count=ext["rel_doc_count"], valid_rel_doc_count=None)
        assert z["train"] == x["train"] and z["valid"] == y["valid"]
