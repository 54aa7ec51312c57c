"""AdaRank (-ranker 3) on the MI355X: every round's feature, alpha, train and validation score, every rollback, the model and the final
scores bit-identical to the literal restatement of AdaRank.learn (tests/ada_restatement.py); the weak-ranker table bit-identical to the
restatement's Sorter order; the refusals; and the reference's testAdaRank flow through the command line.

-qrel judgments are covered by test_external_judgments_match_the_restatement (per set), test_weak_table_external_judgments_across_the_
length_classes, test_cli_qrel_reaches_the_trainer and test_external_judgment_refusals; labels of 31 and above (gains that wrap as Java
ints) by test_weak_table_wrapped_labels and test_learn_wrapped_labels; fractional labels by test_fractional_labels."""
import functools

import numpy as np
import pytest

import ada_restatement as AR
import linear_ext as E
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd.learning import AdaRank, CoorAscent, DataPoint, RankList, java_double_str
from ranklib_amd.metric import ERRScorer, MetricScorerFactory

pytestmark = pytest.mark.gpu

_STATICS = ("nIteration", "tolerance", "trainWithEnqueue", "maxSelCount", "device")


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = {k: getattr(AdaRank, k) for k in _STATICS}
    gmax, ca_tol, rf_frate, rf_bag = ERRScorer.MAX, CoorAscent.tolerance, learning.RFRanker.featureSamplingRate, learning.RFRanker.nBag
    yield
    for k, v in saved.items():
        setattr(AdaRank, k, v)
    ERRScorer.MAX, CoorAscent.tolerance, learning.RFRanker.featureSamplingRate, learning.RFRanker.nBag = gmax, ca_tol, rf_frate, rf_bag


def _data(rng, lengths, F, levels=3, labels=3):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    X = (rng.integers(0, levels, (qoff[-1], F)).astype(np.float32) * np.float32(0.37)).astype(np.float32)
    X[rng.random(X.shape) < 0.1] = 0.0
    lab = rng.integers(0, labels, qoff[-1]).astype(np.float32)
    return X, lab, qoff, ["q%d" % i for i in range(len(lengths))]


def _trainer(train, valid=None, metric="NDCG", k=10, err_max=16.0, ext=None, **p):
    """ext: the per-list external judgments of linear_ext.feed (ideal_tr / ideal_va / rdc_tr / rdc_va)"""
    return E.feed(N.AdaRankTrainer(metric=metric, metric_k=k, err_max=err_max, **p), train, valid, **(ext or {}))


def _bits(v):
    return np.float64(v).tobytes()


def _events(r, n_iteration):
    ev = set()
    for t in r["trace"]:
        if t[1] == AR.ROLLBACK:
            ev.add("ROLLBACK")
        elif t[1] == AR.ROUND and t[3] == AR.FREM:
            ev.add("F. REM.")
        elif t[1] == AR.ROUND and t[3] == AR.DAMN:
            ev.add("STOP")
    if any(t[1] == AR.ROUND and t[0] == n_iteration for t in r["trace"]):
        ev.add("ROUND LIMIT")
    if r["restored"]:
        ev.add("BEST ON VALIDATION")
    return ev


# (metric, k, -gmax, validation, enqueue, -max, -round, -tolerance, list lengths [lo, hi), labels, seed, events the case must cover)
_CASES = [
    ("NDCG", 10, 16.0, True, True, 5, 60, 0.002, (1, 25), 3, 0, {"ROLLBACK", "F. REM.", "STOP", "ROUND LIMIT", "BEST ON VALIDATION"}),
    ("DCG", 1, 16.0, False, True, 5, 60, 0.002, (1, 25), 2, 0, {"STOP"}),
    ("MAP", 0, 16.0, True, False, 2, 40, 0.05, (1, 6), 2, 0, {"F. REM.", "ROUND LIMIT", "BEST ON VALIDATION"}),
    ("ERR", 10, 8.0, True, True, 5, 60, 0.002, (1, 25), 3, 0, {"ROLLBACK", "F. REM.", "STOP", "BEST ON VALIDATION"}),
    ("P", 5, 16.0, False, False, 2, 40, 0.002, (1, 25), 3, 2, {"STOP"}),
    ("RR", 10, 16.0, True, True, 5, 30, 0.002, (1, 25), 3, 1, {"ROLLBACK", "STOP", "BEST ON VALIDATION"}),
    ("NDCG", 3, 16.0, False, False, 2, 15, 0.05, (1, 6), 2, 0, {"F. REM.", "ROUND LIMIT"}),
    ("DCG", 1, 16.0, True, True, 5, 40, 0.01, (1, 6), 2, 2, {"ROLLBACK", "STOP", "BEST ON VALIDATION"}),
]


@pytest.mark.parametrize("case", _CASES, ids=["%s%d-%s-%s" % (c[0], c[1], "valid" if c[3] else "novalid", "enq" if c[4] else "noeq")
                                              for c in _CASES])
def test_trace_parity_with_the_restatement(case):
    metric, k, gmax, valid, enq, mx, rounds, tol, (lo, hi), labels, seed, expect = case
    rng = np.random.default_rng(seed)
    tr = _data(rng, rng.integers(lo, hi, 37), 5, labels=labels)              # 37 lists: the float start weight 1.0f / 37 is inexact
    va = _data(rng, rng.integers(lo, hi, 23), 5, labels=labels) if valid else None
    r = AR.learn(tr, va, metric=metric, k=k, nIteration=rounds, tolerance=tol, trainWithEnqueue=enq, maxSelCount=mx, err_max=gmax)
    assert expect <= _events(r, rounds), _events(r, rounds)
    t = _trainer(tr, va, metric, k, gmax, n_iteration=rounds, tolerance=tol, train_with_enqueue=enq, max_sel_count=mx)
    t.learn()
    assert np.array_equal(t.weak_table().view(np.int64), r["M"].view(np.int64))
    g = [tuple(x.item()) for x in t.trace()]
    assert len(g) == len(r["trace"])
    for a, b in zip(g, r["trace"]):
        assert a[:4] == b[:4] and all(_bits(a[i]) == _bits(b[i]) for i in (4, 5, 6)), (a, b)
    fid, w = t.model()
    assert list(fid) == r["fid"] and [_bits(x) for x in w] == [_bits(x) for x in r["weight"]]
    ts, vs = t.scores()
    assert _bits(ts) == _bits(r["train"])
    if valid:
        assert _bits(vs) == _bits(r["valid"])


def _weak_gpu(train, metric, k):
    t = _trainer(train, None, metric, k, n_iteration=0)
    t.learn()
    return t.weak_table()


@pytest.mark.parametrize("metric,k", [("MAP", 0), ("NDCG", 10), ("ERR", 5), ("P", 3), ("RR", 10), ("DCG", 4)])
def test_weak_table_on_heavy_ties(metric, k):
    rng = np.random.default_rng(17)
    tr = _data(rng, rng.integers(1, 60, 45), 6, levels=2, labels=3)
    tr[0][:, 3] = (rng.integers(0, 3, tr[0].shape[0]) * 0.5).astype(np.float32)     # three distinct values
    tr[0][:, 5] = 1.0                                                                   # constant: the identity order
    sc = AR.CR.LiteralScorer(metric, k)
    M = AR.weak_table(tr[0], tr[1], tr[2], tr[3], sc, metric, k)
    assert np.array_equal(_weak_gpu(tr, metric, k).view(np.int64), M.view(np.int64))
    if metric == "MAP":                                      # a stable order would give other values on these ties
        X, lab, qoff, qid = tr
        stable = [sc.m.score([float(lab[qoff[q] + i]) for i in learning.stable_desc_order(X[qoff[q]:qoff[q + 1], f])], qid[q])
                  for f in range(X.shape[1]) for q in range(len(qoff) - 1)]
        assert np.any(np.array(stable).reshape(M.shape) != M)


@pytest.mark.parametrize("metric,k,levels", [("MAP", 0, 3), ("NDCG", 10, 3), ("NDCG", 10, 1000), ("ERR", 20, 4)])
def test_weak_table_length_classes(metric, k, levels):
    rng = np.random.default_rng(23)
    lengths = np.array([1, 9, 16, 17, 50, 64, 65, 200, 384, 385, 1200, 5000, 5001, 6100])
    tr = _data(rng, lengths, 3, levels=levels, labels=3)
    sc = AR.CR.LiteralScorer(metric, k)
    M = AR.weak_table(tr[0], tr[1], tr[2], tr[3], sc, metric, k)
    assert np.array_equal(_weak_gpu(tr, metric, k).view(np.int64), M.view(np.int64))


def test_refusals():
    rng = np.random.default_rng(2)
    X, lab, qoff, qid = _data(rng, [4, 5, 6], 3)
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[4, 1] = bad
        with pytest.raises(N.RankLibError):
            N.AdaRankTrainer().set_train(Xb, lab, qoff)
    with pytest.raises(N.RankLibError):
        N.AdaRankTrainer(metric="BEST")
    lab = np.array([1, 0, 1, 0, 0, 1], np.float32)                      # feature 0 ranks every list perfectly under MAP
    Xp = np.array([[1.0, 0.3], [0.0, 0.9], [1.0, 0.1], [0.0, 0.5], [0.2, 0.5], [0.7, 0.4]], np.float32)
    qoff = np.array([0, 2, 4, 6], np.int32)
    with pytest.raises(AR.NonFiniteAlpha):
        AR.learn((Xp, lab, qoff, ["a", "b", "c"]), metric="MAP", k=0)
    t = _trainer((Xp, lab, qoff, ["a", "b", "c"]), None, "MAP", 0)
    with pytest.raises(N.RankLibError) as e:
        t.learn()
    assert "round 1" in str(e.value) and "feature index 0" in str(e.value) and "denom = 0" in str(e.value)


def _write_count_data(path, n_q, n_d, flip=0.0, seed=0):
    """test:eval/EvaluatorTest.java:78-92 writeRandomDataCount (P docs 1:1.0, N docs 1:0.9, 2:+-1), a fraction `flip` of labels flipped"""
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for q in range(n_q):
            for i in range(n_d):
                w1, w2 = rng.choice([-1.0, 1.0], 2)
                lp, ln = (0 if rng.random() < flip else 1), (1 if rng.random() < flip else 0)
                f.write("%d qid:%d 1:1.0 2:%s # P%d\n" % (lp, q, w1, i))
                f.write("%d qid:%d 1:0.9 2:%s # N%d\n" % (ln, q, w2, i))


_FLOW = ["-metric2t", "map", "-ranker", "3", "-frate", "1.0", "-bag", "10", "-round", "10", "-epoch", "10"]


def test_reference_testAdaRank_flow_is_refused(tmp_path):
    """test:eval/EvaluatorTest.java:161-172 (@Ignore'd there: feature 1 is perfect under MAP on round 1, alpha = Infinity)"""
    data, model = str(tmp_path / "data.txt"), str(tmp_path / "model.txt")
    _write_count_data(data, 20, 20)
    with pytest.raises(N.RankLibError) as e:
        evaluator.main(["-train", data] + _FLOW + ["-save", model])
    assert "AdaRank round 1" in str(e.value) and "alpha" in str(e.value)


def _read_count_data(path):
    rows = [line.split() for line in open(path)]
    X = np.array([[float(r[2][2:]), float(r[3][2:])] for r in rows], np.float32)
    lab = np.array([float(r[0]) for r in rows], np.float32)
    qs = [r[1][4:] for r in rows]
    qoff = np.array([0] + [i for i in range(1, len(qs)) if qs[i] != qs[i - 1]] + [len(qs)], np.int32)
    return X, lab, qoff, [qs[a] for a in qoff[:-1]]


def test_reference_testAdaRank_flow_with_flipped_labels(tmp_path):
    """the same flow on data that trains.  With the verbatim flags feature 1 is queued on round 2 (chosen twice in a row) and -round 10
    ends before its turn, so the model holds feature 2 only: the model text is the restatement's.  With -noeq added feature 1 stays, and
    the -rank -indri check of testRanker holds: a P document at rank 1, no N document there."""
    data, model, model2, run = (str(tmp_path / n) for n in ("data.txt", "model.txt", "model2.txt", "run.txt"))
    _write_count_data(data, 20, 20, flip=0.1, seed=4)
    evaluator.main(["-train", data] + _FLOW + ["-save", model])
    r = AR.learn(_read_count_data(data), None, "MAP", 0, nIteration=10)
    head = ["## AdaRank", "## Iteration = 10", "## Train with enqueue: Yes", "## Tolerance = 0.002", "## Max consecutive selection count = 5"]
    assert open(model).read() == "\n".join(head) + "\n" + " ".join("%d:%s" % (f + 1, java_double_str(w)) for f, w in zip(r["fid"], r["weight"]))
    evaluator.main(["-train", data] + _FLOW + ["-noeq", "-save", model2])
    evaluator.main(["-rank", data, "-load", model2, "-indri", run])
    head[2] = "## Train with enqueue: No"
    assert open(model2).read().split("\n")[:5] == head
    m = learning.RankerFactory().loadRankerFromFile(model2)
    assert isinstance(m, AdaRank) and m.rankers and set(m.rankers) == {1}
    p_rank = n_rank = 2 ** 31 - 1
    for line in open(run):
        row = line.split()
        assert row[1] == "Q0"
        rank, score = int(row[3]), float(row[4])
        assert np.isfinite(score) and rank > 0
        if row[2].startswith("P"):
            p_rank = min(rank, p_rank)
        else:
            n_rank = min(rank, n_rank)
    assert p_rank < n_rank and p_rank == 1


def test_prediction_with_repeated_fids():
    ada = learning.RankerFactory().loadRankerFromString("## AdaRank\n2:0.75 1:-1.5 2:0.125 3:1.0E-5")
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((37, 4)).astype(np.float32)
    rl = RankList([DataPoint("%d qid:1 %s" % (i % 2, " ".join("%d:%r" % (j + 1, float(rows[i, j])) for j in range(4))))
                   for i in range(37)])
    got = ada.evalList(rl)
    for i, dp in enumerate(rl.rl):
        s = 0.0
        for f, w in zip(ada.rankers, ada.rweight):
            s += w * float(dp.getFeatureValue(f))
        assert _bits(got[i]) == _bits(s)


def _letor(path, X, lab, qoff):
    with open(path, "w") as f:
        for q in range(len(qoff) - 1):
            for i in range(qoff[q], qoff[q + 1]):
                feats = " ".join("%d:%s" % (j + 1, repr(float(X[i, j]))) for j in range(X.shape[1]))
                f.write("%d qid:%d %s # d%d\n" % (int(lab[i]), q, feats, i))


def test_feature_subset_in_any_order_and_splits(tmp_path):
    """-feature in non-ascending order: the model text and the -score file are the restatement's, byte for byte; -kcv 3 -tvs 0.8 runs"""
    rng = np.random.default_rng(31)
    X, lab, qoff, _ = _data(rng, rng.integers(2, 20, 30), 6)
    data, feats, model, scores = (str(tmp_path / n) for n in ("d.txt", "f.txt", "m.txt", "s.txt"))
    _letor(data, X, lab, qoff)
    with open(feats, "w") as f:
        f.write("5\n2\n6\n")
    evaluator.main(["-train", data, "-ranker", "3", "-feature", feats, "-metric2t", "NDCG@5", "-round", "20", "-save", model])
    fids = (5, 2, 6)
    r = AR.learn((X[:, [f - 1 for f in fids]], lab, qoff, [str(q) for q in range(len(qoff) - 1)]), None, "NDCG", 5, nIteration=20)
    body = " ".join("%d:%s" % (fids[c], java_double_str(w)) for c, w in zip(r["fid"], r["weight"]))
    assert r["fid"] and open(model).read() == ("## AdaRank\n## Iteration = 20\n## Train with enqueue: Yes\n## Tolerance = 0.002\n"
                                               "## Max consecutive selection count = 5\n" + body)
    evaluator.main(["-load", model, "-rank", data, "-score", scores])
    want = []
    for i in range(X.shape[0]):
        s = 0.0
        for c, w in zip(r["fid"], r["weight"]):
            s += w * float(X[i, fids[c] - 1])
        want.append(s)
    rows = [line.rstrip("\n").split("\t") for line in open(scores)]
    assert [x[2] for x in rows] == [java_double_str(v) for v in want]
    evaluator.main(["-train", data, "-ranker", "3", "-kcv", "3", "-tvs", "0.8", "-metric2t", "MAP", "-round", "15"])


# ---- -qrel judgments, labels of 31 and above, fractional labels ---------------------------------------------------------------------
def _learn_or_refuse(tr, va, metric, k, rounds, arrays=None, ext=None):
    """The restatement says what must happen.  Its alpha_t is not finite (a list scoring above 1 can turn sum w (1 - m) negative): rlhip
    refuses with RL_ERR_UNSUPPORTED at that round and feature.  Otherwise: table, trace, model and scores are equal.  Returns the
    restatement's run, or None after a refusal."""
    t = _trainer(tr, va, metric, k, ext=arrays, n_iteration=rounds)
    try:
        r = AR.learn(tr, va, metric=metric, k=k, nIteration=rounds, **(ext or {}))
    except AR.NonFiniteAlpha as want:
        rnd, feat = str(want).split(",")[:2]
        with pytest.raises(N.RankLibError) as e:
            t.learn()
        assert "status -4" in str(e.value) and "AdaRank %s:" % rnd in str(e.value) and "feature index %s " % feat.split()[1] in str(e.value)
        return None
    t.learn()
    assert np.array_equal(t.weak_table().view(np.int64), r["M"].view(np.int64))
    g = [tuple(x.item()) for x in t.trace()]
    assert len(g) == len(r["trace"])
    for a, b in zip(g, r["trace"]):
        assert a[:4] == b[:4] and all(_bits(a[i]) == _bits(b[i]) for i in (4, 5, 6)), (a, b)
    fid, w = t.model()
    assert list(fid) == r["fid"] and [_bits(x) for x in w] == [_bits(x) for x in r["weight"]]
    ts, vs = t.scores()
    assert _bits(ts) == _bits(r["train"])
    if va is not None:
        assert _bits(vs) == _bits(r["valid"])
    return r


def _ext_case(metric):
    rng = np.random.default_rng(71)
    tr, va = E.shared_sets(rng, n_train=40)
    # ideals of at least every list's own: a smaller one scores a list above 1, where only the weak table is compared
    m = E.ideal_map([tr, va], 10, rng, (1.0, 2.0)) if metric == "NDCG" else E.count_map([tr, va], rng)
    return tr, va, m


@functools.lru_cache(maxsize=None)
def _plain(metric, k):
    """the restatement's run without judgments: computed once per metric, never changed"""
    tr, va, _ = _ext_case(metric)
    return AR.learn(tr, va, metric=metric, k=k, nIteration=18)


@pytest.mark.parametrize("where", ["train", "valid", "both"])
@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_external_judgments_match_the_restatement(metric, k, where):
    """external ideal DCGs (NaN for the qids without one) and relevant-document counts (0, own, larger) given to the training set, the
    validation set or both; a qid of both sets given through the validation set alone reaches the training list's score"""
    tr, va, m = _ext_case(metric)
    assert any(q in m for q in set(tr[3]) & set(va[3])) and any(q not in m for q in set(tr[3])) and any(q not in m for q in set(va[3]))
    arrays, ext = E.judgments(metric, m, tr, va, where)
    r = _learn_or_refuse(tr, va, metric, k, 18, arrays, ext)
    assert r is not None and sum(1 for x in r["trace"] if x[1] == AR.ROUND) >= 10
    plain = _plain(metric, k)
    assert r["trace"] != plain["trace"]
    if where != "valid" or metric == "NDCG":
        assert not np.array_equal(r["M"], plain["M"])


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_weak_table_external_judgments_across_the_length_classes(metric, k):
    """an external entry (ideals below, at and above the lists' own) on lists of every length class of k_ada_weak"""
    rng = np.random.default_rng(72)
    tr = E.data(rng, E.LENGTH_CLASSES, 3, levels=3, prefix="L")
    m = E.ideal_map([tr], 10, rng, missing=0.2) if metric == "NDCG" else E.count_map([tr], rng)
    n = np.diff(tr[2])
    for lo, hi in ((0, 16), (16, 384), (384, 5000), (5000, 1 << 30)):
        cls = [q for q in range(len(n)) if lo < n[q] <= hi]
        assert any(tr[3][q] in m and q != cls.index(q) for q in cls), (lo, hi)
    arrays, ext = E.judgments(metric, m, tr, None, "train")
    M = AR.weak_table(tr[0], tr[1], tr[2], tr[3], AR.CR.LiteralScorer(metric, k, **ext), metric, k)
    assert not np.array_equal(M, AR.weak_table(tr[0], tr[1], tr[2], tr[3], AR.CR.LiteralScorer(metric, k), metric, k))
    t = _trainer(tr, None, metric, k, ext=arrays, n_iteration=0)
    t.learn()
    assert np.array_equal(t.weak_table().view(np.int64), M.view(np.int64))


def _wrapped_sets(seed, sparse):
    """labels from {0, 1, 2, 31, 32, 33}; sparse: four documents of the training set hold one of 31, 32, 33"""
    rng = np.random.default_rng(seed)
    tr, va = E.shared_sets(rng, labels=(0, 1, 2) if sparse else E.WRAPPED, n_train=40)
    if sparse:
        idx = rng.choice(len(tr[1]), 4, replace=False)
        tr[1][idx] = rng.choice(np.array([31, 32, 33], np.float32), 4)
    return tr, va


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("DCG", 5), ("ERR", 10)])
def test_weak_table_wrapped_labels(metric, k):
    """gains 2147483647, 0 and 1 for labels 31, 32 and 33 (metric/DCGScorer.java:28-31,137-139; ERRScorer.java:71-73)"""
    tr, _ = _wrapped_sets(0, False)
    assert {31.0, 32.0, 33.0} <= set(tr[1].tolist())
    M = AR.weak_table(tr[0], tr[1], tr[2], tr[3], AR.CR.LiteralScorer(metric, k), metric, k)
    assert np.abs(M).max() > 1e6
    assert np.array_equal(_weak_gpu(tr, metric, k).view(np.int64), M.view(np.int64))


@pytest.mark.parametrize("metric,k,seed,sparse,refused", [
    ("NDCG", 10, 11, True, False),       # lists score up to 2.49 and every alpha stays finite: 14 rounds
    ("NDCG", 10, 0, False, True),        # sum w (1 - m) is negative on round 1
    ("ERR", 10, 7, True, False),
    ("ERR", 10, 0, False, True),
    ("DCG", 5, 0, False, True),
])
def test_learn_wrapped_labels(metric, k, seed, sparse, refused):
    tr, va = _wrapped_sets(seed, sparse)
    r = _learn_or_refuse(tr, va, metric, k, 15)
    assert (r is None) == refused
    if r is not None:
        assert sum(1 for x in r["trace"] if x[1] == AR.ROUND) >= 10 and (metric != "NDCG" or r["M"].max() > 1.0)


@pytest.mark.parametrize("metric,k", [("MAP", 0), ("P", 3), ("RR", 10), ("NDCG", 10)])
def test_fractional_labels(metric, k):
    """labels of 0.5, 1.5 and 2.99: relevant (label > 0) for MAP / P / RR, (int) label for NDCG"""
    rng = np.random.default_rng(74)
    tr, va = E.shared_sets(rng, labels=E.FRACTIONAL, n_train=40)
    assert {0.5, 1.5} <= set(tr[1].tolist())
    assert _learn_or_refuse(tr, va, metric, k, 18) is not None


def test_external_judgment_refusals():
    """rl_ada_set_external_judgments forwards to rl_ca_set_external_judgments; a later set_train discards the judgments"""
    rng = np.random.default_rng(75)
    tr = E.data(rng, [4, 5, 6, 3], 3)
    t, t2 = E.forwarded_refusals(lambda: N.AdaRankTrainer(metric="MAP", metric_k=0, n_iteration=2), tr, N.RankLibError)
    judged = AR.weak_table(tr[0], tr[1], tr[2], tr[3], AR.CR.LiteralScorer("MAP", 0, rel_doc_count=E.REFUSAL_MAP), "MAP", 0)
    plain = AR.weak_table(tr[0], tr[1], tr[2], tr[3], AR.CR.LiteralScorer("MAP", 0), "MAP", 0)
    assert not np.array_equal(judged, plain)
    assert np.array_equal(t.weak_table().view(np.int64), judged.view(np.int64))
    assert np.array_equal(t2.weak_table().view(np.int64), plain.view(np.int64))


@pytest.mark.parametrize("m2t", ["NDCG@10", "MAP"])
def test_cli_qrel_reaches_the_trainer(tmp_path, m2t):
    """-qrel <file> with -ranker 3: the saved model is the restatement's, fed the maps the host scorer loaded from the same file, and
    differs from the model trained without the judgments"""
    rng = np.random.default_rng(76)
    X, lab, qoff, _ = _data(rng, rng.integers(2, 25, 30), 4, labels=4)
    data, qrel, m_q, m_raw = (str(tmp_path / n) for n in ("d.txt", "qrel.txt", "q.txt", "raw.txt"))
    E.write_letor(data, X, lab, qoff)
    E.write_qrel(qrel, rng, np.diff(qoff))
    sc = MetricScorerFactory().createScorer(m2t)
    sc.loadExternalRelevanceJudgment(qrel)
    ext = dict(ideal=dict(sc.idealGains)) if m2t != "MAP" else dict(rel_doc_count=dict(sc.relDocCount))
    metric, k = ("MAP", 0) if m2t == "MAP" else ("NDCG", 10)
    train = (X, lab, qoff, [str(q) for q in range(len(qoff) - 1)])
    r, plain = AR.learn(train, None, metric, k, nIteration=15, **ext), AR.learn(train, None, metric, k, nIteration=15)
    assert r["fid"] and (r["fid"], r["weight"]) != (plain["fid"], plain["weight"])
    args = ["-train", data, "-ranker", "3", "-metric2t", m2t, "-round", "15"]
    evaluator.main(args + ["-qrel", qrel, "-save", m_q])
    evaluator.main(args + ["-save", m_raw])
    assert evaluator.Evaluator.qrelFile == ""
    head = "## AdaRank\n## Iteration = 15\n## Train with enqueue: Yes\n## Tolerance = 0.002\n## Max consecutive selection count = 5\n"
    body = lambda m: " ".join("%d:%s" % (f + 1, java_double_str(w)) for f, w in zip(m["fid"], m["weight"]))      # noqa: E731
    assert open(m_q).read() == head + body(r)
    assert open(m_raw).read() == head + body(plain)
