"""RankBoost (-ranker 2) on the MI355X: every round's feature, threshold, maxR, R_t, alpha_t, Z_t, train and validation score, the model and
the final scores bit-identical to the literal restatement of RankBoost.init / learn (tests/rb_restatement.py); the potentials (device-only
state) bit-identical too; the length classes; the refusals; and the reference's testRanker flow for ranker 2 through the command line.

-qrel judgments are covered by test_external_judgments_match_the_restatement (per set), test_cli_qrel_reaches_the_trainer and
test_external_judgment_refusals; labels of 31 and above (gains that wrap as Java ints) by test_wrapped_labels; fractional labels, which
the crucial pairs and getCorrectRanking() compare as floats (RankBoost.java:157,173; RankList.java:84-90), by test_fractional_labels."""
import functools

import numpy as np
import pytest

import linear_ext as E
import rb_restatement as RB
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd.learning import AdaRank, DataPoint, LambdaMART, RankBoost, RankList, java_double_str
from ranklib_amd.metric import ERRScorer, MetricScorerFactory

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = (RankBoost.nIteration, RankBoost.nThreshold, RankBoost.device, AdaRank.nIteration, LambdaMART.nThreshold, ERRScorer.MAX,
             learning.RFRanker.featureSamplingRate, learning.RFRanker.nBag)
    RankBoost.nIteration, RankBoost.nThreshold = 300, 10      # the Java's defaults, whatever an earlier test's command line left
    yield
    (RankBoost.nIteration, RankBoost.nThreshold, RankBoost.device, AdaRank.nIteration, LambdaMART.nThreshold, ERRScorer.MAX,
     learning.RFRanker.featureSamplingRate, learning.RFRanker.nBag) = saved


def _data(rng, lengths, F, levels=3, labels=3):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    X = (rng.integers(0, levels, (qoff[-1], F)).astype(np.float32) * np.float32(0.37)).astype(np.float32)
    X[rng.random(X.shape) < 0.1] = 0.0
    lab = rng.integers(0, labels, qoff[-1]).astype(np.float32)
    return X, lab, qoff, ["q%d" % i for i in range(len(lengths))]


def _trainer(train, valid=None, metric="NDCG", k=10, err_max=16.0, ext=None, **p):
    """ext: the per-list external judgments of linear_ext.feed (ideal_tr / ideal_va / rdc_tr / rdc_va)"""
    return E.feed(N.RankBoostTrainer(metric=metric, metric_k=k, err_max=err_max, **p), train, valid, **(ext or {}))


def _bits(v):
    return np.float64(v).tobytes()


def _events(r, n_iteration):
    ev = set()
    if any(t[0] == n_iteration for t in r["trace"]):
        ev.add("ROUND LIMIT")
    if r["restored"]:
        ev.add("BEST ON VALIDATION")
    fids = [t[1] for t in r["trace"]]
    if len(set(fids)) < len(fids):
        ev.add("FEATURE AGAIN")
    return ev


def _assert_same_run(t, r, valid):
    g = [tuple(x.item()) for x in t.trace()]
    assert len(g) == len(r["trace"])
    for a, b in zip(g, r["trace"]):
        assert a[:2] == b[:2] and all(_bits(a[i]) == _bits(b[i]) for i in range(2, 9)), (a, b)
    fid, thr, w = t.model()
    assert list(fid) == r["fid"]
    assert [_bits(x) for x in thr] == [_bits(x) for x in r["thr"]] and [_bits(x) for x in w] == [_bits(x) for x in r["weight"]]
    ts, vs = t.scores()
    assert _bits(ts) == _bits(r["train"])
    if valid:
        assert _bits(vs) == _bits(r["valid"])


# (metric, k, -gmax, validation, -tc, -round, value levels, seed, events the case must cover)
_ALL = {"ROUND LIMIT", "BEST ON VALIDATION", "FEATURE AGAIN"}
_CASES = [
    ("NDCG", 10, 16.0, True, 10, 25, 3, 0, _ALL),
    ("NDCG", 10, 16.0, False, -1, 25, 7, 1, {"ROUND LIMIT", "FEATURE AGAIN"}),
    ("DCG", 3, 16.0, True, 3, 25, 7, 1, _ALL),
    ("DCG", 1, 16.0, False, 10, 25, 3, 2, {"ROUND LIMIT", "FEATURE AGAIN"}),
    ("MAP", 0, 16.0, True, -1, 25, 3, 2, _ALL),
    ("MAP", 0, 16.0, False, 3, 25, 7, 3, {"ROUND LIMIT", "FEATURE AGAIN"}),
    ("ERR", 10, 8.0, True, 10, 30, 7, 3, _ALL),
    ("ERR", 5, 16.0, False, -1, 25, 3, 4, {"ROUND LIMIT", "FEATURE AGAIN"}),
    ("P", 5, 16.0, True, 3, 25, 3, 4, _ALL),
    ("P", 3, 16.0, False, 10, 25, 7, 5, {"ROUND LIMIT", "FEATURE AGAIN"}),
    ("RR", 10, 16.0, True, -1, 25, 7, 5, _ALL),
    ("RR", 10, 16.0, False, 3, 25, 3, 0, {"ROUND LIMIT", "FEATURE AGAIN"}),
]


@pytest.mark.parametrize("case", _CASES, ids=["%s%d-%s-tc%d" % (c[0], c[1], "valid" if c[3] else "novalid", c[4]) for c in _CASES])
def test_trace_parity_with_the_restatement(case):
    metric, k, gmax, valid, tc, rounds, levels, seed, expect = case
    rng = np.random.default_rng(seed)
    tr = _data(rng, rng.integers(1, 25, 30), 5, levels=levels)
    va = _data(rng, rng.integers(1, 25, 30), 5, levels=levels) if valid else None
    r = RB.learn(tr, va, metric=metric, k=k, nIteration=rounds, nThreshold=tc, err_max=gmax)
    assert expect <= _events(r, rounds), _events(r, rounds)
    t = _trainer(tr, va, metric, k, gmax, n_iteration=rounds, n_threshold=tc)
    t.learn()
    _assert_same_run(t, r, valid)


@pytest.mark.parametrize("tc", [10, -1])
def test_potentials_after_rounds_1_and_5(tc):
    rng = np.random.default_rng(11)
    tr = _data(rng, rng.integers(1, 25, 30), 5, levels=7)
    r = RB.learn(tr, None, "NDCG", 10, nIteration=6, nThreshold=tc, keep_potentials=5)
    t = _trainer(tr, None, "NDCG", 10, n_iteration=6, n_threshold=tc, keep_potentials=5)
    t.learn()
    for rnd in (1, 5):
        assert np.array_equal(t.potentials(rnd).view(np.int64), r["pots"][rnd - 1].view(np.int64)), rnd
    assert np.any(r["pots"][0] != r["pots"][4])
    with pytest.raises(N.RankLibError):
        t.potentials(6)


@pytest.mark.parametrize("metric,k,tc,levels,labels", [("NDCG", 10, 10, 3, 3), ("MAP", 0, -1, 3, 2), ("ERR", 20, 3, 1000, 5)])
def test_length_classes(metric, k, tc, levels, labels):
    """lists of 1, 2, 16, 17, 384, 385 and 5 003 documents (every class of the ranking kernel, several tiles of both staged chains), heavy
    ties in labels and values, and single-label lists, which hold no pair"""
    rng = np.random.default_rng(23)
    lengths = np.array([1, 2, 16, 17, 9, 384, 385, 5003, 12])
    tr = list(_data(rng, lengths, 3, levels=levels, labels=labels))
    tr[1][int(tr[2][4]):int(tr[2][5])] = 1.0                 # the list of 9: one label
    tr[1][int(tr[2][8]):int(tr[2][9])] = 0.0                 # the list of 12: no relevant document
    rounds = 3
    r = RB.learn(tr, None, metric, k, nIteration=rounds, nThreshold=tc, vector=True, keep_potentials=rounds)
    assert len(r["trace"]) == rounds
    t = _trainer(tr, None, metric, k, n_iteration=rounds, n_threshold=tc, keep_potentials=rounds)
    t.learn()
    for rnd in range(1, rounds + 1):
        assert np.array_equal(t.potentials(rnd).view(np.int64), r["pots"][rnd - 1].view(np.int64)), rnd
    _assert_same_run(t, r, False)


def test_refusals():
    rng = np.random.default_rng(2)
    X, lab, qoff, qid = _data(rng, [4, 5, 6], 3)
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[4, 1] = bad
        with pytest.raises(N.RankLibError):
            N.RankBoostTrainer().set_train(Xb, lab, qoff)
    with pytest.raises(N.RankLibError):
        N.RankBoostTrainer(metric="BEST")
    same = np.array([1, 1, 1, 1, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2], np.float32)      # every list holds one label: no crucial pair
    with pytest.raises(RB.NonFiniteRound):
        RB.learn((X, same, qoff, qid), None, "NDCG", 10)
    t = _trainer((X, same, qoff, qid))
    with pytest.raises(N.RankLibError) as e:
        t.learn()
    assert "no crucial pair" in str(e.value)
    lab = np.array([1, 0, 1, 0, 0, 1], np.float32)                      # feature 0 orders every pair correctly
    Xp = np.array([[1.0, 0.3], [0.0, 0.9], [1.0, 0.1], [0.0, 0.5], [0.2, 0.5], [0.7, 0.4]], np.float32)
    qoff = np.array([0, 2, 4, 6], np.int32)
    with pytest.raises(RB.NonFiniteRound) as want:
        RB.learn((Xp, lab, qoff, ["a", "b", "c"]), None, "MAP", 0)
    t = _trainer((Xp, lab, qoff, ["a", "b", "c"]), None, "MAP", 0)
    with pytest.raises(N.RankLibError) as e:
        t.learn()
    assert "RankBoost round %d:" % want.value.round in str(e.value) and "feature index 0" in str(e.value)
    assert len(t.trace()) == want.value.round - 1


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


def _read_count_data(path):
    rows = [line.split() for line in open(path)]
    X = np.array([[float(r[2][2:]), float(r[3][2:])] for r in rows], np.float32)
    lab = np.array([float(r[0]) for r in rows], np.float32)
    qs = [r[1][4:] for r in rows]
    qoff = np.array([0] + [i for i in range(1, len(qs)) if qs[i] != qs[i - 1]] + [len(qs)], np.int32)
    return X, lab, qoff, [qs[a] for a in qoff[:-1]]


_FLOW = ["-metric2t", "map", "-ranker", "2", "-frate", "1.0", "-bag", "10", "-round", "10", "-epoch", "10"]


def test_reference_testRanker_flow_is_refused_on_separable_data(tmp_path):
    """test:eval/EvaluatorTest.java:207-220 with rnum = 2 (testRankBoost is @Ignore'd there, "Fails with NaN"): feature 1 orders every pair,
    maxR is 1 - 1e-14 on round 1 and alpha_t finite; round 2 has a non-positive (Z + R) / (Z - R)"""
    data, model = str(tmp_path / "data.txt"), str(tmp_path / "model.txt")
    _write_count_data(data, 20, 20)
    with pytest.raises(RB.NonFiniteRound) as want:
        RB.learn(_read_count_data(data), None, "MAP", 0, nIteration=10)
    with pytest.raises(N.RankLibError) as e:
        evaluator.main(["-train", data] + _FLOW + ["-save", model])
    assert "RankBoost round %d:" % want.value.round in str(e.value) and "alpha_t" in str(e.value)


def test_reference_testRanker_flow_with_flipped_labels(tmp_path):
    """the same flow on data that trains: the saved model is the restatement's, and the -rank -indri check of testRanker (:222-259) holds
    line by line: a P document at rank 1, no N document above it"""
    data, model, run = (str(tmp_path / n) for n in ("data.txt", "model.txt", "run.txt"))
    _write_count_data(data, 20, 20, flip=0.1, seed=4)
    evaluator.main(["-train", data] + _FLOW + ["-save", model])
    r = RB.learn(_read_count_data(data), None, "MAP", 0, nIteration=10)
    assert len(r["fid"]) == 10
    head = "## RankBoost\n## Iteration = 10\n## No. of threshold candidates = 10\n"
    assert open(model).read() == head + " ".join("%d:%s:%s" % (f + 1, java_double_str(t), java_double_str(w))
                                                  for f, t, w in zip(r["fid"], r["thr"], r["weight"]))
    evaluator.main(["-rank", data, "-load", model, "-indri", run])
    m = learning.RankerFactory().loadRankerFromFile(model)
    assert isinstance(m, RankBoost) and len(m.wRankers) == 10
    p_rank = n_rank = 2 ** 31 - 1
    n_lines = 0
    for line in open(run):
        row = line.split()
        assert row[1] == "Q0"
        rank, score = int(row[3]), float(row[4])
        assert np.isfinite(score) and rank > 0
        if row[2].startswith("P"):
            p_rank = min(rank, p_rank)
        else:
            n_rank = min(rank, n_rank)
        assert p_rank < n_rank and p_rank == 1, line
        n_lines += 1
    assert n_lines == 800


def test_prediction_with_repeated_fids():
    rb = learning.RankerFactory().loadRankerFromString("## RankBoost\n2:0.25:0.75 1:-0.5:-1.5 2:1.0:0.125 3:0.0:1.0E-5")
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((37, 4)).astype(np.float32)
    rl = RankList([DataPoint("%d qid:1 %s" % (i % 2, " ".join("%d:%r" % (j + 1, float(rows[i, j])) for j in range(4))))
                   for i in range(37)])
    got = rb.evalList(rl)
    for i, dp in enumerate(rl.rl):
        s = 0.0
        for (f, thr), w in zip(rb.wRankers, rb.rWeight):
            s += w * (1 if float(dp.getFeatureValue(f)) > thr else 0)
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
    X, lab, qoff, _ = _data(rng, rng.integers(2, 20, 30), 6, levels=7)
    data, feats, model, scores = (str(tmp_path / n) for n in ("d.txt", "f.txt", "m.txt", "s.txt"))
    _letor(data, X, lab, qoff)
    with open(feats, "w") as f:
        f.write("5\n2\n6\n")
    evaluator.main(["-train", data, "-ranker", "2", "-feature", feats, "-metric2t", "NDCG@5", "-round", "20", "-tc", "4", "-save", model])
    fids = (5, 2, 6)
    r = RB.learn((X[:, [f - 1 for f in fids]], lab, qoff, [str(q) for q in range(len(qoff) - 1)]), None, "NDCG", 5, nIteration=20,
                 nThreshold=4)
    body = " ".join("%d:%s:%s" % (fids[c], java_double_str(t), java_double_str(w)) for c, t, w in zip(r["fid"], r["thr"], r["weight"]))
    assert r["fid"] and open(model).read() == "## RankBoost\n## Iteration = 20\n## No. of threshold candidates = 4\n" + body
    evaluator.main(["-load", model, "-rank", data, "-score", scores])
    want = []
    for i in range(X.shape[0]):
        s = 0.0
        for c, t, w in zip(r["fid"], r["thr"], r["weight"]):
            s += w * (1 if float(X[i, fids[c] - 1]) > t else 0)
        want.append(s)
    rows = [line.rstrip("\n").split("\t") for line in open(scores)]
    assert [x[2] for x in rows] == [java_double_str(v) for v in want]
    evaluator.main(["-train", data, "-ranker", "2", "-kcv", "3", "-tvs", "0.8", "-metric2t", "MAP", "-round", "15"])
    evaluator.main(["-train", data, "-ranker", "2", "-tvs", "0.8", "-metric2t", "NDCG@10", "-round", "15", "-tc", "-1"])


# ---- -qrel judgments, labels of 31 and above, fractional labels ---------------------------------------------------------------------
def _ext_case(metric):
    rng = np.random.default_rng(81)
    tr, va = E.shared_sets(rng)
    m = E.ideal_map([tr, va], 10, rng) if metric == "NDCG" else E.count_map([tr, va], rng)
    return tr, va, m


@functools.lru_cache(maxsize=None)
def _plain(metric, k):
    """the restatement's run without judgments: computed once per metric, never changed"""
    tr, va, _ = _ext_case(metric)
    return RB.learn(tr, va, metric=metric, k=k, nIteration=15)


@pytest.mark.parametrize("where", ["train", "valid", "both"])
@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_external_judgments_match_the_restatement(metric, k, where):
    """external ideal DCGs (NaN for the qids without one; below, at and above the lists' own) and relevant-document counts (0, own, larger)
    given to the training set, the validation set or both: every round's train and validation score, and the best prefix on validation data"""
    tr, va, m = _ext_case(metric)
    assert any(q in m for q in set(tr[3]) & set(va[3])) and any(q not in m for q in set(tr[3])) and any(q not in m for q in set(va[3]))
    arrays, ext = E.judgments(metric, m, tr, va, where)
    r = RB.learn(tr, va, metric=metric, k=k, nIteration=15, **ext)
    plain = _plain(metric, k)
    assert len(r["trace"]) == 15
    if where != "train" or metric == "NDCG":                 # counts stay with their set; an ideal DCG is cached for both
        assert [x[8] for x in r["trace"]] != [x[8] for x in plain["trace"]]
    if where != "valid" or metric == "NDCG":                 # (valid, NDCG): a qid of both sets, given through the validation set alone
        assert [x[7] for x in r["trace"]] != [x[7] for x in plain["trace"]]
    t = _trainer(tr, va, metric, k, ext=arrays, n_iteration=15)
    t.learn()
    _assert_same_run(t, r, True)


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("DCG", 5), ("ERR", 10)])
def test_wrapped_labels(metric, k):
    """labels of 31, 32 and 33: gains 2147483647, 0 and 1 (metric/DCGScorer.java:28-31,137-139; ERRScorer.java:71-73), while the pairs
    compare the labels themselves"""
    rng = np.random.default_rng(83)
    tr, va = E.shared_sets(rng, labels=E.WRAPPED)
    assert {31.0, 32.0, 33.0} <= set(tr[1].tolist())
    r = RB.learn(tr, va, metric=metric, k=k, nIteration=15)
    assert len(r["trace"]) == 15 and max(abs(x[7]) for x in r["trace"]) > (1e6 if metric != "NDCG" else 1.0)
    t = _trainer(tr, va, metric, k, n_iteration=15)
    t.learn()
    _assert_same_run(t, r, True)


@pytest.mark.parametrize("metric,k", [("MAP", 0), ("P", 3), ("RR", 10), ("NDCG", 10)])
def test_fractional_labels(metric, k):
    """labels of 0.5, 1.5 and 2.99: (0.5, 0) and (2.99, 2) are crucial pairs -- the potentials of round 1 say so directly -- and a 0.5 is
    relevant for MAP / P / RR, gain 0 for NDCG"""
    rng = np.random.default_rng(84)
    tr, va = E.shared_sets(rng, labels=E.FRACTIONAL)
    assert {0.5, 1.5} <= set(tr[1].tolist())
    r = RB.learn(tr, va, metric=metric, k=k, nIteration=15, keep_potentials=1)
    trunc = (tr[0], np.floor(tr[1]), tr[2], tr[3])           # the same lists with (int) labels hold fewer crucial pairs
    assert not np.array_equal(RB.learn(trunc, None, metric=metric, k=k, nIteration=1, keep_potentials=1)["pots"][0], r["pots"][0])
    t = _trainer(tr, va, metric, k, n_iteration=15, keep_potentials=1)
    t.learn()
    assert np.array_equal(t.potentials(1).view(np.int64), r["pots"][0].view(np.int64))
    _assert_same_run(t, r, True)


def test_external_judgment_refusals():
    """rl_rb_set_external_judgments forwards to rl_ca_set_external_judgments; a later set_train discards the judgments"""
    rng = np.random.default_rng(85)
    tr = E.data(rng, [4, 5, 6, 3], 3)
    t, t2 = E.forwarded_refusals(lambda: N.RankBoostTrainer(metric="MAP", metric_k=0, n_iteration=2), tr, N.RankLibError)
    judged, plain = RB.learn(tr, None, "MAP", 0, nIteration=2, rel_doc_count=E.REFUSAL_MAP), RB.learn(tr, None, "MAP", 0, nIteration=2)
    assert judged["train"] != plain["train"]
    _assert_same_run(t, judged, False)
    _assert_same_run(t2, plain, False)


@pytest.mark.parametrize("m2t", ["NDCG@10", "MAP"])
def test_cli_qrel_reaches_the_trainer(tmp_path, m2t):
    """-qrel <file> with -ranker 2 and -validate (the judgments reach a RankBoost model through the best prefix on validation data only):
    the saved model is the restatement's, fed the maps the host scorer loaded from the same file, and differs from the model trained
    without the judgments"""
    rng = np.random.default_rng(86)
    tr = E.data(rng, rng.integers(2, 25, 30), 4, (0, 1, 2, 3), levels=7)
    va = E.data(rng, rng.integers(2, 25, 12), 4, (0, 1, 2, 3), levels=7)
    data, vdata, qrel, m_q, m_raw = (str(tmp_path / n) for n in ("d.txt", "v.txt", "qrel.txt", "q.txt", "raw.txt"))
    E.write_letor(data, *tr[:3])
    E.write_letor(vdata, *va[:3], qid0=30)                   # the validation qids go on from the training file's: 30 .. 41
    E.write_qrel(qrel, rng, np.concatenate([np.diff(tr[2]), np.diff(va[2])]))
    sc = MetricScorerFactory().createScorer(m2t)
    sc.loadExternalRelevanceJudgment(qrel)
    ext = dict(ideal=dict(sc.idealGains)) if m2t != "MAP" else dict(rel_doc_count=dict(sc.relDocCount))
    metric, k = ("MAP", 0) if m2t == "MAP" else ("NDCG", 10)
    train, valid = tr[:3] + ([str(q) for q in range(30)],), va[:3] + ([str(q + 30) for q in range(12)],)
    r, plain = RB.learn(train, valid, metric, k, nIteration=15, **ext), RB.learn(train, valid, metric, k, nIteration=15)
    assert r["fid"] and len(r["fid"]) != len(plain["fid"])
    args = ["-train", data, "-validate", vdata, "-ranker", "2", "-metric2t", m2t, "-round", "15"]
    evaluator.main(args + ["-qrel", qrel, "-save", m_q])
    evaluator.main(args + ["-save", m_raw])
    assert evaluator.Evaluator.qrelFile == ""
    head = "## RankBoost\n## Iteration = 15\n## No. of threshold candidates = 10\n"
    body = lambda m: " ".join("%d:%s:%s" % (f + 1, java_double_str(t), java_double_str(w))      # noqa: E731
                              for f, t, w in zip(m["fid"], m["thr"], m["weight"]))
    assert open(m_q).read() == head + body(r)
    assert open(m_raw).read() == head + body(plain)
