"""Coordinate Ascent (-ranker 4) on the MI355X: every trial's score, the weights, the scores and the model text bit-identical to the
numpy restatement of CoorAscent.learn (tests/ca_restatement.py), and the reference's own testCoorAscent / testRanker flows.

-qrel judgments (external ideal DCGs and relevant-document counts, per set, per length class, through the command line, and what
rl_ca_set_external_judgments refuses) are covered by test_external_judgments_*, test_cli_qrel_reaches_the_trainer and
test_external_judgment_refusals_and_lifetime; labels of 31 and above, whose gain wraps as a Java int, by test_wrapped_labels; fractional
labels, relevant for MAP / P / RR and truncated for NDCG / DCG / ERR, by test_fractional_labels."""
import functools

import numpy as np
import pytest

import ca_restatement as CR
import linear_ext as E
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd.learning import CoorAscent, java_double_str
from ranklib_amd.metric import ERRScorer, MetricScorerFactory
from test_host_mirror import write_random_data

pytestmark = pytest.mark.gpu

_STATICS = ("nRestart", "nMaxIteration", "stepBase", "stepScale", "tolerance", "regularized", "slack", "seed", "device")


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = {k: getattr(CoorAscent, k) for k in _STATICS}
    gmax, rf_seed, fh_seed = ERRScorer.MAX, learning.RFRanker.seed, learning.FeatureHistogram.seed
    yield
    for k, v in saved.items():
        setattr(CoorAscent, k, v)
    ERRScorer.MAX, learning.RFRanker.seed, learning.FeatureHistogram.seed = gmax, rf_seed, fh_seed


def _data(rng, lengths, F, levels=4, labels=3):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    X = (rng.integers(0, levels, (qoff[-1], F)).astype(np.float32) * np.float32(0.37)).astype(np.float32)
    X[rng.random(X.shape) < 0.1] = 0.0                           # exact zeros: ties and -0.0 / +0.0 chains
    lab = rng.integers(0, labels, qoff[-1]).astype(np.float32)
    return X, lab, qoff


def _gpu(train, valid=None, metric="NDCG", k=10, err_max=16.0, ext=None, **p):
    """ext: the per-list external judgments of linear_ext.feed (ideal_tr / ideal_va / rdc_tr / rdc_va)"""
    t = N.CoorAscentTrainer(metric=metric, metric_k=k, err_max=err_max, **{_ARG[a]: v for a, v in p.items()})
    E.feed(t, train, valid, **(ext or {}))
    t.learn()
    ts, vs = t.scores()
    return dict(weight=list(t.weights()), train=ts, valid=vs, trace=[tuple(r.item()) for r in t.trace()])


_ARG = dict(nRestart="n_restart", nMaxIteration="n_max_iteration", stepBase="step_base", stepScale="step_scale", tolerance="tolerance",
            regularized="regularized", slack="slack", seed="seed")


def _same(g, r):
    assert len(g["trace"]) == len(r["trace"])
    for a, b in zip(g["trace"], r["trace"]):
        assert a[:6] == b[:6] and np.float64(a[6]).tobytes() == np.float64(b[6]).tobytes() \
            and np.float64(a[7]).tobytes() == np.float64(b[7]).tobytes(), (a, b)
    assert np.array_equal(np.array(g["weight"]).view(np.int64), np.array(r["weight"]).view(np.int64))
    assert np.float64(g["train"]).tobytes() == np.float64(r["train"]).tobytes()
    if r["valid"] is not None:
        assert np.float64(g["valid"]).tobytes() == np.float64(r["valid"]).tobytes()


@pytest.mark.parametrize("metric,k,err_max,valid,extra", [
    ("NDCG", 10, 16.0, True, {}),
    ("DCG", 5, 16.0, False, {}),
    ("MAP", 0, 16.0, True, dict(regularized=True, slack=0.01)),
    ("ERR", 10, 8.0, True, {}),                    # -gmax 3
    ("P", 5, 16.0, False, dict(seed=7)),
    ("RR", 10, 16.0, True, {}),
    ("NDCG", 10, 16.0, False, dict(nMaxIteration=70)),     # more trials than one launch takes: the chain continues across launches
])
def test_trace_parity_with_the_restatement(metric, k, err_max, valid, extra):
    rng = np.random.default_rng(11)
    tr = _data(rng, rng.integers(1, 30, 40), 5)
    qid = ["q%d" % (i % 33) for i in range(40)]                  # repeated qids: the NDCG ideal-DCG cache quirk
    train = tr + (qid,)
    va = None
    if valid:
        v = _data(rng, rng.integers(1, 20, 15), 5)
        va = v + (["q%d" % (i + 25) for i in range(15)],)           # some validation qids also name training lists
    p = dict(nRestart=2, nMaxIteration=12, tolerance=0.001, seed=3)
    p.update(extra)
    g = _gpu(train, va, metric, k, err_max, **p)
    r = CR.learn(train, va, metric, k, err_max=err_max, **p)
    _same(g, r)
    assert sum(1 for t in r["trace"] if t[0] == CR.TRIAL) > 100


def test_single_feature_and_small_weights():
    rng = np.random.default_rng(5)
    tr = _data(rng, rng.integers(2, 12, 20), 1) + (["a%d" % i for i in range(20)],)
    p = dict(nRestart=2, nMaxIteration=8, seed=1)
    _same(_gpu(tr, None, "NDCG", 10, **p), CR.learn(tr, None, "NDCG", 10, **p))
    # 520 features: every weight starts below 0.002, where the step becomes stepBase * |w| -- upward even for dir = -1 (point 4)
    tr = _data(rng, rng.integers(2, 8, 10), 520) + (["b%d" % i for i in range(10)],)
    p = dict(nRestart=1, nMaxIteration=3, seed=2, tolerance=1.0)
    r = CR.learn(tr, None, "MAP", 0, **p)
    w0 = float(np.float32(1.0) / np.float32(520))
    assert any(t[0] == CR.TRIAL and t[3] == -1 and t[6] > w0 for t in r["trace"])
    _same(_gpu(tr, None, "MAP", 0, **p), r)


def test_length_classes():
    """lists of <= 16, <= 384, <= 5000 and more documents in one set: every length class of k_ca_trials"""
    rng = np.random.default_rng(9)
    lengths = [3, 16, 17, 120, 384, 385, 1500, 5000, 5001, 7000] + list(rng.integers(1, 40, 30))
    tr = _data(rng, lengths, 4, levels=6) + (["L%d" % i for i in range(len(lengths))],)
    p = dict(nRestart=1, nMaxIteration=5, seed=4)
    for metric, k in (("NDCG", 10), ("ERR", 10)):
        _same(_gpu(tr, None, metric, k, **p), CR.learn(tr, None, metric, k, **p))


def test_infinite_feature_value_is_refused():
    rng = np.random.default_rng(1)
    X, lab, qoff = _data(rng, [4, 5], 3)
    X[2, 1] = np.inf
    t = N.CoorAscentTrainer()
    with pytest.raises(N.RankLibError) as e:
        t.set_train(X, lab, qoff)
    assert "Infinity" in str(e.value)


def test_reference_testCoorAscent_verbatim(tmp_path):
    """test:eval/EvaluatorTest.java:34-62"""
    data, model = str(tmp_path / "data.txt"), str(tmp_path / "model.txt")
    write_random_data(data)
    evaluator.main(["-train", data, "-metric2t", "map", "-ranker", "4", "-save", model])
    m = learning.RankerFactory().loadRankerFromFile(model)
    assert isinstance(m, CoorAscent)
    assert m.weight[0] > m.weight[1]
    assert m.weight[0] > 0.9
    assert m.weight[1] < 0.1


def test_reference_test_flow_ranker4(tmp_path):
    """testRanker (test:eval/EvaluatorTest.java:207-260) for -ranker 4, flag for flag"""
    data, model, run = (str(tmp_path / n) for n in ("data.txt", "model.txt", "run.txt"))
    write_random_data(data)
    evaluator.main(["-train", data, "-metric2t", "map", "-ranker", "4", "-frate", "1.0", "-bag", "10", "-round", "10",
                    "-epoch", "10", "-save", model])
    evaluator.main(["-rank", data, "-load", model, "-indri", run])
    assert open(model).read().startswith("## Coordinate Ascent\n## Restart = 5\n## MaxIteration = 25\n## StepBase = 0.05\n")
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


def _letor(path, X, lab, qoff):
    with open(path, "w") as f:
        for q in range(len(qoff) - 1):
            for i in range(qoff[q], qoff[q + 1]):
                feats = " ".join("%d:%s" % (j + 1, repr(float(X[i, j]))) for j in range(X.shape[1]))
                f.write("%d qid:%d %s # d%d\n" % (int(lab[i]), q, feats, i))


def test_default_ranker_feature_subset_model_text_and_score_file(tmp_path):
    """no -ranker trains Coordinate Ascent; -feature / -r / -i / -seed reach it; the model text and the -score file are the
    restatement's, byte for byte"""
    rng = np.random.default_rng(21)
    X, lab, qoff = _data(rng, rng.integers(2, 25, 30), 6)
    data, feat, model, sc = (str(tmp_path / n) for n in ("d.txt", "f.txt", "m.txt", "s.txt"))
    _letor(data, X, lab, qoff)
    with open(feat, "w") as f:
        f.write("2\n5\n3\n")
    evaluator.main(["-train", data, "-metric2t", "NDCG@10", "-feature", feat, "-r", "2", "-i", "10", "-seed", "5", "-save", model])
    cols = [1, 4, 2]
    r = CR.learn((X[:, cols], lab, qoff, [str(q) for q in range(len(qoff) - 1)]), None, "NDCG", 10, nRestart=2, nMaxIteration=10, seed=5)
    body = " ".join("%d:%s" % (f, java_double_str(w)) for f, w in zip((2, 5, 3), r["weight"]))
    assert open(model).read() == ("## Coordinate Ascent\n## Restart = 2\n## MaxIteration = 10\n## StepBase = 0.05\n## StepScale = 2.0\n"
                                  "## Tolerance = 0.001\n## Regularized = false\n## Slack = 0.001\n" + body)
    evaluator.main(["-load", model, "-rank", data, "-score", sc])
    Xr = np.zeros((X.shape[0], 7), np.float32)
    Xr[:, 1:] = X
    want = CR.dot_scores(Xr, (2, 5, 3), r["weight"])
    rows = [l.rstrip("\n").split("\t") for l in open(sc)]
    assert [x[2] for x in rows] == [java_double_str(v) for v in want]


def test_kcv_and_validation_flows(tmp_path):
    rng = np.random.default_rng(33)
    X, lab, qoff = _data(rng, rng.integers(2, 20, 24), 4)
    data = str(tmp_path / "d.txt")
    _letor(data, X, lab, qoff)
    CoorAscent.nRestart, CoorAscent.nMaxIteration = 1, 8
    e = evaluator.Evaluator(learning.RankerType.COOR_ASCENT, "NDCG@10", "NDCG@10")
    scores = e.evaluate_kcv(data, None, 3)
    assert len(scores) == 3 and all(0.0 <= a <= 1.0 and 0.0 <= b <= 1.0 for a, b in scores)
    ranker, s = e.evaluate_tvs(data, 0.7, data, None, None)
    assert isinstance(ranker, CoorAscent) and 0.0 <= s <= 1.0 and ranker.getScoreOnValidationData() > 0.0


# ---- -qrel judgments, labels of 31 and above, fractional labels ---------------------------------------------------------------------
_P_EXT = dict(nRestart=2, nMaxIteration=12, seed=3)


def _ext_case(metric):
    rng = np.random.default_rng(61)
    tr, va = E.shared_sets(rng)
    m = E.ideal_map([tr, va], 10, rng) if metric == "NDCG" else E.count_map([tr, va], rng)
    return tr, va, m


@functools.lru_cache(maxsize=None)
def _plain(metric, k):
    """the restatement's run without judgments: computed once per metric, never changed"""
    tr, va, _ = _ext_case(metric)
    return CR.learn(tr, va, metric, k, **_P_EXT)


@pytest.mark.parametrize("where", ["train", "valid", "both"])
@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_external_judgments_match_the_restatement(metric, k, where):
    """external ideal DCGs (NaN for the qids without one; below, at and above the lists' own) and relevant-document counts (0, own, larger)
    given to the training set, the validation set or both.  Given to the validation set only, the entry of a qid both sets hold is in the
    ideal-DCG cache before the training list is scored (NDCGScorer.java:114-122); the counts stay with the set they were given to."""
    tr, va, m = _ext_case(metric)
    shared = set(tr[3]) & set(va[3])
    assert any(q in m for q in shared) and any(q not in m for q in set(tr[3])) and any(q not in m for q in set(va[3]))
    if metric == "NDCG":
        nan = np.isnan(E.per_list(m, tr[3], "ideal"))
        assert len(tr[3]) // 4 <= nan.sum() <= len(tr[3]) // 2
    else:
        assert 0 in m.values() and sum(1 for v in m.values() if v > 0) >= 10
    arrays, ext = E.judgments(metric, m, tr, va, where)
    r = CR.learn(tr, va, metric, k, **_P_EXT, **ext)
    plain = _plain(metric, k)
    assert r["trace"] != plain["trace"]
    if where != "valid" or metric == "NDCG":                 # the very first score of the training set already differs
        assert r["trace"][0][7] != plain["trace"][0][7]
    _same(_gpu(tr, va, metric, k, ext=arrays, **_P_EXT), r)


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_external_judgments_across_the_length_classes(metric, k):
    """an external entry on lists of every length class of k_ca_trials: the list index and its slot in the class differ in every class"""
    rng = np.random.default_rng(62)
    tr = E.data(rng, E.LENGTH_CLASSES, 4, levels=6, prefix="L")
    m = E.ideal_map([tr], 10, rng, missing=0.2) if metric == "NDCG" else E.count_map([tr], rng)
    n = np.diff(tr[2])
    for lo, hi in ((0, 16), (16, 384), (384, 5000), (5000, 1 << 30)):
        cls = [q for q in range(len(n)) if lo < n[q] <= hi]
        assert any(tr[3][q] in m and q != cls.index(q) for q in cls), (lo, hi)
    arrays, ext = E.judgments(metric, m, tr, None, "train")
    p = dict(nRestart=1, nMaxIteration=5, seed=4)
    r = CR.learn(tr, None, metric, k, **p, **ext)
    assert r["trace"][0][7] != CR.VectorScorer(metric, k).score(CR.VectorScorer(metric, k).dot(tr[0], [0.25] * 4), tr[1], tr[2], tr[3])
    _same(_gpu(tr, None, metric, k, ext=arrays, **p), r)


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("DCG", 5), ("ERR", 10)])
def test_wrapped_labels(metric, k):
    """labels of 31, 32 and 33: gains 2147483647, 0 and 1 (metric/DCGScorer.java:28-31,137-139; ERRScorer.java:71-73)"""
    rng = np.random.default_rng(63)
    tr, va = E.shared_sets(rng, labels=E.WRAPPED)
    assert {31.0, 32.0, 33.0} <= set(tr[1].tolist())
    r = CR.learn(tr, va, metric, k, **_P_EXT)
    assert np.isfinite(r["train"]) and sum(1 for t in r["trace"] if t[0] == CR.TRIAL) > 100
    _same(_gpu(tr, va, metric, k, **_P_EXT), r)


@pytest.mark.parametrize("metric,k", [("MAP", 0), ("P", 3), ("RR", 10), ("NDCG", 10)])
def test_fractional_labels(metric, k):
    """labels of 0.5, 1.5 and 2.99: relevant (label > 0) for MAP / P / RR, (int) label for NDCG"""
    rng = np.random.default_rng(64)
    tr, va = E.shared_sets(rng, labels=E.FRACTIONAL)
    assert {0.5, 1.5} <= set(tr[1].tolist())
    r = CR.learn(tr, va, metric, k, **_P_EXT)
    _same(_gpu(tr, va, metric, k, **_P_EXT), r)


def test_external_judgment_refusals_and_lifetime():
    rng = np.random.default_rng(65)
    tr, va = E.shared_sets(rng, 4, n_train=12, n_valid=5, hi=10)
    counts = E.per_list(E.count_map([tr, va], rng, missing=0.0), tr[3], "count")
    p = dict(nRestart=1, nMaxIteration=4, seed=1)

    def new():
        return N.CoorAscentTrainer(metric="MAP", metric_k=0, **{_ARG[a]: v for a, v in p.items()})

    t = new()
    with pytest.raises(N.RankLibError) as e:                 # RL_ERR_STATE: no set to attach them to
        t.set_external_judgments(False, None, counts)
    assert "status -3" in str(e.value)
    E.feed(t, tr)
    with pytest.raises(N.RankLibError) as e:                 # ... and no validation set either
        t.set_external_judgments(True, None, counts[:len(va[3])])
    assert "status -3" in str(e.value)
    bad = counts.copy()
    bad[3] = -1
    with pytest.raises(N.RankLibError) as e:                 # RL_ERR_INVALID
        t.set_external_judgments(False, None, bad)
    assert "status -1" in str(e.value) and "negative" in str(e.value)
    t.set_external_judgments(False, None, counts)
    t.learn()
    with_counts = dict(weight=list(t.weights()), train=t.scores()[0], valid=None, trace=[tuple(x.item()) for x in t.trace()])
    with pytest.raises(N.RankLibError) as e:                 # the sets are on the device: RL_ERR_STATE after learn()
        t.set_external_judgments(False, None, counts)
    assert "status -3" in str(e.value) and "after rl_ca_learn" in str(e.value)
    plain = CR.learn(tr, None, "MAP", 0, **p)
    judged = CR.learn(tr, None, "MAP", 0, rel_doc_count=dict(zip(tr[3], counts.tolist())), **p)
    assert judged["trace"] != plain["trace"]
    _same(with_counts, judged)
    t = new()                                                # a later set_train discards the judgments given before it
    E.feed(t, tr, rdc_tr=counts)
    E.feed(t, tr)
    t.learn()
    ts, _ = t.scores()
    _same(dict(weight=list(t.weights()), train=ts, valid=None, trace=[tuple(x.item()) for x in t.trace()]), plain)


@pytest.mark.parametrize("m2t", ["NDCG@10", "MAP"])
def test_cli_qrel_reaches_the_trainer(tmp_path, m2t):
    """-qrel <file> with -ranker 4: the saved model is the restatement's, fed the maps the host scorer loaded from the same file, and
    differs from the model trained without the judgments"""
    rng = np.random.default_rng(66)
    X, lab, qoff = _data(rng, rng.integers(2, 25, 30), 4, labels=4)
    data, qrel, m_q, m_raw = (str(tmp_path / n) for n in ("d.txt", "qrel.txt", "q.txt", "raw.txt"))
    E.write_letor(data, X, lab, qoff)
    E.write_qrel(qrel, rng, np.diff(qoff))
    sc = MetricScorerFactory().createScorer(m2t)
    sc.loadExternalRelevanceJudgment(qrel)
    ext = dict(ideal=dict(sc.idealGains)) if m2t != "MAP" else dict(rel_doc_count=dict(sc.relDocCount))
    metric, k = ("MAP", 0) if m2t == "MAP" else ("NDCG", 10)
    train = (X, lab, qoff, [str(q) for q in range(len(qoff) - 1)])
    p = dict(nRestart=1, nMaxIteration=8, seed=5)
    r, plain = CR.learn(train, None, metric, k, **p, **ext), CR.learn(train, None, metric, k, **p)
    assert r["weight"] != plain["weight"]
    args = ["-train", data, "-ranker", "4", "-metric2t", m2t, "-r", "1", "-i", "8", "-seed", "5"]
    evaluator.main(args + ["-qrel", qrel, "-save", m_q])
    evaluator.main(args + ["-save", m_raw])
    assert evaluator.Evaluator.qrelFile == ""
    head = ("## Coordinate Ascent\n## Restart = 1\n## MaxIteration = 8\n## StepBase = 0.05\n## StepScale = 2.0\n"
            "## Tolerance = 0.001\n## Regularized = false\n## Slack = 0.001\n")
    body = lambda w: " ".join("%d:%s" % (f + 1, java_double_str(v)) for f, v in enumerate(w))      # noqa: E731
    assert open(m_q).read() == head + body(r["weight"])
    assert open(m_raw).read() == head + body(plain["weight"])
