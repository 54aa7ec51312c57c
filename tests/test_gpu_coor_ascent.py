"""Coordinate Ascent (-ranker 4) on the MI355X: every trial's score, the weights, the scores and the model text bit-identical to the
numpy restatement of CoorAscent.learn (tests/ca_restatement.py), and the reference's own testCoorAscent / testRanker flows."""
import numpy as np
import pytest

import ca_restatement as CR
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd.learning import CoorAscent, java_double_str
from ranklib_amd.metric import ERRScorer
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


def _gpu(train, valid=None, metric="NDCG", k=10, err_max=16.0, **p):
    t = N.CoorAscentTrainer(metric=metric, metric_k=k, err_max=err_max, **{_ARG[a]: v for a, v in p.items()})
    X, lab, qoff, qid = train
    keys = {}
    qkey = np.array([keys.setdefault(q, len(keys)) for q in qid], np.int32)
    t.set_train(X, lab, qoff, qkey=qkey)
    if valid is not None:
        Xv, lv, qv, qidv = valid
        t.set_validation(Xv, lv, qv, qkey=np.array([keys.setdefault(q, len(keys)) for q in qidv], np.int32))
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
