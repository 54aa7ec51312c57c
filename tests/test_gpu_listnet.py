"""ListNet training (-ranker 7) on the MI355X against the literal restatement (tests/listnet_restatement.py): the weights after every
run as uint64, the per-epoch trace and both final metric values as doubles, no tolerance anywhere.

Shapes: k_ln_epoch is one block of B = 256 threads that keeps up to 2048 per-document values and up to 4096 weights in LDS; the sets mix
list lengths 1, 2, 63, 64, 65, B - 1, B, B + 1 and 2 B + 37, one list exactly at and one above the document cap, F = 1, 2, 63, 64, 136,
F + 1 > B and F + 1 above the weight cap."""
import os

import numpy as np
import pytest

import linear_ext as E
import listnet_restatement as LN
from ca_restatement import LiteralScorer
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, ListNet, Neuron, RankerFactory, RankerType, flatten, java_round
from ranklib_amd.metric import ERRScorer, MetricScorerFactory

pytestmark = pytest.mark.gpu

B, DOC_CAP, W_CAP = 256, 2048, 4096
LENGTHS = [1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 37]


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = (ListNet.seed, ListNet.nIteration, ListNet.learningRate, Neuron.learningRate, ERRScorer.MAX, DataPoint.missingZero,
             evaluator.Evaluator.normalize, evaluator.Evaluator.qrelFile)
    yield
    (ListNet.seed, ListNet.nIteration, ListNet.learningRate, Neuron.learningRate, ERRScorer.MAX, DataPoint.missingZero,
     evaluator.Evaluator.normalize, evaluator.Evaluator.qrelFile) = saved


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def _u64(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64).tolist()


def _data(rng, lengths, F, labels=(0, 1, 2, 3, 4), prefix="q", scale=1.0):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(qoff[-1])
    X = (rng.standard_normal((n, F)) * scale).astype(np.float32)
    X[rng.random(X.shape) < 0.15] = 0.0
    lab = rng.choice(np.array(labels, np.float32), n).astype(np.float32)
    return X, lab, qoff, ["%s%d" % (prefix, i) for i in range(len(lengths))]


def _mixed(rng, F, **kw):
    """about 40 lists: every length of LENGTHS once, in a shuffled order among short lists"""
    lengths = list(LENGTHS) + [int(v) for v in rng.integers(1, 20, 31)]
    rng.shuffle(lengths)
    return _data(rng, lengths, F, **kw)


def _gpu(train, valid, start, epochs, lr, metric="NDCG", k=10, ext=None):
    t = E.feed(N.ListNetTrainer(n_epochs=epochs, learning_rate=lr, metric=metric, metric_k=k), train, valid, **(ext or {}))
    t.set_weights(start)
    return t


def _same_run(t, r, valid):
    assert _u64(t.weights()) == _u64(r["weight"])
    tr = t.trace()
    assert [int(e) for e in tr["epoch"]] == [e for e, _, _, _ in r["trace"]]
    assert [int(s) for s in tr["saved"]] == [s for _, s, _, _ in r["trace"]]
    assert _bits(tr["train"]) == _bits([a for _, _, a, _ in r["trace"]])
    assert _bits(tr["valid"]) == _bits([v for _, _, _, v in r["trace"]])
    ts, vs = t.scores()
    assert _bits(ts) == _bits(r["train"])
    if valid:
        assert _bits(vs) == _bits(r["valid"])
    assert _bits(t.doc_scores()) == _bits(r["train_scores"])


def _run(train, valid=None, seed=3, epochs=2, lr=0.5, metric="NDCG", k=10, start=None, vector=True):
    start = LN.draw_weights(seed, train[0].shape[1] + 1) if start is None else list(start)
    r = LN.learn(train, valid, metric, k, n_iteration=epochs, lr=lr, start=start, vector=vector)
    t = _gpu(train, valid, start, epochs, lr, metric, k)
    t.learn()
    _same_run(t, r, valid is not None)
    return t, r, start


# (F, epochs, learning rate, validation set, metric)
_SHAPES = [(1, 3, 0.5, False, "NDCG"), (2, 2, 0.00001, True, "MAP"), (63, 2, 0.5, True, "NDCG"), (64, 1, 0.00001, False, "ERR"),
           (136, 2, 0.5, False, "NDCG"), (B + 44, 1, 0.5, True, "DCG")]


@pytest.mark.parametrize("F,epochs,lr,valid,metric", _SHAPES, ids=["F%d" % c[0] for c in _SHAPES])
def test_list_lengths_and_feature_counts(F, epochs, lr, valid, metric):
    rng = np.random.default_rng(50 + F)
    tr = _mixed(rng, F)
    va = _data(rng, rng.integers(1, 30, 12), F, prefix="v") if valid else None
    _, r, start = _run(tr, va, epochs=epochs, lr=lr, metric=metric, k=0 if metric == "MAP" else 10)
    assert _u64(r["weight"]) != _u64(start) or valid


def test_the_vector_form_of_the_restatement_is_the_literal_one_here():
    rng = np.random.default_rng(2)
    tr = _data(rng, [1, 2, 63, 64, 65, 5, 9], 3)
    start = LN.draw_weights(9, 4)
    a = LN.learn(tr, None, n_iteration=2, lr=0.5, start=start, vector=False)
    b = LN.learn(tr, None, n_iteration=2, lr=0.5, start=start, vector=True)
    assert _u64(a["weight"]) == _u64(b["weight"])
    _run(tr, None, epochs=2, lr=0.5, start=start, vector=False)


def test_lists_at_and_above_the_lds_document_cap():
    rng = np.random.default_rng(11)
    _run(_data(rng, [DOC_CAP, 7, DOC_CAP + 1, 1, DOC_CAP - 1], 3), None, epochs=1, lr=0.5)


def test_more_weights_than_the_lds_holds():
    rng = np.random.default_rng(12)
    _run(_data(rng, [3, 70, 1, B + 9], W_CAP + 5), None, epochs=1, lr=0.5)
    _run(_data(rng, [3, 70, 1, B + 9], W_CAP - 1), None, epochs=1, lr=0.5)       # F + 1 == the cap: the last set that stays in LDS


def test_a_single_list():
    rng = np.random.default_rng(13)
    _run(_data(rng, [37], 5), None, epochs=3, lr=0.5)
    t, r, start = _run(_data(rng, [1], 5), None, epochs=2, lr=0.5)
    assert _u64(r["weight"]) == _u64(start)                   # one document: d1 = d2 = 1


@pytest.mark.parametrize("labels", [(0, 1, 2, 3, 4), (2,), (0, 0.5, 1, 1.5, 2.99), (0, 30)], ids=["0-4", "equal", "fractional", "30"])
def test_labels(labels):
    rng = np.random.default_rng(14)
    tr = _data(rng, rng.integers(1, 40, 25), 4, labels=labels)
    va = _data(rng, rng.integers(2, 40, 8), 4, labels=labels, prefix="v")
    _run(tr, va, epochs=2, lr=0.5, metric="MAP", k=0)


@pytest.mark.parametrize("wsum", [40.0, -40.0, 800.0, -800.0])
def test_saturated_outputs(wsum):
    rng = np.random.default_rng(15)
    X, lab, qoff, qid = _data(rng, [5, 9, 70, 3], 3)
    X[:, 0] = 1.0
    start = [wsum, 0.0, 0.0, 0.0]
    out = LN.scores(X, start)
    if abs(wsum) == 800.0:
        assert set(out.tolist()) == {1.0 if wsum > 0 else 0.0}    # exactly saturated: exp(-800) is 0.0, 1 / (1 + Infinity) is 0.0
    _run((X, lab, qoff, qid), None, epochs=2, lr=0.00001, start=start)
    _run((X, lab, qoff, qid), None, epochs=2, lr=0.5, start=start)


def test_the_order_of_the_lists_matters():
    rng = np.random.default_rng(16)
    X, lab, qoff, qid = _data(rng, [6, 9, 4, 7, 12], 4)
    order = [0, 3, 2, 1, 4]                                   # lists 1 and 3 swapped
    rows = np.concatenate([np.arange(qoff[q], qoff[q + 1]) for q in order])
    swapped = (X[rows], lab[rows], np.concatenate([[0], np.cumsum([qoff[q + 1] - qoff[q] for q in order])]).astype(np.int32),
               [qid[q] for q in order])
    t1, r1, _ = _run((X, lab, qoff, qid), None, epochs=1, lr=0.5)
    t2, r2, _ = _run(swapped, None, epochs=1, lr=0.5)
    assert _u64(t1.weights()) != _u64(t2.weights()) and _u64(r1["weight"]) != _u64(r2["weight"])


def test_validation_picks_the_restatements_epoch_and_a_tie_does_not_replace_it():
    rng = np.random.default_rng(17)
    tr = _data(rng, rng.integers(2, 30, 30), 5)
    va = _data(rng, rng.integers(2, 30, 10), 5, prefix="v")
    t, r, start = _run(tr, va, epochs=3, lr=0.5)
    saved = [e for e, s, _, _ in r["trace"] if s]
    assert saved and _bits(r["valid"]) == _bits(r["trace"][saved[-1] - 1][3])      # the final score is the saved epoch's
    # a learning rate of 0.0: every epoch scores the same, only the first is saved
    t0, r0, start0 = _run(tr, va, epochs=3, lr=0.0)
    assert [int(s) for s in t0.trace()["saved"]] == [1, 0, 0] and _u64(t0.weights()) == _u64(start0)
    # no relevant document on the validation side: the Java's restore throws; -epoch 0 ends the same way
    dead = (va[0], np.zeros_like(va[1]), va[2], va[3])
    for sets, epochs in ((dead, 2), (va, 0)):
        with pytest.raises(LN.RestoreError):
            LN.learn(tr, sets, n_iteration=epochs, lr=0.5, start=start, vector=True)
        t = _gpu(tr, sets, start, epochs, 0.5)
        with pytest.raises(N.NoBestModelError) as e:
            t.learn()
        assert "status -7" in str(e.value)


def test_weights_that_overflow_are_refused_with_the_epoch():
    rng = np.random.default_rng(18)
    tr = _data(rng, rng.integers(2, 12, 6), 3, scale=100.0)
    start = LN.draw_weights(3, 4)
    with pytest.raises(OverflowError) as want:                # the restatement overflows first, on the CPU
        LN.learn(tr, None, n_iteration=3, lr=1.7e308, start=start, vector=True)
    t = _gpu(tr, None, start, 3, 1.7e308)
    with pytest.raises(N.RankLibError) as e:
        t.learn()
    assert "status -4" in str(e.value) and "after %s " % want.value in str(e.value)


@pytest.mark.parametrize("epochs", [0, 1])
def test_the_scoring_kernel_gives_the_forward_kernels_bits(epochs):
    rng = np.random.default_rng(19)
    F = 7
    tr = _data(rng, [300, 1, 400, 299], F)                    # 1000 documents: not a multiple of 256
    va = _data(rng, [130, 131], F, prefix="v")
    start = LN.draw_weights(5, F + 1)
    t = _gpu(tr, va if epochs else None, start, epochs, 0.5)
    t.learn()
    w = t.weights()
    net = N.NetModel(list(range(1, F + 1)), [], w)
    for validation, s in ((False, tr), (True, va)):
        if validation and not epochs:
            continue
        rows = np.zeros((s[0].shape[0], F + 1), np.float32)
        rows[:, 1:] = s[0]
        assert _bits(t.doc_scores(validation)) == _bits(net.predict_rows(rows))


def test_refusals_on_a_handle():
    rng = np.random.default_rng(20)
    tr = _data(rng, [4, 5], 3)
    t = E.feed(N.ListNetTrainer(n_epochs=1), tr)
    with pytest.raises(N.RankLibError) as e:                  # learn without weights
        t.learn()
    assert "status -1" in str(e.value)
    for n in (3, 5):
        with pytest.raises(N.RankLibError) as e:
            t.set_weights(np.zeros(n))
        assert "status -1" in str(e.value)
    t.set_weights(np.zeros(4))
    t.learn()
    with pytest.raises(N.RankLibError):                       # once per handle
        t.learn()
    t2 = N.ListNetTrainer(n_epochs=1)
    with pytest.raises(N.RankLibError) as e:                  # learn without a training set
        t2.learn()
    assert "status -1" in str(e.value)


# ---- the Python class and the command line --------------------------------------------------------------------------------------------
def _read(path, F):
    lists = FeatureManager.readInput(path)
    X, lab, qoff, _ = flatten(lists, list(range(1, F + 1)))
    return lists, (X, lab, qoff, [rl.getID() for rl in lists])


def _files(tmp_path, seed=21, F=4):
    rng = np.random.default_rng(seed)
    tr = _data(rng, rng.integers(2, 25, 24), F)
    va = _data(rng, rng.integers(2, 25, 8), F)
    te = _data(rng, rng.integers(2, 25, 6), F)
    paths = [str(tmp_path / n) for n in ("train.txt", "valid.txt", "test.txt")]
    for p, s, q0 in zip(paths, (tr, va, te), (0, 100, 200)):
        E.write_letor(p, s[0], s[1], s[2], q0)
    return paths


def test_command_line_train_save_load_test(tmp_path):
    F = 4
    train, valid, test = _files(tmp_path)
    m1, m2 = str(tmp_path / "m1.txt"), str(tmp_path / "m2.txt")
    args = ["-train", train, "-ranker", "7", "-netseed", "3", "-epoch", "3", "-metric2t", "NDCG@10", "-validate", valid]
    evaluator.main(args + ["-save", m1])
    assert (ListNet.seed, ListNet.nIteration) == (None, 1500)
    _, tr = _read(train, F)
    _, va = _read(valid, F)
    lists_te, te = _read(test, F)
    r = LN.learn(tr, va, "NDCG", 10, n_iteration=3, lr=0.00001, seed=3)
    text = open(m1).read()
    assert text == LN.model_text(r["weight"], list(range(1, F + 1)), 3) and "## Epochs = 3\n" in text
    evaluator.main(args + ["-save", m2])                      # the same run again: the same bytes
    assert open(m2).read() == text
    e = evaluator.Evaluator(RankerType.LAMBDAMART, "NDCG@10", "NDCG@10")
    got = e.test(m1, test)
    loaded = RankerFactory().loadRankerFromFile(m1)
    assert _u64(loaded.weights[0].ravel()) == _u64(r["weight"])
    want = LiteralScorer("NDCG", 10).score([float(v) for v in LN.scores(te[0], r["weight"])], te[1], te[2], te[3])
    assert _bits(got) == _bits(want)
    evaluator.main(["-load", m1, "-test", test])
    # -lr x: the Java's quirk gives 0.001 whatever x is
    evaluator.main(["-train", train, "-ranker", "7", "-netseed", "3", "-epoch", "2", "-lr", "0.5", "-metric2t", "NDCG@10", "-save", m2])
    r2 = LN.learn(tr, None, "NDCG", 10, n_iteration=2, lr=0.001, seed=3)
    assert open(m2).read() == LN.model_text(r2["weight"], list(range(1, F + 1)), 2)
    assert (ListNet.learningRate, Neuron.learningRate) == (0.00001, 0.001)
    # the Python class: rounded training score, the validation score as it is
    ListNet.seed, ListNet.nIteration = 3, 3
    ranker = evaluator.Evaluator(RankerType.LISTNET, "NDCG@10", "NDCG@10").evaluate(train, valid)
    assert type(ranker) is ListNet and ranker.hidden == [] and _u64(ranker.weights[0].ravel()) == _u64(r["weight"])
    assert ranker.getScoreOnTrainingData() == java_round(r["train"], 4) and _bits(ranker.getScoreOnValidationData()) == _bits(r["valid"])
    assert _bits(np.concatenate([ranker.evalList(rl) for rl in lists_te])) == _bits(LN.scores(te[0], r["weight"]))


def test_command_line_restore_error_kcv_and_norm(tmp_path):
    train, valid, test = _files(tmp_path, seed=22)
    dead = str(tmp_path / "dead.txt")
    with open(dead, "w") as f:
        f.write("0 qid:900 1:1 2:0 3:1 4:0\n0 qid:900 1:0 2:1 3:0 4:1\n")
    with pytest.raises(N.RankLibError) as e:
        evaluator.main(["-train", train, "-ranker", "7", "-netseed", "3", "-epoch", "1", "-metric2t", "NDCG@10", "-validate", dead])
    assert str(e.value).startswith("Error in NeuralNetwork.restoreBestModelOnValidation(): ")
    assert ListNet.seed is None
    evaluator.main(["-train", train, "-ranker", "7", "-netseed", "3", "-epoch", "2", "-kcv", "2", "-metric2t", "MAP"])
    evaluator.main(["-train", train, "-ranker", "7", "-netseed", "3", "-epoch", "2", "-tvs", "0.8", "-norm", "zscore", "-metric2t", "NDCG@10",
                    "-test", test])


def test_qrel_judgments_reach_the_metric(tmp_path):
    F = 4
    train, _, _ = _files(tmp_path, seed=23)
    qrel = str(tmp_path / "qrel.txt")
    _, tr = _read(train, F)
    E.write_qrel(qrel, np.random.default_rng(24), np.diff(tr[2]))
    sc = MetricScorerFactory().createScorer("NDCG@10")
    sc.loadExternalRelevanceJudgment(qrel)
    judged = LN.learn(tr, None, "NDCG", 10, n_iteration=2, lr=0.00001, seed=3, ideal=dict(sc.idealGains))
    plain = LN.learn(tr, None, "NDCG", 10, n_iteration=2, lr=0.00001, seed=3)
    assert java_round(judged["train"], 4) != java_round(plain["train"], 4) and _u64(judged["weight"]) == _u64(plain["weight"])
    ListNet.seed, ListNet.nIteration = 3, 2
    evaluator.Evaluator.qrelFile = qrel
    a = evaluator.Evaluator(RankerType.LISTNET, "NDCG@10", "NDCG@10").evaluate(train)
    evaluator.Evaluator.qrelFile = ""
    b = evaluator.Evaluator(RankerType.LISTNET, "NDCG@10", "NDCG@10").evaluate(train)
    assert a.getScoreOnTrainingData() == java_round(judged["train"], 4) and b.getScoreOnTrainingData() == java_round(plain["train"], 4)
