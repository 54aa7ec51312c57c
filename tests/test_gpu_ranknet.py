"""RankNet training (-ranker 1) on the MI355X against the restatement (tests/ranknet_restatement.py): the weights after every run as
uint64, the per-epoch trace (saved, mis-ordered pairs, total pairs, both scores) and both final metric values as doubles, the scores of
every document, no tolerance anywhere.

Shapes: k_rn_epoch is one block of B = 1024 threads.  It keeps up to 2048 weights, a list's kept values (3 n H + n + H doubles, H = the
neurons past the input) up to 9216 doubles and its X tile (F (n | 1) floats) up to 8192 floats in LDS, and reads global memory beyond
each cap.  The sets mix list lengths 1, 2, 63, 64, 65, B - 1, B, B + 1, pair counts of a step of 0, 64, 65, B and B + 1, lists at and
one past every cap, and the networks -layer 0, [1], [10] and [3, 2].

The learning rates are larger than RankNet's default 0.00005 and chosen per shape on the restatement, so that one epoch moves the largest
weight by roughly 0.01 to 0.3 (a step's update grows with its pair count: 0.001 for the lists of a thousand documents, 0.05 for short
lists) and the outputs stay away from saturation; every run checks there that the weights moved and stayed finite (learn() raises
OverflowError else)."""
import numpy as np
import pytest

import linear_ext as E
import ranknet_restatement as RN
from ca_restatement import LiteralScorer
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, ListNet, Neuron, RankerFactory, RankerType, RankNet, flatten, java_round
from ranklib_amd.metric import ERRScorer

pytestmark = pytest.mark.gpu

B, W_CAP, POOL, X_CAP = 1024, 2048, 9216, 8192
_STATICS = ("nIteration", "nHiddenLayer", "nHiddenNodePerLayer", "learningRate", "seed")


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = ([getattr(RankNet, k) for k in _STATICS], ListNet.seed, Neuron.learningRate, ERRScorer.MAX, DataPoint.missingZero,
             evaluator.Evaluator.normalize, evaluator.Evaluator.qrelFile)
    yield
    for k, v in zip(_STATICS, saved[0]):
        setattr(RankNet, k, v)
    (ListNet.seed, Neuron.learningRate, ERRScorer.MAX, DataPoint.missingZero, evaluator.Evaluator.normalize,
     evaluator.Evaluator.qrelFile) = saved[1:]


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def _u64(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64).tolist()


def _labels(rng, n, kind, labels):
    if kind == "equal":
        return np.full(n, 2.0, np.float32)
    if kind == "first":                                       # the first document outranks all others: its step has n - 1 pairs
        lab = np.zeros(n, np.float32)
        lab[0] = 1.0
        return lab
    return rng.choice(np.array(labels, np.float32), n).astype(np.float32)


def _data(rng, lengths, F, labels=(0, 1, 2), prefix="q", scale=1.0, kinds=None):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(qoff[-1])
    X = (rng.standard_normal((n, F)) * scale).astype(np.float32)
    X[rng.random(X.shape) < 0.15] = 0.0
    kinds = kinds or ["ties"] * len(lengths)
    lab = np.concatenate([_labels(rng, int(m), k, labels) for m, k in zip(lengths, kinds)])
    return X, lab, qoff, ["%s%d" % (prefix, i) for i in range(len(lengths))]


def _nw(F, hidden):
    n = [F] + list(hidden) + [1]
    return sum(n[l] * (n[l - 1] + 1) for l in range(1, len(n)))


def _gpu(train, valid, start, epochs, lr, hidden, metric="NDCG", k=10):
    t = E.feed(N.RankNetTrainer(n_epochs=epochs, learning_rate=lr, hidden_sizes=hidden, metric=metric, metric_k=k), train, valid)
    t.set_weights(start)
    return t


def _same_run(t, r, valid):
    assert _u64(t.weights()) == _u64(r["weight"])
    tr = t.trace()
    for name, col in (("epoch", 0), ("saved", 1), ("misordered", 2), ("total_pairs", 3)):
        assert [int(e) for e in tr[name]] == [rec[col] for rec in r["trace"]], name
    assert _bits(tr["train"]) == _bits([rec[4] for rec in r["trace"]])
    assert _bits(tr["valid"]) == _bits([rec[5] for rec in r["trace"]])
    ts, vs = t.scores()
    assert _bits(ts) == _bits(r["train"])
    if valid:
        assert _bits(vs) == _bits(r["valid"])
    assert _bits(t.doc_scores()) == _bits(r["train_scores"])


def _run(train, valid=None, hidden=(10,), seed=3, epochs=2, lr=0.05, metric="NDCG", k=10, start=None, moves=True):
    F = train[0].shape[1]
    start = RN.draw_weights(RN.build(F, hidden), seed).abi_weights() if start is None else np.array(start, np.float64)
    assert len(start) == _nw(F, hidden)
    r = RN.learn(train, valid, metric, k, n_iteration=epochs, lr=lr, hidden=hidden, start=start)
    if moves and valid is None:
        assert _u64(r["weight"]) != _u64(start) and np.all(np.isfinite(r["weight"]))
    t = _gpu(train, valid, start, epochs, lr, list(hidden), metric, k)
    t.learn()
    _same_run(t, r, valid is not None)
    return t, r, start


def test_list_lengths_and_pair_counts_around_the_wavefront_and_the_block():
    """every length once among short lists; a step's pair count is 0 (equal labels), 64, 65, B and B + 1 (the first document outranks
    the rest), and anything in between (ties)"""
    rng = np.random.default_rng(50)
    lengths = [1, 2, 63, 64, 65, 7, B - 1, 70, B, 65, 66, B + 1, 12, B + 1, B + 2, 3]
    kinds = ["ties"] * 9 + ["first", "first", "ties", "ties", "first", "first", "ties"]
    kinds[7] = "equal"
    _run(_data(rng, lengths, 3, kinds=kinds), None, hidden=[2], epochs=1, lr=0.001)


_NETS = [([], "NDCG", False), ([1], "MAP", True), ([10], "ERR", True), ([3, 2], "NDCG", True), ([10], "DCG", False)]


@pytest.mark.parametrize("hidden,metric,valid", _NETS, ids=["layer0", "h1", "h10-err", "h3-2", "h10-dcg"])
def test_networks_and_metrics(hidden, metric, valid):
    rng = np.random.default_rng(60 + len(hidden) + sum(hidden))
    tr = _data(rng, [int(v) for v in rng.integers(1, 40, 14)] + [65, 1, 130], 5, labels=(0, 1, 2, 3, 4))
    va = _data(rng, rng.integers(2, 30, 8), 5, prefix="v") if valid else None
    _run(tr, va, hidden=hidden, epochs=2, metric=metric, k=0 if metric == "MAP" else 10)


def test_more_weights_than_threads():
    rng = np.random.default_rng(70)
    F = 110                                                   # 111 * 10 + 11 = 1121 weights: the update takes two rounds
    assert B < _nw(F, [10]) <= W_CAP
    _run(_data(rng, [9, 30, 1, 17, 66], F), None, hidden=[10], epochs=1, lr=0.02)


def test_more_weights_than_the_lds_holds():
    rng = np.random.default_rng(71)
    assert _nw(205, [10]) > W_CAP >= _nw(202, [10])
    _run(_data(rng, [5, 40, 1, 13], 205), None, hidden=[10], epochs=1)       # 2071 weights: k_rn_epoch<false>, the weights in global memory
    _run(_data(rng, [5, 40, 1, 13], 202), None, hidden=[10], epochs=1)       # 2041: the largest of these networks that stays in LDS


def test_lists_at_and_above_the_lds_caps():
    rng = np.random.default_rng(72)
    need = lambda n, H: 3 * n * H + n + H                     # noqa: E731
    assert need(270, 11) <= POOL < need(271, 11)
    _run(_data(rng, [270, 5, 271, 1, 269], 3, labels=(0, 0, 0, 1)), None, hidden=[10], epochs=1, lr=0.01)      # the kept values of list 2 are global
    assert 30 * (273 | 1) <= X_CAP < 30 * (274 | 1) and need(274, 2) <= POOL
    _run(_data(rng, [273, 4, 274, 9], 30, labels=(0, 0, 0, 1)), None, hidden=[1], epochs=1, lr=0.01)           # the X tile of list 2 is not staged


def test_a_single_list_and_lists_without_pairs():
    rng = np.random.default_rng(73)
    _run(_data(rng, [37], 5), None, hidden=[4], epochs=3)
    for kinds, lengths in ((["equal"], [9]), (["ties"], [1])):
        t, r, start = _run(_data(rng, lengths, 5, kinds=kinds), None, hidden=[4], epochs=2, moves=False)
        assert _u64(r["weight"]) == _u64(start) and [rec[3] for rec in r["trace"]] == [0, 0]
    # the step without pairs is still taken: -0.0 + lr * (0.0 * x - 0.0) is +0.0 where x >= 0
    X, lab, qoff, qid = _data(rng, [6, 3], 3, kinds=["equal", "equal"])
    start = RN.draw_weights(RN.build(3, [2]), 5).abi_weights()
    start[0] = start[7] = -0.0
    t, r, _ = _run((np.abs(X), lab, qoff, qid), None, hidden=[2], epochs=1, start=start, moves=False)
    assert _bits(t.weights()[[0, 7]]) == _bits([0.0, 0.0])


@pytest.mark.parametrize("labels", [(0, 0.5, 1, 1.5, 2.99), (0, 30)], ids=["fractional", "30"])
def test_labels(labels):
    rng = np.random.default_rng(74)
    tr = _data(rng, rng.integers(1, 40, 20), 4, labels=labels)
    va = _data(rng, rng.integers(2, 40, 8), 4, labels=labels, prefix="v")
    _run(tr, va, hidden=[3], epochs=2, metric="MAP", k=0)


@pytest.mark.parametrize("wsum", [40.0, -800.0])
def test_saturated_outputs(wsum):
    rng = np.random.default_rng(75)
    X, lab, qoff, qid = _data(rng, [5, 9, 70, 3], 3)
    X[:, 0] = 1.0
    start = np.zeros(_nw(3, [2]))
    start[0] = start[4] = wsum                                # both hidden neurons saturate
    _run((X, lab, qoff, qid), None, hidden=[2], epochs=2, start=start, moves=False)
    _run((X, lab, qoff, qid), None, hidden=[], epochs=2, start=[wsum, 0.0, 0.0, 0.0], moves=False)


def test_the_order_of_the_documents_in_a_list_matters():
    rng = np.random.default_rng(76)
    X, lab, qoff, qid = _data(rng, [9, 12], 4)
    rows = np.arange(21)
    rows[[2, 5]] = rows[[5, 2]]
    t1, r1, _ = _run((X, lab, qoff, qid), None, hidden=[3], epochs=1)
    t2, r2, _ = _run((X[rows], lab[rows], qoff, qid), None, hidden=[3], epochs=1)
    assert _u64(t1.weights()) != _u64(t2.weights())


def test_validation_saves_in_some_epochs_and_the_restore_throws_when_none_did():
    rng = np.random.default_rng(77)
    tr = _data(rng, rng.integers(2, 30, 30), 5)
    va = _data(rng, rng.integers(2, 30, 10), 5, prefix="v")
    t, r, start = _run(tr, va, hidden=[4], epochs=3, lr=2.0)
    saved = [rec[0] for rec in r["trace"] if rec[1]]
    assert saved and _bits(r["valid"]) == _bits(r["trace"][saved[-1] - 1][5])      # the final score is the saved epoch's
    # a learning rate of 0.0: every epoch scores the same, only the first is saved
    t0, r0, start0 = _run(tr, va, hidden=[4], epochs=3, lr=0.0)
    assert [int(s) for s in t0.trace()["saved"]] == [1, 0, 0] and _u64(t0.weights()) == _u64(start0)
    # no relevant document on the validation side: the Java's restore throws; -epoch 0 ends the same way
    dead = (va[0], np.zeros_like(va[1]), va[2], va[3])
    for sets, epochs in ((dead, 2), (va, 0)):
        with pytest.raises(RN.RestoreError):
            RN.learn(tr, sets, n_iteration=epochs, lr=0.05, hidden=[4], start=start)
        t = _gpu(tr, sets, start, epochs, 0.05, [4])
        with pytest.raises(N.NoBestModelError) as e:
            t.learn()
        assert "status -7" in str(e.value)


def test_some_epochs_save_and_others_do_not():
    """found on the restatement: a seed and a rate at which the validation score rises in a later epoch and falls in another"""
    rng = np.random.default_rng(78)
    tr = _data(rng, rng.integers(2, 20, 12), 4)
    va = _data(rng, rng.integers(2, 20, 6), 4, prefix="v")
    for seed in range(12):
        start = RN.draw_weights(RN.build(4, [3]), seed).abi_weights()
        r = RN.learn(tr, va, "NDCG", 10, n_iteration=3, lr=2.0, hidden=[3], start=start)
        flags = [rec[1] for rec in r["trace"]]
        if flags[0] == 1 and 0 in flags and sum(flags) >= 2:
            break
    else:
        pytest.fail("no seed below 12 gives a run that saves in some later epoch and not in another")
    _run(tr, va, hidden=[3], epochs=3, lr=2.0, start=start)


def test_weights_that_overflow_are_refused_with_the_epoch():
    rng = np.random.default_rng(79)
    tr = _data(rng, rng.integers(2, 12, 6), 3, scale=100.0)
    start = RN.draw_weights(RN.build(3, [2]), 3).abi_weights()
    with pytest.raises(OverflowError) as want:                # the restatement overflows first, on the CPU
        RN.learn(tr, None, n_iteration=3, lr=1.7e308, hidden=[2], start=start)
    t = _gpu(tr, None, start, 3, 1.7e308, [2])
    with pytest.raises(N.RankLibError) as e:
        t.learn()
    assert "status -4" in str(e.value) and "after %s " % want.value in str(e.value)


@pytest.mark.parametrize("hidden", [[], [10], [3, 2]], ids=["layer0", "h10", "h3-2"])
def test_the_scoring_kernel_gives_the_forward_kernels_bits(hidden):
    rng = np.random.default_rng(80)
    F = 7
    tr = _data(rng, [300, 1, 400, 299], F, labels=(0, 0, 0, 0, 1))      # 1000 documents: not a multiple of 256
    va = _data(rng, [130, 131], F, prefix="v")
    start = RN.draw_weights(RN.build(F, hidden), 5).abi_weights()
    t = _gpu(tr, va, start, 1, 0.01, hidden)
    t.learn()
    net = N.NetModel(list(range(1, F + 1)), hidden, t.weights())
    for validation, s in ((False, tr), (True, va)):
        rows = np.zeros((s[0].shape[0], F + 1), np.float32)
        rows[:, 1:] = s[0]
        assert _bits(t.doc_scores(validation)) == _bits(net.predict_rows(rows))


def test_refusals_on_a_handle():
    rng = np.random.default_rng(81)
    tr = _data(rng, [4, 5], 3)
    t = E.feed(N.RankNetTrainer(n_epochs=1, hidden_sizes=[2]), tr)
    with pytest.raises(N.RankLibError) as e:                  # learn without weights
        t.learn()
    assert "status -1" in str(e.value)
    for n in (10, 12, 4):                                     # the network has 4 * 2 + 3 = 11
        with pytest.raises(N.RankLibError) as e:
            t.set_weights(np.zeros(n))
        assert "status -1" in str(e.value)
    t.set_weights(np.zeros(11))
    t.learn()
    with pytest.raises(N.RankLibError):                       # once per handle
        t.learn()
    t2 = N.RankNetTrainer(n_epochs=1)
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
    paths = [str(tmp_path / n) for n in ("train.txt", "valid.txt", "test.txt")]
    for p, m, q0 in zip(paths, (20, 8, 6), (0, 100, 200)):
        s = _data(rng, rng.integers(2, 25, m), F)
        E.write_letor(p, s[0], s[1], s[2], q0)
    return paths


def test_command_line_train_save_load_test(tmp_path):
    F = 4
    train, valid, test = _files(tmp_path)
    m1, m2 = str(tmp_path / "m1.txt"), str(tmp_path / "m2.txt")
    args = ["-train", train, "-ranker", "1", "-rnseed", "3", "-layer", "1", "-node", "4", "-epoch", "2", "-metric2t", "NDCG@10"]
    evaluator.main(args + ["-save", m1])
    assert tuple(getattr(RankNet, s) for s in _STATICS) == (100, 1, 10, 0.00005, None) and Neuron.learningRate == 0.001
    _, tr = _read(train, F)
    _, va = _read(valid, F)
    lists_te, te = _read(test, F)
    r = RN.learn(tr, None, "NDCG", 10, n_iteration=2, lr=0.00005, hidden=[4], seed=3)
    text = open(m1).read()
    assert text == RN.model_text(r["weight"], list(range(1, F + 1)), [4], 2) and "## Epochs = 2\n" in text
    loaded = RankerFactory().loadRankerFromFile(m1)           # the saved file loads again with the same bits
    assert type(loaded) is RankNet and loaded.hidden == [4]
    assert _u64(np.concatenate([m.ravel() for m in loaded.weights])) == _u64(r["weight"])
    e = evaluator.Evaluator(RankerType.LAMBDAMART, "NDCG@10", "NDCG@10")
    want = LiteralScorer("NDCG", 10).score([float(v) for v in RN.scores(r["matrices"], te[0])], te[1], te[2], te[3])
    assert _bits(e.test(m1, test)) == _bits(want)
    # -lr x is x, a validation set, two hidden layers, another metric
    evaluator.main(["-train", train, "-ranker", "1", "-rnseed", "7", "-layer", "2", "-node", "3", "-epoch", "3", "-lr", "0.5", "-metric2t", "MAP",
                    "-validate", valid, "-save", m2])
    r2 = RN.learn(tr, va, "MAP", 0, n_iteration=3, lr=0.5, hidden=[3, 3], seed=7)
    assert open(m2).read() == RN.model_text(r2["weight"], list(range(1, F + 1)), [3, 3], 3)
    assert RankNet.learningRate == 0.00005 and RankNet.seed is None
    # the Python class: rounded training score, the validation score as it is, evalList
    RankNet.seed, RankNet.nIteration, RankNet.nHiddenNodePerLayer, RankNet.learningRate = 7, 3, 3, 0.5
    RankNet.nHiddenLayer = 2
    ranker = evaluator.Evaluator(RankerType.RANKNET, "MAP", "MAP").evaluate(train, valid)
    assert type(ranker) is RankNet and ranker.hidden == [3, 3]
    assert _u64(np.concatenate([m.ravel() for m in ranker.weights])) == _u64(r2["weight"])
    assert ranker.getScoreOnTrainingData() == java_round(r2["train"], 4) and _bits(ranker.getScoreOnValidationData()) == _bits(r2["valid"])
    assert _bits(np.concatenate([ranker.evalList(rl) for rl in lists_te])) == _bits(RN.scores(r2["matrices"], te[0]))
    assert ranker.model() == open(m2).read()


def test_command_line_restore_error_and_kcv(tmp_path):
    train, valid, test = _files(tmp_path, seed=22)
    dead = str(tmp_path / "dead.txt")
    with open(dead, "w") as f:
        f.write("0 qid:900 1:1 2:0 3:1 4:0\n0 qid:900 1:0 2:1 3:0 4:1\n")
    with pytest.raises(N.RankLibError) as e:
        evaluator.main(["-train", train, "-ranker", "1", "-rnseed", "3", "-epoch", "1", "-node", "2", "-metric2t", "NDCG@10", "-validate", dead])
    assert str(e.value).startswith("Error in NeuralNetwork.restoreBestModelOnValidation(): ")
    assert RankNet.seed is None
    evaluator.main(["-train", train, "-ranker", "1", "-rnseed", "3", "-epoch", "1", "-layer", "0", "-kcv", "2", "-metric2t", "MAP"])
    for refused in (["-ranker", "5", "-rnseed", "3"], ["-ranker", "1"]):
        with pytest.raises(N.RankLibError) as e:
            evaluator.main(["-train", train] + refused)
        assert "out of scope" in str(e.value)
