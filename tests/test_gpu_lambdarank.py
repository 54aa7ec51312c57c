"""LambdaRank training (-ranker 5) on the MI355X against the restatement (tests/lambdarank_restatement.py): the weights after every run
as uint64, the per-epoch trace (saved, mis-ordered pairs, total pairs, both scores) and both final metric values as doubles, the scores
of every document, no tolerance anywhere.

Shapes: k_lrk_epoch is one block of B = 1024 threads.  Beside k_rn_epoch's LDS caps (2048 weights, 9216 doubles of kept values, an X
tile of 8192 floats) it keeps the per-list arrays of LambdaRank (the rank, the ranked labels, the weight row, two scorer tables) in LDS
for lists of up to LRK_LIST = 1024 documents and in a global pool beyond.  The sets mix list lengths 1, 2, 63, 64, 65, B - 1, B, B + 1,
lists at and one past every cap, and the networks -layer 0, [1], [10] and [3, 2].

The learning rates are chosen per shape on the restatement (swap changes are small, so they are larger than RankNet's tests use) so that a
epoch moves the largest weight by 0.01 to 0.3, and every run with a hidden layer asserts that for each of its epochs on the restatement's
weights (with a validation set too: on the weights after every epoch, before any restore), which must all be finite.  The exceptions
are named where they stand: saturated starts (d() of a saturated output is about 1e-18) and the hand-built weight_0 data.
Without a hidden layer this cannot be asked: every pair is taken from both sides with the same lambda and no delta depends on a weight,
so the steps of a list cancel up to rounding (tests/test_lambdarank_cpu.py shows it on two documents); those runs assert the bits only."""
import logging

import numpy as np
import pytest

import lambdarank_restatement as LR
import linear_ext as E
import ranknet_restatement as RN
from ca_restatement import LiteralScorer
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, LambdaRank, ListNet, Neuron, RankerFactory, RankerType, RankNet, flatten, java_double_str, java_round
from ranklib_amd.metric import ERRScorer

pytestmark = pytest.mark.gpu

B, W_CAP, POOL, X_CAP, LRK_LIST = 1024, 2048, 9216, 8192, 1024      # kRnThreads, kRnMaxW, kRnPool, kRnXCap, kLrkList (rl_rn.inc)
CHAIN_LIST = 4096                                                   # kLrkChainList
_STATICS = ("nIteration", "nHiddenLayer", "nHiddenNodePerLayer", "learningRate", "seed")


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = ([getattr(RankNet, k) for k in _STATICS], LambdaRank.lamseed, ListNet.seed, Neuron.learningRate, ERRScorer.MAX, DataPoint.missingZero,
             evaluator.Evaluator.normalize, evaluator.Evaluator.qrelFile)
    yield
    for k, v in zip(_STATICS, saved[0]):
        setattr(RankNet, k, v)
    (LambdaRank.lamseed, ListNet.seed, Neuron.learningRate, ERRScorer.MAX, DataPoint.missingZero, evaluator.Evaluator.normalize,
     evaluator.Evaluator.qrelFile) = saved[1:]


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def _u64(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64).tolist()


def _data(rng, lengths, F, labels=(0, 1, 2), prefix="q", scale=1.0, equal=()):
    """equal: the lists whose labels are all the same (no pairs; their steps are still taken)"""
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(qoff[-1])
    X = (rng.standard_normal((n, F)) * scale).astype(np.float32)
    X[rng.random(X.shape) < 0.15] = 0.0
    lab = rng.choice(np.array(labels, np.float32), n).astype(np.float32)
    for q in equal:
        lab[qoff[q]:qoff[q + 1]] = 2.0
    return X, lab, qoff, ["%s%d" % (prefix, i) for i in range(len(lengths))]


def _nw(F, hidden):
    n = [F] + list(hidden) + [1]
    return sum(n[l] * (n[l - 1] + 1) for l in range(1, len(n)))


def _gpu(train, valid, start, epochs, lr, hidden, metric="NDCG", k=10, err_max=16.0, arrays=None):
    t = E.feed(N.RankNetTrainer(n_epochs=epochs, learning_rate=lr, hidden_sizes=hidden, metric=metric, metric_k=k, err_max=err_max,
                                lambdarank=True), train, valid, **(arrays or {}))
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


def _run(train, valid=None, hidden=(10,), seed=3, epochs=2, lr=1.0, metric="NDCG", k=10, start=None, moves=True, err_max=16.0, arrays=None,
         **judged):
    """moves: every epoch has to move the largest weight by 0.01 to 0.3 (the weights after each epoch, before any restore)"""
    F = train[0].shape[1]
    start = RN.draw_weights(RN.build(F, hidden), seed).abi_weights() if start is None else np.array(start, np.float64)
    assert len(start) == _nw(F, hidden)
    r = LR.learn(train, valid, metric, k, n_iteration=epochs, lr=lr, hidden=hidden, start=start, err_max=err_max, **judged)
    assert np.all(np.isfinite(r["weight"]))
    if moves:
        ew = r["epoch_weights"]
        steps = [float(np.max(np.abs(ew[e] - ew[e - 1]))) for e in range(1, len(ew))]
        print("largest weight moved per epoch by", ", ".join("%.4g" % v for v in steps))
        assert len(steps) == epochs and all(0.01 <= v <= 0.3 for v in steps), steps
    t = _gpu(train, valid, start, epochs, lr, list(hidden), metric, k, err_max, arrays)
    t.learn()
    _same_run(t, r, valid is not None)
    return t, r, start


def test_list_lengths_around_the_wavefront_and_the_block():
    """every length once among short lists, one list with equal labels: no pairs, its steps are still taken"""
    rng = np.random.default_rng(50)
    lengths = [1, 2, 63, 64, 65, 7, B - 1, 70, B, 65, 66, B + 1, 12, 3]
    assert LRK_LIST == B                                      # B + 1 is also the first length whose LambdaRank arrays are global
    _run(_data(rng, lengths, 3, equal=[7]), None, hidden=[2], epochs=1, lr=LRS["lengths"])


@pytest.mark.parametrize("top", ["highest", "lowest"])
def test_a_top_document_with_the_unique_highest_or_lowest_label(top):
    """the first list is ranked with the start weights: the document they put on top gets the unique highest label (every target of its
    step is 1) or the unique lowest (every target 0)"""
    rng = np.random.default_rng(51)
    X, lab, qoff, qid = _data(rng, [70, 9], 3, labels=(1, 2))
    start = RN.draw_weights(RN.build(3, [2]), 3).abi_weights()
    W, at = [], 0
    for n_l, n_s in ((2, 3), (1, 2)):
        W.append(start[at:at + n_l * (n_s + 1)].reshape(n_l, n_s + 1))
        at += n_l * (n_s + 1)
    first = LR.rank([float(v) for v in RN.scores(W, X[:70])])[0]
    lab[first] = 3.0 if top == "highest" else 0.0
    _run((X, lab, qoff, qid), None, hidden=[2], epochs=1, lr=LRS["top"], start=start)


_METRICS = [("NDCG", 10), ("NDCG", 3), ("DCG", 10), ("MAP", 0), ("ERR", 10), ("ERR", 2)]
_NETS = [(h, m, k, (a + b) % 2 == 1) for a, h in enumerate(([], [1], [10], [3, 2])) for b, (m, k) in enumerate(_METRICS)]


@pytest.mark.parametrize("hidden,metric,k,valid", _NETS, ids=["%s-%s%d%s" % ("h" + "-".join(map(str, h)) if h else "layer0", m, k, "-v" if v else "")
                                                                for h, m, k, v in _NETS])
def test_networks_and_metrics(hidden, metric, k, valid):
    """lists shorter than k, of k and of k + 1 documents and longer ones"""
    rng = np.random.default_rng(60 + len(hidden) + sum(hidden))
    lengths = [1, 2, 3, 4, 9, 10, 11] + [int(v) for v in rng.integers(1, 40, 8)] + [65, 130]
    tr = _data(rng, lengths, 5, labels=(0, 1, 2, 3, 4))
    va = _data(rng, rng.integers(2, 30, 8), 5, prefix="v") if valid else None
    _run(tr, va, hidden=hidden, epochs=2, metric=metric, k=k, lr=LRS["nets", tuple(hidden), metric, k], moves=bool(hidden))


def test_some_epochs_save_and_others_do_not():
    """found on the restatement: a seed at which the validation score rises in a later epoch and not in another"""
    rng = np.random.default_rng(78)
    tr = _data(rng, rng.integers(2, 20, 12), 4)
    va = _data(rng, rng.integers(2, 20, 6), 4, prefix="v")
    for seed in range(12):
        start = RN.draw_weights(RN.build(4, [3]), seed).abi_weights()
        r = LR.learn(tr, va, "NDCG", 10, n_iteration=3, lr=LRS["saves"], hidden=[3], start=start)
        flags = [rec[1] for rec in r["trace"]]
        if flags[0] == 1 and 0 in flags and sum(flags) >= 2:
            break
    else:
        pytest.fail("no seed below 12 gives a run that saves in some later epoch and not in another")
    _run(tr, va, hidden=[3], epochs=3, lr=LRS["saves"], start=start)


def test_identical_rows_and_saturated_outputs_tie_and_the_given_order_decides():
    rng = np.random.default_rng(75)
    X, lab, qoff, qid = _data(rng, [5, 9, 70, 3], 3)
    X[[6, 11, 13]] = X[5]                                     # identical rows placed apart, in one list, with different labels
    lab[[5, 6, 11, 13]] = [0, 2, 1, 2]
    _run((X, lab, qoff, qid), None, hidden=[2], epochs=2, lr=LRS["ties"])
    X[:, 0] = 1.0
    for wsum in (40.0, -800.0):                               # both hidden neurons saturate: every output of a list is the same
        start = np.zeros(_nw(3, [2]))
        start[0] = start[4] = wsum
        _run((X, lab, qoff, qid), None, hidden=[2], epochs=2, start=start, moves=False, lr=LRS["ties"])
        _run((X, lab, qoff, qid), None, hidden=[], epochs=2, start=[wsum, 0.0, 0.0, 0.0], moves=False, lr=LRS["ties"])


def test_the_given_order_matters_only_among_tied_outputs():
    """the lists are re-ranked, so two documents that change places change nothing -- unless their outputs tie: with a saturated start
    the whole list ties, the rank keeps the given order, and the same exchange changes the weights"""
    rng = np.random.default_rng(76)
    X, lab, qoff, qid = _data(rng, [9, 12], 4)
    X[:, 0] = 1.0
    lab[[2, 5]] = [0, 2]
    rows = np.arange(21)
    rows[[2, 5]] = rows[[5, 2]]
    t1, r1, _ = _run((X, lab, qoff, qid), None, hidden=[3], epochs=1, lr=LRS["order"])
    t2, r2, _ = _run((X[rows], lab[rows], qoff, qid), None, hidden=[3], epochs=1, lr=LRS["order"])
    assert _u64(t1.weights()) == _u64(t2.weights())
    tied = [40.0, 0.0, 0.0, 0.0, 0.0]
    t3, r3, _ = _run((X, lab, qoff, qid), None, hidden=[], epochs=1, lr=LRS["order"], start=tied, moves=False)
    t4, r4, _ = _run((X[rows], lab[rows], qoff, qid), None, hidden=[], epochs=1, lr=LRS["order"], start=tied, moves=False)
    assert _u64(t3.weights()) != _u64(t4.weights())


def test_the_weight_0_quirk():
    train, start = LR.quirk_data()
    _run(train, None, hidden=[1], epochs=1, lr=0.5, metric="NDCG", k=2, start=start, moves=False)


def test_more_weights_than_threads():
    rng = np.random.default_rng(70)
    F = 110                                                   # 111 * 10 + 11 = 1121 weights: the update takes two rounds
    assert B < _nw(F, [10]) <= W_CAP
    _run(_data(rng, [9, 30, 1, 17, 66], F), None, hidden=[10], epochs=1, lr=LRS["w1121"])


def test_more_weights_than_the_lds_holds():
    rng = np.random.default_rng(71)
    assert _nw(205, [10]) > W_CAP >= _nw(202, [10])
    _run(_data(rng, [5, 40, 1, 13], 205), None, hidden=[10], epochs=1, lr=LRS["w2071"])      # 2071 weights: k_lrk_epoch<false>
    _run(_data(rng, [5, 40, 1, 13], 202), None, hidden=[10], epochs=1, lr=LRS["w2041"])      # 2041: the largest of these that stays in LDS


def test_lists_at_and_above_the_lds_caps():
    rng = np.random.default_rng(72)
    need = lambda n, H: 3 * n * H + n + H                     # noqa: E731
    assert need(270, 11) <= POOL < need(271, 11)
    _run(_data(rng, [270, 5, 271, 1, 269], 3, labels=(0, 0, 0, 1)), None, hidden=[10], epochs=1, lr=LRS["pool"])      # the kept values of list 2 are global
    assert 30 * (273 | 1) <= X_CAP < 30 * (274 | 1) and need(274, 2) <= POOL
    _run(_data(rng, [273, 4, 274, 9], 30, labels=(0, 0, 0, 1)), None, hidden=[1], epochs=1, lr=LRS["xcap"])          # the X tile of list 2 is not staged
    assert need(LRK_LIST + 1, 2) <= POOL
    for metric, k in (("MAP", 0), ("ERR", 10)):               # the rank, the weight row and the tables of list 2 are global (NDCG: the lengths test)
        _run(_data(rng, [LRK_LIST, 6, LRK_LIST + 1, 2], 2, labels=(0, 0, 0, 1, 2)), None, hidden=[1], epochs=1, metric=metric, k=k,
             lr=LRS["lrk", metric])


_FRACTIONAL = (0, 0.5, 1, 1.5, 2.99)


@pytest.mark.parametrize("labels,metric,k", [(_FRACTIONAL, "NDCG", 10), (_FRACTIONAL, "MAP", 0), (_FRACTIONAL, "ERR", 10), ((0, 30), "NDCG", 10),
                                             ((0, 30), "MAP", 0)], ids=["fractional-NDCG", "fractional-MAP", "fractional-ERR", "30-NDCG", "30-MAP"])
def test_labels(labels, metric, k):
    """0 and 0.5 are a pair (the floats differ) whose NDCG and ERR weight is 0 (the gains come from (int) label); label 30 is a gain of
    2^30 - 1.  (ERR with label 30 has R = (2^30 - 1) / 16: its swap changes leave the float range, which is the refusal tested below.)"""
    rng = np.random.default_rng(74)
    tr = _data(rng, rng.integers(1, 40, 20), 4, labels=labels)
    va = _data(rng, rng.integers(2, 40, 8), 4, labels=labels, prefix="v")
    _run(tr, va, hidden=[3], epochs=2, metric=metric, k=k, lr=LRS["labels", metric, labels[-1]])


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_external_judgments(metric, k):
    rng = np.random.default_rng(82)
    tr = _data(rng, rng.integers(2, 30, 20), 4)
    va = _data(rng, rng.integers(2, 30, 8), 4, prefix="v")
    m = E.ideal_map([tr, va], k, rng) if metric == "NDCG" else E.count_map([tr, va], rng)
    if metric == "MAP":
        m[tr[3][1]] = 0                                       # rdCount == 0: that list's matrix is zero
        assert any(q not in m for q in tr[3])                 # and a list the file does not name counts 0 too
    arrays, judged = E.judgments(metric, m, tr, va, "both")
    t, r, start = _run(tr, va, hidden=[3], epochs=2, metric=metric, k=k, lr=LRS["qrel", metric], arrays=arrays, **judged)
    plain = LR.learn(tr, va, metric, k, n_iteration=2, lr=LRS["qrel", metric], hidden=[3], start=start)
    assert _u64(plain["weight"]) != _u64(r["weight"])


def test_a_swap_change_that_is_not_finite_is_refused_with_the_epoch():
    """ERR with MAX = 1 (-gmax 0) and labels {0, 1}: R(1) = 1, so 1 - R = 0 divides in swapChange's last term.  ERR with MAX = 16 and
    labels {0, 30}: R(30) = (2^30 - 1) / 16, and the chains' products leave the float range of the pair weight"""
    rng = np.random.default_rng(79)
    for labels, err_max in (((0, 1), 1.0), ((0, 30), 16.0)):
        tr = _data(rng, rng.integers(2, 12, 6), 3, labels=labels)
        start = RN.draw_weights(RN.build(3, [2]), 3).abi_weights()
        with pytest.raises(OverflowError) as want:            # the restatement overflows first, on the CPU
            LR.learn(tr, None, "ERR", 10, n_iteration=3, lr=0.5, hidden=[2], start=start, err_max=err_max)
        assert str(want.value) == "epoch 1"
        t = _gpu(tr, None, start, 3, 0.5, [2], "ERR", 10, err_max=err_max)
        with pytest.raises(N.RankLibError) as e:
            t.learn()
        assert "status -4" in str(e.value) and "LambdaRank" in str(e.value) and "after %s " % want.value in str(e.value)


def test_refusals_on_a_handle():
    rng = np.random.default_rng(81)
    tr = _data(rng, [4, 5], 3)
    L = N.lib()
    for metric in ("P", "RR"):                                # their swap changes are not built
        with pytest.raises(N.RankLibError) as e:
            N.RankNetTrainer(n_epochs=1, hidden_sizes=[2], metric=metric, lambdarank=True)
        assert "status -4" in str(e.value) and "NDCG, DCG, MAP, ERR" in str(e.value) and "LambdaRank" in str(e.value)
        t = N.RankNetTrainer(n_epochs=1, hidden_sizes=[2], metric=metric)
        assert L.rl_rn_set_lambdarank(t.h, 0) == 0 and L.rl_rn_set_lambdarank(t.h, 1) == -4
        t.close()
    t = E.feed(N.RankNetTrainer(n_epochs=1, hidden_sizes=[2], lambdarank=True), tr)
    t.set_weights(np.zeros(11))
    t.learn()
    assert L.rl_rn_set_lambdarank(t.h, 0) == -3 and L.rl_rn_set_lambdarank(t.h, 1) == -3      # RL_ERR_STATE after learn
    assert b"rl_rn_set_lambdarank after rl_rn_learn" in L.rl_last_error()
    # MAP walks a serial chain per pair: lists beyond CHAIN_LIST documents are refused before anything is uploaded; NDCG takes them
    long = _data(rng, [CHAIN_LIST + 1, 3], 1)
    for metric, refused in (("MAP", True), ("NDCG", False)):
        t = E.feed(N.RankNetTrainer(n_epochs=0, hidden_sizes=[], metric=metric, metric_k=0 if metric == "MAP" else 10, lambdarank=True), long)
        t.set_weights(np.zeros(2))
        if refused:
            with pytest.raises(N.RankLibError) as e:
                t.learn()
            assert "status -4" in str(e.value) and str(CHAIN_LIST) in str(e.value) and "MAP" in str(e.value)
        else:
            t.learn()
        t.close()
    # switched off again before learning, the handle trains RankNet
    start = RN.draw_weights(RN.build(3, [2]), 3).abi_weights()
    t = E.feed(N.RankNetTrainer(n_epochs=1, learning_rate=0.05, hidden_sizes=[2], lambdarank=True), tr)
    assert L.rl_rn_set_lambdarank(t.h, 0) == 0
    t.set_weights(start)
    t.learn()
    assert _u64(t.weights()) == _u64(RN.learn(tr, None, "NDCG", 10, n_iteration=1, lr=0.05, hidden=[2], start=start)["weight"])


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


def test_command_line_train_save_load_test(tmp_path, caplog):
    F = 4
    train, valid, test = _files(tmp_path)
    m1 = str(tmp_path / "m1.txt")
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        evaluator.main(["-train", train, "-ranker", "5", "-lamseed", "3", "-epoch", "2", "-lr", "2.0", "-metric2t", "NDCG@10", "-validate", valid,
                        "-save", m1])
    assert tuple(getattr(RankNet, s) for s in _STATICS) == (100, 1, 10, 0.00005, None) and LambdaRank.lamseed is None
    assert Neuron.learningRate == 0.001
    _, tr = _read(train, F)
    _, va = _read(valid, F)
    lists_te, te = _read(test, F)
    r = LR.learn(tr, va, "NDCG", 10, n_iteration=2, lr=2.0, hidden=[10], seed=3)
    text = open(m1).read()
    assert text == LR.model_text(r["weight"], list(range(1, F + 1)), [10], 2) and text.startswith("## LambdaRank\n## Epochs = 2\n")
    lines = [rec.getMessage() for rec in caplog.records]
    for rec in r["trace"]:                                    # the printed columns: epoch, round(mis-ordered / total, 4), both scores rounded
        cols = [str(rec[0]), java_double_str(java_round(rec[2] / rec[3], 4)), java_double_str(java_round(rec[4], 4)),
                java_double_str(java_round(rec[5], 4))]
        assert any([c.strip() for c in ln.split("|")][:4] == [c[:w] for c, w in zip(cols, (7, 14, 9, 9))] for ln in lines), cols
    loaded = RankerFactory().loadRankerFromFile(m1)           # the saved file loads again with the same bits
    assert type(loaded) is LambdaRank and loaded.hidden == [10]
    assert _u64(np.concatenate([m.ravel() for m in loaded.weights])) == _u64(r["weight"])
    e = evaluator.Evaluator(RankerType.LAMBDAMART, "NDCG@10", "NDCG@10")
    want = LiteralScorer("NDCG", 10).score([float(v) for v in RN.scores(r["matrices"], te[0])], te[1], te[2], te[3])
    assert _bits(e.test(m1, test)) == _bits(want)
    net = N.NetModel(list(range(1, F + 1)), [10], r["weight"])      # rl_net_predict's bits
    rows = np.zeros((te[0].shape[0], F + 1), np.float32)
    rows[:, 1:] = te[0]
    assert _bits(np.concatenate([loaded.evalList(rl) for rl in lists_te])) == _bits(net.predict_rows(rows))
    # the Python class: rounded training score, the validation score as it is, the model text
    LambdaRank.lamseed, RankNet.nIteration, RankNet.nHiddenNodePerLayer, RankNet.learningRate, RankNet.nHiddenLayer = 7, 2, 3, 2.0, 2
    ranker = evaluator.Evaluator(RankerType.LAMBDARANK, "MAP", "MAP").evaluate(train, valid)
    r2 = LR.learn(tr, va, "MAP", 0, n_iteration=2, lr=2.0, hidden=[3, 3], seed=7)
    assert type(ranker) is LambdaRank and ranker.hidden == [3, 3] and ranker.name() == "LambdaRank"
    assert _u64(np.concatenate([m.ravel() for m in ranker.weights])) == _u64(r2["weight"])
    assert ranker.getScoreOnTrainingData() == java_round(r2["train"], 4) and _bits(ranker.getScoreOnValidationData()) == _bits(r2["valid"])
    assert ranker.model() == LR.model_text(r2["weight"], list(range(1, F + 1)), [3, 3], 2)


def test_command_line_kcv_and_refusals(tmp_path):
    train, valid, test = _files(tmp_path, seed=22)
    evaluator.main(["-train", train, "-ranker", "5", "-lamseed", "3", "-epoch", "1", "-node", "2", "-kcv", "2", "-metric2t", "MAP"])
    assert LambdaRank.lamseed is None
    for refused in (["-ranker", "5", "-rnseed", "3"], ["-ranker", "5"], ["-ranker", "5", "-netseed", "3"]):
        with pytest.raises(N.RankLibError) as e:
            evaluator.main(["-train", train] + refused)
        assert "out of scope" in str(e.value) and "-lamseed" in str(e.value)
    with pytest.raises(N.RankLibError) as e:
        evaluator.main(["-train", train, "-ranker", "5", "-lamseed", "3", "-metric2t", "P@10"])
    assert "NDCG, DCG, MAP, ERR" in str(e.value)


# the learning rates, chosen on the restatement (see the module's docstring)
LRS = {"top": 2.1, ("qrel", "NDCG"): 6.0, ("qrel", "MAP"): 3.9, "ties": 3.4, ("labels", "NDCG", 2.99): 7.7, ("labels", "MAP", 2.99): 7.5,
       ("labels", "ERR", 2.99): 3.3, ("labels", "NDCG", 30): 6.0, ("labels", "MAP", 30): 8.4, "lengths": 0.23, "pool": 0.46, "xcap": 0.6,
       ("lrk", "MAP"): 0.98, ("lrk", "ERR"): 0.86, "w2071": 1.3, "w2041": 2.5, "w1121": 1.1, "saves": 15.0, "order": 45.0,
       # -layer 0: the steps of a list cancel, any rate serves
       ("nets", (), "NDCG", 10): 1.0, ("nets", (), "NDCG", 3): 1.0, ("nets", (), "DCG", 10): 1.0, ("nets", (), "MAP", 0): 1.0,
       ("nets", (), "ERR", 10): 1.0, ("nets", (), "ERR", 2): 1.0,
       ("nets", (1,), "NDCG", 10): 2.5, ("nets", (1,), "NDCG", 3): 0.8, ("nets", (1,), "DCG", 10): 0.0025, ("nets", (1,), "MAP", 0): 6.7,
       ("nets", (1,), "ERR", 10): 0.5, ("nets", (1,), "ERR", 2): 0.5,
       ("nets", (10,), "NDCG", 10): 4.9, ("nets", (10,), "NDCG", 3): 1.3, ("nets", (10,), "DCG", 10): 0.0013, ("nets", (10,), "MAP", 0): 5.0,
       ("nets", (10,), "ERR", 10): 0.46, ("nets", (10,), "ERR", 2): 0.27,
       ("nets", (3, 2), "NDCG", 10): 5.0, ("nets", (3, 2), "NDCG", 3): 3.6, ("nets", (3, 2), "DCG", 10): 0.003, ("nets", (3, 2), "MAP", 0): 11.0,
       ("nets", (3, 2), "ERR", 10): 13.0, ("nets", (3, 2), "ERR", 2): 16.0}
