"""ListNet training (-ranker 7) without a GPU: java.util.Random and Synapse's draw, one update step re-derived operation by operation, the
save rule and the restore's exception in the restatement, the gating behind ListNet.seed / -netseed with the statics restored, and the
argument refusals that precede the device check."""
import ctypes as C

import numpy as np
import pytest

import listnet_restatement as LN
from np_restatement import jexp
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd._native import RankLibError
from ranklib_amd.learning import LambdaRank, ListNet, Neuron, RankerFactory, RankerType, RankNet


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = (ListNet.seed, ListNet.nIteration, ListNet.learningRate, Neuron.learningRate)
    yield
    ListNet.seed, ListNet.nIteration, ListNet.learningRate, Neuron.learningRate = saved


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def test_java_random_anchors_and_the_draw():
    for cls in (learning.JavaRandom, LN.JavaRandom):
        assert cls(0).nextInt() == -1155484576 and cls(42).nextInt() == -1170105035      # new Random(seed).nextInt()
        r = cls(7)
        for _ in range(50):
            assert r.nextInt(2) in (0, 1)
            f = r.nextFloat()
            assert isinstance(f, np.float32) and 0.0 <= f < 1.0 and float(f) * (1 << 24) == int(float(f) * (1 << 24))
    a, b = learning.JavaRandom(5), LN.JavaRandom(5)
    assert [a.nextInt(2) for _ in range(20)] == [b.nextInt(2) for _ in range(20)] and a.nextFloat() == b.nextFloat()
    assert [learning.JavaRandom(9).nextInt(10) for _ in range(3)] == [LN.JavaRandom(9).nextInt(10) for _ in range(3)]


@pytest.mark.parametrize("seed", [0, 3, 42, -17, 2 ** 40 + 1])
def test_start_weights_are_floats_widened_in_wire_order(seed):
    F = 6
    w = ListNet.initial_weights(seed, F + 1)
    assert _bits(w) == _bits(LN.draw_weights(seed, F + 1))
    assert all(float(np.float32(v)) == v for v in w) and all(abs(v) < 0.1 for v in w) and len(set(w.tolist())) > 1
    # two draws per synapse, nextInt(2) then nextFloat(), inputs first and the bias last: re-derived draw by draw
    r = LN.JavaRandom(seed)
    as_double = []
    for k in range(F + 1):
        sign = 1 if r.nextInt(2) == 0 else -1
        f = r.nextFloat()
        assert w[k] == float(np.float32(np.float32(sign * f) / np.float32(10)))
        as_double.append(sign * float(f) / 10.0)
    assert w.tolist() != as_double                            # a float division by 10, not a double one
    # every init() starts from the seed: a shorter network is a prefix
    assert _bits(ListNet.initial_weights(seed, 3)) == _bits(w[:3])


def test_one_update_step_by_hand():
    x0, x1 = np.float32(0.7), np.float32(-1.3)
    l0, l1 = np.float32(2.0), np.float32(0.0)
    w, b, lr = 0.25, -0.5, 0.5
    X, lab = np.array([[x0], [x1]], np.float32), np.array([l0, l1], np.float32)
    weight = [w, b]
    LN.epoch(X, lab, [0, 2], weight, lr)
    # feedForward
    s0 = 0.0
    s0 += float(x0) * w
    s0 += 1.0 * b
    o0 = 1.0 / (1.0 + jexp(-s0))
    s1 = 0.0
    s1 += float(x1) * w
    s1 += 1.0 * b
    o1 = 1.0 / (1.0 + jexp(-s1))
    # computeDelta
    sl = 0.0
    sl += jexp(2.0)
    sl += jexp(0.0)
    ss = 0.0
    ss += jexp(o0)
    ss += jexp(o1)
    d0 = jexp(2.0) / sl - jexp(o0) / ss
    d1 = jexp(0.0) / sl - jexp(o1) / ss
    # updateWeight
    dw = 0.0
    dw += d0 * float(x0)
    dw += d1 * float(x1)
    dw *= lr
    db = 0.0
    db += d0 * 1.0
    db += d1 * 1.0
    db *= lr
    assert _bits(weight) == _bits([w + dw, b + db]) and weight != [w, b]
    again = [w, b]
    LN.epoch_vector(X, lab, [0, 2], again, lr)
    assert _bits(again) == _bits(weight)


def test_a_one_document_list_leaves_the_weights_unchanged():
    X, lab = np.array([[0.3, -2.0]], np.float32), np.array([3.0], np.float32)
    weight = [0.05, -0.07, 0.01]
    LN.epoch(X, lab, [0, 1], weight, 0.5)                     # d1 = d2 = 1: every dw is 0.0
    assert _bits(weight) == _bits([0.05, -0.07, 0.01])


def test_both_forms_of_the_epoch_agree():
    rng = np.random.default_rng(4)
    qoff = np.concatenate([[0], np.cumsum(rng.integers(1, 9, 12))])
    X = rng.standard_normal((qoff[-1], 5)).astype(np.float32)
    lab = rng.integers(0, 5, qoff[-1]).astype(np.float32)
    a, b = LN.draw_weights(3, 6), LN.draw_weights(3, 6)
    for _ in range(2):
        LN.epoch(X, lab, qoff, a, 0.5)
        LN.epoch_vector(X, lab, qoff, b, 0.5)
    assert _bits(a) == _bits(b) and _bits(a) != _bits(LN.draw_weights(3, 6))


def _sets():
    rng = np.random.default_rng(8)
    qoff = np.concatenate([[0], np.cumsum(rng.integers(2, 9, 10))]).astype(np.int32)
    X = rng.standard_normal((qoff[-1], 3)).astype(np.float32)
    lab = rng.integers(0, 3, qoff[-1]).astype(np.float32)
    qv = np.array([0, 4, 9], np.int32)
    Xv = rng.standard_normal((9, 3)).astype(np.float32)
    lv = np.array([1, 0, 0, 0, 0, 2, 0, 0, 0], np.float32)
    return (X, lab, qoff, ["q%d" % i for i in range(10)]), (Xv, lv, qv, ["v0", "v1"])


def test_the_save_rule_is_strict_and_the_restore_throws():
    tr, va = _sets()
    r = LN.learn(tr, va, "NDCG", 10, n_iteration=4, lr=0.5, seed=3)
    best = 0.0
    for ep, saved, _, v in r["trace"]:
        assert saved == (1 if v > best else 0)
        best = max(best, v)
    assert sum(s for _, s, _, _ in r["trace"]) >= 1
    # a learning rate of 0.0 leaves every epoch at the same score: only the first is saved, a tie never replaces it
    r0 = LN.learn(tr, va, "NDCG", 10, n_iteration=3, lr=0.0, seed=3)
    assert [s for _, s, _, _ in r0["trace"]] == [1, 0, 0] and len({v for _, _, _, v in r0["trace"]}) == 1
    assert _bits(r0["weight"]) == _bits(LN.draw_weights(3, 4))
    # no relevant document in the validation set: no epoch scores above 0.0, nothing is saved, the restore throws
    dead = (va[0], np.zeros_like(va[1]), va[2], va[3])
    with pytest.raises(LN.RestoreError) as e:
        LN.learn(tr, dead, "NDCG", 10, n_iteration=2, lr=0.5, seed=3)
    assert str(e.value).startswith("Error in NeuralNetwork.restoreBestModelOnValidation(): ")
    with pytest.raises(LN.RestoreError):                      # -epoch 0 with a validation set
        LN.learn(tr, va, "NDCG", 10, n_iteration=0, lr=0.5, seed=3)
    assert _bits(LN.learn(tr, None, "NDCG", 10, n_iteration=0, seed=3)["weight"]) == _bits(LN.draw_weights(3, 4))


def test_model_text_of_the_restatement_is_the_classes():
    w = LN.draw_weights(11, 4)
    r = ListNet()
    r.features, r.hidden, r.weights = [4, 2, 9], [], [np.array(w).reshape(1, 4)]
    ListNet.nIteration = 5
    assert r.model() == LN.model_text(w, [4, 2, 9], 5) and "## Epochs = 5\n" in r.model()
    loaded = RankerFactory().loadRankerFromString(r.model())
    assert _bits(loaded.weights[0]) == _bits(w)


def test_without_a_seed_everything_is_refused_as_before(tmp_path):
    assert ListNet.seed is None
    data = tmp_path / "d.txt"
    data.write_text("1 qid:1 1:1 2:0\n0 qid:1 1:0 2:1\n")
    for n in ("1", "5", "7"):
        with pytest.raises(RankLibError) as e:
            evaluator.main(["-train", str(data), "-ranker", n])
        assert "-ranker 9 (Linear Regression)" in str(e.value) and "neural-net" in str(e.value) and "only" in str(e.value)
        assert "-ranker 2 (RankBoost)" in str(e.value) and "out of scope" in str(e.value)
        assert ("-netseed" in str(e.value)) == (n == "7")
    for bad in (["-netseed", "3", "-ranker", "1"], ["-netseed", "3", "-ranker", "5"]):      # the seed opens ListNet only
        with pytest.raises(RankLibError) as e:
            evaluator.main(["-train", str(data)] + bad)
        assert "out of scope" in str(e.value)
    f = RankerFactory()
    with pytest.raises(RankLibError) as e:
        f.createRanker(RankerType.LISTNET)
    assert "LISTNET" in str(e.value) and "out of scope" in str(e.value) and "ListNet.seed" in str(e.value)
    r = f.loadRankerFromString("## ListNet\n1\n0\n0 0 1.0\n0 1 0.0\n")
    for call in (r.init, r.learn, ListNet().learn, ListNet().init):
        with pytest.raises(RankLibError) as e:
            call()
        assert "out of scope" in str(e.value) and "neural-net" in str(e.value) and "LISTNET" in str(e.value)
    ListNet.seed = 3
    assert type(f.createRanker(RankerType.LISTNET)) is ListNet and type(f.createRanker("LISTNET")) is ListNet
    for t in (RankerType.RANKNET, RankerType.LAMBDARANK):    # the other two stay refused whatever the seed
        with pytest.raises(RankLibError):
            f.createRanker(t)
    with pytest.raises(RankLibError):
        RankNet().init()
    with pytest.raises(RankLibError):
        LambdaRank().learn()


def test_cli_statics_are_set_for_the_run_and_restored(monkeypatch):
    seen = []
    real = evaluator.Evaluator.__init__

    def spy(self, rtype, *a, **k):
        seen.append((rtype, ListNet.nIteration, ListNet.learningRate, ListNet.seed, RankNet.nIteration, RankNet.learningRate))
        real(self, rtype, *a, **k)
    monkeypatch.setattr(evaluator.Evaluator, "__init__", spy)
    with pytest.raises(RankLibError):                        # the reader refuses the missing file after the flags are parsed
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "7", "-netseed", "3", "-epoch", "2", "-lr", "0.5"])
    assert seen == [(RankerType.LISTNET, 2, 0.001, 3, 100, 0.00005)]      # -lr x gives Neuron.learningRate, not x
    assert (ListNet.nIteration, ListNet.seed, ListNet.learningRate, Neuron.learningRate) == (1500, None, 0.00001, 0.001)
    with pytest.raises(RankLibError):                        # without -lr: ListNet's own default
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "7", "-netseed", "-9"])
    assert seen[-1] == (RankerType.LISTNET, 1500, 0.00001, -9, 100, 0.00005)
    assert (ListNet.nIteration, ListNet.seed, ListNet.learningRate) == (1500, None, 0.00001)
    # with another ranker -netseed, -epoch and -lr are parsed and change nothing
    with pytest.raises(RankLibError):
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "6", "-netseed", "3", "-epoch", "10", "-lr", "0.5"])
    assert seen[-1] == (RankerType.LAMBDAMART, 1500, 0.00001, None, 100, 0.00005)
    assert (RankNet.nIteration, LambdaRank.nIteration, ListNet.nIteration) == (100, 100, 1500) and ListNet.seed is None


def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    L = N.lib()
    for own in (dict(n_epochs=-1), dict(learning_rate=float("nan")), dict(learning_rate=float("inf"))):
        with pytest.raises(RankLibError) as e:
            N.ListNetTrainer(**own)
        assert "status -1" in str(e.value), own            # RL_ERR_INVALID
    p = N.RlLnParams()
    L.rl_ln_params_default(C.byref(p))
    assert (p.n_epochs, p.learning_rate, p.metric, p.metric_k, p.device, p.err_max) == (1500, 0.00001, 0, 10, 0, 16.0)
    h = C.c_void_p()
    assert L.rl_ln_create(None, C.byref(h)) == -1 and L.rl_ln_create(C.byref(p), None) == -1
    assert L.rl_ln_learn(None) == -1 and L.rl_ln_set_weights(None, None, 0) == -1
    n = C.c_int32(0)
    assert L.rl_ln_get_weights(None, None, 0, C.byref(n)) == -1
    with pytest.raises(RankLibError):                        # the metric is checked before the device too
        N.ListNetTrainer(metric="BEST")
