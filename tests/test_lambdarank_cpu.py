"""LambdaRank training (-ranker 5) without a GPU: the vector form of the restatement against the literal one, one step of a two-document
list written out operation by operation, the `weight_0` quirk of updateDelta, the stable rank under tied outputs, the swap changes of MAP
with an external count, the gating behind LambdaRank.lamseed / -lamseed with RankNet's statics set for the run and restored, the usage
text, the metric refusal and the C ABI's null-handle refusal."""
import numpy as np
import pytest

import ca_restatement as CR
import lambdarank_restatement as LR
import np_restatement as R
import ranknet_restatement as RN
from np_restatement import jexp
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd._native import RankLibError
from ranklib_amd.learning import DataPoint, LambdaRank, ListNet, Neuron, RankerFactory, RankerType, RankList, RankNet
from ranklib_amd.metric import MetricScorerFactory

_STATICS = ("nIteration", "nHiddenLayer", "nHiddenNodePerLayer", "learningRate", "seed")


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = ([getattr(RankNet, k) for k in _STATICS], LambdaRank.lamseed, ListNet.seed, Neuron.learningRate)
    yield
    for k, v in zip(_STATICS, saved[0]):
        setattr(RankNet, k, v)
    LambdaRank.lamseed, ListNet.seed, Neuron.learningRate = saved[1:]


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def _data(rng, lengths, F, labels=(0, 1, 2)):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    X = rng.standard_normal((int(qoff[-1]), F)).astype(np.float32)
    lab = rng.choice(np.array(labels, np.float32), int(qoff[-1])).astype(np.float32)
    return X, lab, qoff, ["q%d" % i for i in range(len(lengths))]


# ---- the restatement's two forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,k", [("NDCG", 3), ("DCG", 10), ("MAP", 0), ("ERR", 2)])
@pytest.mark.parametrize("hidden", [[], [1], [3, 2]], ids=["layer0", "h1", "h3-2"])
def test_the_vector_form_is_the_literal_form(hidden, metric, k):
    rng = np.random.default_rng(5 + len(hidden))
    tr = _data(rng, [1, 2, 7, 4, 9, 3], 3, labels=(0, 0.5, 1, 2, 3))
    tr[0][9] = tr[0][7]                                       # identical rows placed apart: their outputs tie
    va = _data(rng, [4, 6, 2], 3)
    rdc = {"q2": 0, "q3": 5, "q4": 2} if metric == "MAP" else None      # q0, q1, q5 have no entry: rdCount 0
    for valid, counts in ((None, None), (va, rdc)):
        kw = dict(metric=metric, k=k, n_iteration=2, lr=0.7, hidden=hidden, seed=4, rel_doc_count=counts, valid_rel_doc_count=None)
        a, b = LR.learn(tr, valid, vector=False, **kw), LR.learn(tr, valid, vector=True, **kw)
        assert _bits(a["weight"]) == _bits(b["weight"]) and a["trace"] == b["trace"]
        assert _bits(a["weight"]) != _bits(RN.draw_weights(RN.build(3, hidden), 4).abi_weights())
        assert _bits(a["weight"]) != _bits(RN.learn(tr, valid, metric, k, n_iteration=2, lr=0.7, hidden=hidden, seed=4)["weight"])


@pytest.mark.parametrize("metric,k,err_max", [("NDCG", 3, 16.0), ("DCG", 2, 16.0), ("MAP", 0, 16.0), ("ERR", 3, 16.0), ("ERR", 20, 16.0),
                                              ("ERR", 4, 1.0)])
def test_the_swap_changes_of_the_vector_form(metric, k, err_max):
    rng = np.random.default_rng(11)
    for n, labels in ((1, (0, 1)), (2, (0, 1)), (9, (0, 0.5, 1, 2, 3)), (6, (0, 0)), (12, (0, 1))):
        lab = rng.choice(np.array(labels, np.float32), n).astype(np.float32)
        for rdc in ((None, {"q": 0}, {"q": 7}, {}) if metric == "MAP" else (None,)):
            s = LR.Scorer(CR.LiteralScorer(metric, k, err_max, None, rdc), metric, k, rdc)
            lit = np.abs(np.array(s.swap_change(list(lab), "q"), np.float64)).reshape(n, n)
            assert np.array_equal(lit, s.swap_abs_vector(lab, "q"), equal_nan=True), (n, labels, rdc)


def test_map_divides_by_the_external_count():
    lab = [1.0, 0.0, 1.0, 0.0]
    own = np.array(LR.map_swap_change(lab, None))
    assert np.array_equal(own, np.array(R.MAP().swap_change(lab, "q")))               # without -qrel: the list's own count, 2
    assert np.array_equal(np.array(LR.map_swap_change(lab, 8)), own * 2 / 8) and own[0][1] != 0
    assert not np.any(np.array(LR.map_swap_change(lab, 0))) and not np.any(np.array(LR.map_swap_change([0.0, 0.0], 3)))


# ---- one step by hand --------------------------------------------------------------------------------------------------------------------------
def test_one_list_of_two_documents_by_hand():
    """-layer 0, F = 1, NDCG@10.  The weights are (w, b); the outputs are kept from the forward pass, so both steps use them.  The pair is
    taken twice, once from each side, with the same lambda (weight and pij both change sign), and without a hidden layer no delta depends
    on a weight: step 1 takes back what step 0 gave, as the Java does"""
    w, b, lr = 0.3, -0.1, 0.5
    X = np.array([[1.0], [2.0]], np.float32)                  # document 1 scores higher and is ranked first; it has the lower label
    lab = np.array([2.0, 0.0], np.float32)
    sig = lambda v: 1.0 / (1.0 + jexp(-v))                    # noqa: E731
    d = lambda o: sig(o) * (1.0 - sig(o))                     # noqa: E731
    x = [2.0, 1.0]                                            # the re-ranked list: positions 0, 1 = documents 1, 0; labels 2 -> 0, 0 -> 2
    o = [sig((0.0 + x[0] * w) + 1.0 * b), sig((0.0 + x[1] * w) + 1.0 * b)]
    assert o[0] > o[1]
    ideal = 3.0 * 1.0 + 0.0 * R.discount(1)
    change = (R.discount(0) - R.discount(1)) * (0.0 - 3.0) / ideal       # gains by position: label 0 first, label 2 second
    wf = [float(np.float32(abs(change)) * np.float32(-1)), float(np.float32(abs(change)) * np.float32(1))]      # step 0: label 0 < 2
    # step 0: i = position 0 (label 0), its pair j = 1, target 0
    lam = wf[0] * (0.0 - 1.0 / (1.0 + jexp(-(o[0] - o[1]))))
    delta_i, delta_j = (0.0 + lam) * d(o[0]), lam * d(o[1])
    w += lr * (delta_i * x[0] - (0.0 + delta_j * x[1]))
    b += lr * (delta_i * 1.0 - (0.0 + delta_j * 1.0))
    assert lam > 0 and w != 0.3 and b != -0.1
    # step 1: i = position 1 (label 2), its pair j = 0, target 1
    lam = wf[1] * (1.0 - 1.0 / (1.0 + jexp(-(o[1] - o[0]))))
    delta_i, delta_j = (0.0 + lam) * d(o[1]), lam * d(o[0])
    w += lr * (delta_i * x[1] - (0.0 + delta_j * x[0]))
    b += lr * (delta_i * 1.0 - (0.0 + delta_j * 1.0))
    for vector in (False, True):
        r = LR.learn((X, lab, np.array([0, 2], np.int32), ["q"]), None, "NDCG", 10, n_iteration=1, lr=lr, hidden=[], start=[0.3, -0.1],
                     vector=vector)
        assert _bits(r["weight"]) == _bits([w, b])
    assert abs(w - 0.3) < 1e-15 and abs(b + 0.1) < 1e-15


# ---- the weight_0 quirk ------------------------------------------------------------------------------------------------------------------------
def test_a_first_pair_of_weight_zero_zeroes_the_hidden_delta_i():
    train, start = LR.quirk_data()
    X, lab, qoff, qid = train
    net = RN.set_weights(RN.build(1, [1]), start)
    sc = CR.LiteralScorer("NDCG", 2)
    seen = {}

    def hook(q, net, pairMap, pairWeight, i):
        seen[(q, i)] = (pairMap[i], [float(v) for v in pairWeight[i]], net.layers[1][0].delta_i, list(net.layers[1][0].deltas_j),
                        net.layers[2][0].delta_i)
    LR.epoch(net, X, lab, qoff, qid, 0.5, LR.Scorer(sc, "NDCG", 2, None), hook)
    pm, pw, hid_i, hid_j, out_i = seen[(0, 2)]                # both positions of the first pair at or past k
    assert pm == [3, 4] and pw == [0.0, -0.0] and hid_i == 0.0 and out_i == 0.0
    pm, pw, hid_i, hid_j, out_i = seen[(0, 3)]                # the same document as j of earlier positions: pairs below the cut-off come first
    assert pm[0] == 0 and pw[0] != 0 and hid_i != 0.0
    pm, pw, hid_i, hid_j, out_i = seen[(1, 0)]                # labels 0.5 and 0: a pair with weight 0, first in its step
    assert pm == [1, 2, 3, 4, 5] and pw[0] == 0.0 and pw[1] != 0 and pw[2] != 0
    assert hid_i == 0.0 and out_i != 0.0 and hid_j[0] == 0.0 and hid_j[1] != 0.0
    r = LR.learn(train, None, "NDCG", 2, n_iteration=1, lr=0.5, hidden=[1], start=start, vector=True)
    assert _bits(r["weight"]) == _bits(net.abi_weights()) and _bits(r["weight"]) != _bits(start)


# ---- the rank ------------------------------------------------------------------------------------------------------------------------------------
def test_the_rank_is_stable_under_tied_outputs():
    assert LR.rank([0.5, 0.7, 0.5, 0.7, 0.1, 0.5]) == [1, 3, 0, 2, 5, 4]
    assert LR.rank([1.0] * 5) == [0, 1, 2, 3, 4] and LR.rank([]) == []
    assert list(np.argsort(-np.array([0.5, 0.7, 0.5, 0.7, 0.1, 0.5]), kind="stable")) == [1, 3, 0, 2, 5, 4]      # the vector form's
    # saturated outputs: the whole list ties and the order is the given one, so swapping two documents changes the run
    rng = np.random.default_rng(3)
    X, lab, qoff, qid = _data(rng, [6], 2, labels=(0, 1, 2))
    lab[:] = [0, 2, 1, 0, 2, 1]
    X[:, 0] = 1.0
    a = LR.learn((X, lab, qoff, qid), None, "NDCG", 10, n_iteration=1, lr=0.5, hidden=[], start=[40.0, 0.0, 0.0], vector=False)
    lab2 = lab.copy()
    lab2[[1, 2]] = lab2[[2, 1]]
    b = LR.learn((X, lab2, qoff, qid), None, "NDCG", 10, n_iteration=1, lr=0.5, hidden=[], start=[40.0, 0.0, 0.0], vector=False)
    assert _bits(a["weight"]) != _bits(b["weight"])


# ---- the gating --------------------------------------------------------------------------------------------------------------------------------
def test_lambdarank_trains_only_behind_its_own_seed(tmp_path):
    assert LambdaRank.lamseed is None and RankNet.seed is None
    data = tmp_path / "d.txt"
    data.write_text("1 qid:1 1:1 2:0\n0 qid:1 1:0 2:1\n")
    for extra in ([], ["-rnseed", "3"], ["-netseed", "3"]):  # -rnseed and -netseed do not open -ranker 5
        with pytest.raises(RankLibError) as e:
            evaluator.main(["-train", str(data), "-ranker", "5"] + extra)
        msg = str(e.value)
        assert "out of scope" in msg and "neural-net" in msg and "only" in msg and "-lamseed" in msg and "-ranker 9 (Linear Regression)" in msg
        assert "-netseed" not in msg and "-rnseed" not in msg
    for n in ("1", "7"):                                      # -lamseed opens nothing else
        with pytest.raises(RankLibError) as e:
            evaluator.main(["-train", str(data), "-ranker", n, "-lamseed", "3"])
        assert "out of scope" in str(e.value) and "-lamseed" not in str(e.value)
    f = RankerFactory()
    for seed in (None, 3):                                    # RankNet.seed, which LambdaRank inherits, opens nothing
        RankNet.seed = seed
        assert LambdaRank.seed == seed
        with pytest.raises(RankLibError) as e:
            f.createRanker(RankerType.LAMBDARANK)
        assert "LAMBDARANK" in str(e.value) and "out of scope" in str(e.value) and "LambdaRank.lamseed" in str(e.value)
        for call in (LambdaRank().init, LambdaRank().learn):
            with pytest.raises(RankLibError) as e:
                call()
            assert "out of scope" in str(e.value) and "LambdaRank.lamseed" in str(e.value) and "RankNet.seed" not in str(e.value)
    RankNet.seed = None
    LambdaRank.lamseed = 3
    assert type(f.createRanker(RankerType.LAMBDARANK)) is LambdaRank and type(f.createRanker("LAMBDARANK")) is LambdaRank
    assert RankNet.seed is None and LambdaRank.seed is None and "lamseed" not in RankNet.__dict__ and not hasattr(RankNet, "lamseed")
    for t in (RankerType.RANKNET, RankerType.LISTNET):
        with pytest.raises(RankLibError) as e:
            f.createRanker(t)
        assert "out of scope" in str(e.value)
    with pytest.raises(RankLibError) as e:                    # learn() before init()
        LambdaRank().learn()
    assert "out of scope" in str(e.value)


def test_the_train_metric_has_to_have_a_swap_change():
    LambdaRank.lamseed = 3
    dp = [DataPoint("1 qid:1 1:1 2:0"), DataPoint("0 qid:1 1:0 2:1")]
    for name in ("P@10", "RR@10"):
        r = RankerFactory().createRanker(RankerType.LAMBDARANK, [RankList(dp)], [1, 2], MetricScorerFactory().createScorer(name))
        with pytest.raises(RankLibError) as e:
            r.init()
        assert "LambdaRank train metric must be one of NDCG, DCG, MAP, ERR (got %s)" % name in str(e.value)


def test_cli_statics_are_set_for_the_run_and_restored(monkeypatch):
    seen = []
    real = evaluator.Evaluator.__init__

    def spy(self, rtype, *a, **k):
        seen.append((rtype,) + tuple(getattr(RankNet, s) for s in _STATICS) + (LambdaRank.lamseed, Neuron.learningRate))
        real(self, rtype, *a, **k)
    monkeypatch.setattr(evaluator.Evaluator, "__init__", spy)
    defaults = (100, 1, 10, 0.00005, None)
    Neuron.learningRate = 0.125
    with pytest.raises(RankLibError):                        # the reader throws on the missing file after the flags are parsed
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "5", "-lamseed", "3", "-rnseed", "8", "-epoch", "2", "-layer", "2", "-node", "4",
                        "-lr", "0.5"])
    assert seen == [(RankerType.LAMBDARANK, 2, 2, 4, 0.5, None, 3, 0.125)]      # RankNet's statics, shared; -rnseed reaches nothing
    assert tuple(getattr(RankNet, s) for s in _STATICS) == defaults and LambdaRank.lamseed is None and Neuron.learningRate == 0.125
    with pytest.raises(RankLibError):
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "5", "-lamseed", "-9", "-layer", "0"])
    assert seen[-1] == (RankerType.LAMBDARANK, 100, 0, 10, 0.00005, None, -9, 0.125)
    for n in ("6", "1", "7"):                                 # with another ranker -lamseed is parsed and reaches nothing
        with pytest.raises(RankLibError):
            evaluator.main(["-train", "no_such_file.txt", "-ranker", n, "-lamseed", "3", "-epoch", "9"])
    assert all(s[6] is None for s in seen[2:])
    assert tuple(getattr(RankNet, s) for s in _STATICS) == defaults and LambdaRank.lamseed is None


def test_the_usage_text_names_the_new_form(capsys):
    evaluator.main([])
    out = capsys.readouterr().out
    assert "-ranker 5 -lamseed n" in out and "is not trained" not in out and "-ranker 1 -rnseed n" in out


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_a_null_handle_is_refused_before_the_device_is_looked_at():
    """the null handle is the one error of rl_rn_set_lambdarank that needs no handle.  RL_ERR_STATE (after rl_rn_learn) and the P / RR
    refusal need one, and rl_rn_create looks at the device (RL_ERR_NO_DEVICE without a gfx950): they are in
    tests/test_gpu_lambdarank.py::test_refusals_on_a_handle"""
    L = N.lib()
    assert "rl_rn_set_lambdarank" in N.ABI_SYMBOLS
    assert L.rl_rn_set_lambdarank(None, 1) == -1 and L.rl_rn_set_lambdarank(None, 0) == -1      # RL_ERR_INVALID
    assert b"null handle" in L.rl_last_error()
