"""-m gpu: RL_FLAG_FAST_LEAF -- the leaves' sums as the fixed f64 reduction of DESIGN.md 14 -- against its numpy restatement
(tests/fast_leaf_restatement.py), bit for bit, from the two kernels alone up to the command line.

What the mode promises: the tree of a round is grown exactly as in the default mode (round 1 is the oracle's tree), every leaf output is the
restated arithmetic applied to the round's own lambda / weight and the leaf's members, the scores move by those outputs.  Later rounds are
self-consistent, not the oracle's: a leaf value that differs in its last bits feeds the next round's lambdas.
"""
import os

import numpy as np
import pytest

import fast_leaf_restatement as FL
import oracle_ffi as O
from linear_ext import write_letor
from ranklib_amd import _native as N
from ranklib_amd import evaluator, synth
from ranklib_amd.learning import FeatureHistogram, LambdaMART, RFRanker
from tree_equiv import node_members

pytestmark = pytest.mark.gpu

FAST = N.RL_FLAG_FAST_LEAF
LR = np.float64(np.float32(0.1))
SHAPE_A = (3000, 10, "ns", 0, 10, 8)          # n_docs, n_features, kind, seed, leaves, rounds
SHAPE_B = (2500, 5, "mslr", 4, 31, 4)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the two kernels alone -------------------------------------------------------------------------------------------------------
def test_sum_kernels_equal_the_restatement_on_every_level_edge():
    """tile edges (255 / 256 / 257, 511 / 512 / 513), a second level (up to 65 536 = 256 tiles -> 1), a third (65 537 -> 257 -> 2 -> 1; 200 001 -> 782 ->
    4 -> 1) and the empty segment, in ONE call: the segments share the tile-slot table"""
    lens = [0, 1, 2, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 200001, 0, 256]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg[-1])
    rng = np.random.default_rng(20240614)
    x = rng.standard_normal(n) * np.exp2(rng.integers(-40, 41, n).astype(np.float64))       # magnitudes 2^-40 .. 2^40, both signs
    z = rng.random(n) < 0.05
    x[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)                               # signed zeros
    x[seg[-2]:] = -0.0                                                                        # the last segment: a full tile of -0.0
    got64, got32 = N.debug_fast_sum(x, seg)
    want = np.array([FL.R(x[seg[i]:seg[i + 1]]) for i in range(len(lens))], np.float64)
    assert np.array_equal(_u64(got64), _u64(want)), [(lens[i], got64[i], want[i]) for i in range(len(lens)) if _u64(got64)[i] != _u64(want)[i]]
    assert np.array_equal(_u32(got32), _u32(want.astype(np.float32)))
    assert _u64(got64)[0] == 0 and _u64(got64)[-1] == 0 and _u64(got64)[-2] == 0             # empty and all -0.0 segments: +0.0
    # the order of the adds is visible in these values: the plain left-to-right sum is another number on the long segments
    assert any(got64[i] != FL.serial_f64(x[seg[i]:seg[i + 1]]) for i in (9, 10, 11))


def test_sum_kernels_known_answer_and_single_segment():
    x = np.concatenate([[2.0 ** 53], np.ones(256)])
    got64, got32 = N.debug_fast_sum(x)
    assert got64[0] == 2.0 ** 53 + 256 and got32[0] == np.float32(2.0 ** 53 + 256)          # tests/test_fast_leaf_cpu.py derives it by hand
    with pytest.raises(N.RankLibError):
        N.debug_fast_sum(np.ones(4), [0, 3, 2, 4])                                           # segments must ascend


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def _leaf_members(tr, X):
    mem = node_members(tr, X)
    return [(n, mem[n]) for n in range(len(tr["feature"])) if tr["feature"][n] == -1]


def _chain_output(lam, w, members, mart):
    """the default mode's value of the same leaf: the Java's float running sums (oracle/rl_oracle.c ro_float_chain)"""
    s1 = O.float_chain(lam, members)
    if mart:
        return np.float32(s1 / np.float32(len(members)))
    s2 = O.float_chain(w, members)
    return np.float32(0) if s2 == 0 else np.float32(s1 / s2)


def _run(shape, ranker, flags=FAST):
    n_docs, n_feat, kind, seed, leaves, rounds = shape
    X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind, seed_offset=seed)
    g = N.Trainer(n_trees=rounds, n_leaves=leaves, flags=flags, ranker=ranker)
    g.set_train(X, lab, qoff)
    g.init()
    rec = []
    prev = g.array("SCORE")
    for _ in range(rounds):
        t, tm, _, _ = g.boost_round()
        rec.append(dict(tree=t.trimmed(), lam=g.array("LAMBDA"), w=g.array("WEIGHT"), before=prev, after=g.array("SCORE"), metric=tm))
        prev = rec[-1]["after"]
    rec[0]["model_text"] = g.model_text()
    g.close()
    return X, lab, qoff, rec


_RUNS = {}


def _cached(shape, ranker):
    if (shape, ranker) not in _RUNS:
        _RUNS[(shape, ranker)] = _run(shape, ranker)
    return _RUNS[(shape, ranker)]


def _check_round(X, r, mart, ctx):
    """outputs == the restatement on the round's own lambda / weight and members; scores == previous + lr * output.  Returns per leaf
    (fast bits != chain bits, |fast - chain|)."""
    tr = r["tree"]
    want_scores = r["before"].copy()
    out = []
    for n, members in _leaf_members(tr, X):
        assert tr["count"][n] == len(members), (ctx, n)
        want = FL.leaf_output(r["lam"], r["w"], members, mart)
        assert _u32(tr["output"][n]) == _u32(want), (ctx, "leaf %d of %d samples: %r, restated %r" % (n, len(members), tr["output"][n], want))
        want_scores[members] += LR * np.float64(tr["output"][n])                 # LambdaMART.java:203-210, as tests/np_restatement.py round()
        chain = _chain_output(r["lam"], r["w"], members, mart)
        out.append((_u32(want) != _u32(chain), abs(float(want) - float(chain)), len(members)))
    assert np.array_equal(_u64(r["after"]), _u64(want_scores)), ctx
    return out


def test_round_one_is_the_oracles_tree_with_the_new_leaves():
    X, lab, qoff, rec = _cached(SHAPE_A, "LAMBDAMART")
    o = O.Oracle(X, lab, qoff, n_trees=1, n_leaves=SHAPE_A[4])
    o.init()
    to, _, _, _ = o.round()
    a, b = to.trimmed(), rec[0]["tree"]
    assert np.array_equal(a["feature"], b["feature"]) and np.array_equal(_u32(a["threshold"]), _u32(b["threshold"]))
    assert np.array_equal(a["left"], b["left"]) and np.array_equal(a["right"], b["right"]) and np.array_equal(a["count"], b["count"])
    assert np.array_equal(_u64(rec[0]["lam"]), _u64(o.lambdas())) and np.array_equal(_u64(rec[0]["w"]), _u64(o.weights()))
    _check_round(X, rec[0], False, "round 1")
    assert np.array_equal(a["output"] == 0, b["output"] == 0)


@pytest.mark.parametrize("ranker", ["LAMBDAMART", "MART"])
@pytest.mark.parametrize("shape", [SHAPE_A, SHAPE_B], ids=["3000x10_ns", "2500x5_mslr"])
def test_later_rounds_are_self_consistent_and_within_1e5_of_the_float_chain(shape, ranker):
    """BASELINE.md's bound on leaf values, 1e-5, against the default mode's value of the same leaf (same lambda, weight, members): the definition
    alone stays inside it on these leaves (the largest holds 1 619 samples; the deviation grows with the leaf, so no such bound is
    asserted on larger ones).  At least one leaf differs in its bits: the mode is on."""
    X, lab, qoff, rec = _cached(shape, ranker)
    per_leaf = []
    for i, r in enumerate(rec):
        per_leaf += _check_round(X, r, ranker == "MART", "%s round %d" % (ranker, i + 1))
    differ = sum(1 for d, _, _ in per_leaf if d)
    worst = max(e for _, e, _ in per_leaf)
    print("\n[fast leaf] %s %s: %d of %d leaves differ in bits from the float chain, max |deviation| %.3g, largest leaf %d"
          % (shape[:3], ranker, differ, len(per_leaf), worst, max(c for _, _, c in per_leaf)))
    assert differ >= 1
    assert worst <= 1e-5


def test_a_three_level_leaf_inside_the_trainer():
    """70 000 documents, min_leaf_support 40 000: no split is admissible, the tree is its root, the sample list the identity; 274 tiles -> 2 -> 1"""
    X, lab, qoff = synth.make_dataset(70000, 4, "ns")
    g = N.Trainer(n_trees=2, n_leaves=10, min_leaf_support=40000, flags=FAST)
    g.set_train(X, lab, qoff)
    g.init()
    for r in range(2):
        before = g.array("SCORE")
        t, _, _, _ = g.boost_round()
        tr = t.trimmed()
        assert t.n_nodes == 1 and tr["feature"][0] == -1 and tr["count"][0] == 70000
        lam, w = g.array("LAMBDA"), g.array("WEIGHT")
        assert len(FL.level(lam)) == 274 and len(FL.level(FL.level(lam))) == 2
        want = FL.leaf_output(lam, w, np.arange(70000))
        assert _u32(tr["output"][0]) == _u32(want), (r, tr["output"][0], want)
        assert np.array_equal(_u64(g.array("SCORE")), _u64(before + LR * np.float64(want))), r
    g.close()


def _eval_tree_rows(tr, X):
    out = np.zeros(X.shape[0], np.float64)
    for i in range(X.shape[0]):
        n = 0
        while tr["feature"][n] != -1:
            n = tr["left"][n] if X[i, tr["feature"][n] - 1] <= tr["threshold"][n] else tr["right"][n]
        out[i] = tr["output"][n]
    return out


def test_validation_early_stop_rollback_and_finish():
    X, lab, qoff = synth.make_dataset(4000, 12, "ns", seed_offset=5)
    Xv, labv, qoffv = synth.make_dataset(1500, 12, "ns", seed_offset=6)
    g = N.Trainer(n_trees=40, n_leaves=5, early_stop_rounds=3, flags=FAST)
    g.set_train(X, lab, qoff)
    g.set_validation(Xv, labv, qoffv)
    g.init()
    vs = np.zeros(len(labv))
    record, best, best_round = [], 0.0, None
    for r in range(40):
        t, tm, vm, stop = g.boost_round()
        vs += LR * _eval_tree_rows(t.trimmed(), Xv)                                   # LambdaMART.java:230-234 with the tree's fast-mode outputs
        assert np.array_equal(_u64(g.array("VALID_SCORE")), _u64(vs)), r
        record.append(vm)
        if float(vm) > best:
            best, best_round = float(vm), r
        assert stop == (r - best_round > 3), r
        if stop:
            break
    assert g.best_validation() == (best_round, float(record[best_round]))
    ts, vscore = g.finish()
    assert g.num_trees() == best_round + 1 and len(record) > best_round + 3
    assert g.round_metrics(best_round)[1] == record[best_round]
    assert 0.0 < ts <= 1.0 and 0.0 < vscore <= 1.0 and g.best_validation()[1] == vscore
    text = g.model_text()
    assert text.count("<tree id=") == best_round + 1
    m = N.Model(text)                                                               # the ordinary ensemble text: loads and scores like any other
    assert np.array_equal(_u32(m.predict_rows(np.hstack([np.zeros((50, 1), np.float32), Xv[:50]]))), _u32(g.predict(Xv[:50])))
    g.close()


def test_refusals():
    for other in (N.RL_FLAG_JAVA_ORDER, N.RL_FLAG_SERIAL_CHAIN):
        with pytest.raises(N.RankLibError) as e:
            N.Trainer(n_trees=1, flags=FAST | other)
        assert "(rlhip status -1)" in str(e.value) and "RL_FLAG_FAST_LEAF" in str(e.value)
    X, lab, qoff = synth.make_dataset(600, 4, "ns")
    g = N.Trainer(n_trees=1, flags=FAST)
    g.set_train(X, lab, qoff)
    with pytest.raises(N.RankLibError) as e:                                        # the one-rank host transport, as tests/test_gpu_dist.py
        g.dist_init_callback(0, 1, lambda arr, op: None, lambda src: src.copy())
    assert "(rlhip status -4)" in str(e.value) and "rank-count-invariant" in str(e.value)
    g.init()                                                                        # the refusal left the trainer an ordinary one-GPU trainer
    g.boost_round()
    g.close()
    g = N.Trainer(n_trees=1, flags=FAST | N.RL_FLAG_FIRST_TIE)                      # the speed-first pair
    g.set_train(X, lab, qoff)
    g.init()
    t, _, _, _ = g.boost_round()
    lam, w = g.array("LAMBDA"), g.array("WEIGHT")
    for n, members in _leaf_members(t.trimmed(), X):
        assert _u32(t.trimmed()["output"][n]) == _u32(FL.leaf_output(lam, w, members))
    g.close()


def test_command_line(tmp_path, monkeypatch):
    for cls, names in ((LambdaMART, ("nTrees", "nTreeLeaves", "learningRate", "nThreshold", "minLeafSupport", "nRoundToStopEarly", "fastLeaf")),
                       (RFRanker, ("nTrees", "nTreeLeaves", "nBag", "learningRate", "minLeafSupport")), (FeatureHistogram, ("samplingRate", "seed"))):
        for nm in names:
            monkeypatch.setattr(cls, nm, getattr(cls, nm))                          # restored when the test ends (RFRanker.init never restores them)
    X, lab, qoff, rec = _cached(SHAPE_A, "LAMBDAMART")
    data = str(tmp_path / "train.txt")
    write_letor(data, X, lab, qoff)
    common = ["-train", data, "-metric2t", "NDCG@10", "-tree", "8", "-leaf", "10"]
    m_fast, m_def, m_mart, m_rf = (str(tmp_path / n) for n in ("fast.txt", "default.txt", "mart.txt", "rf.txt"))
    assert evaluator.main(common + ["-ranker", "6", "-fastleaf", "-save", m_fast]) == 0
    assert evaluator.main(["-load", m_fast, "-test", data, "-metric2T", "NDCG@10"]) == 0
    assert evaluator.main(common + ["-ranker", "6", "-save", m_def]) == 0
    fast, default = open(m_fast).read(), open(m_def).read()
    assert fast.startswith("## LambdaMART") and fast.count("<tree id=") == 8
    assert fast != default                                                          # the data of SHAPE_A: leaves differ in their bits from round 1 on
    assert fast == rec[0]["model_text"]                                             # the command line trained what the trainer gives with the flag
    assert evaluator.main(common + ["-ranker", "0", "-fastleaf", "-save", m_mart]) == 0
    assert open(m_mart).read() == _cached(SHAPE_A, "MART")[3][0]["model_text"]
    assert evaluator.main(["-train", data, "-metric2t", "NDCG@10", "-ranker", "8", "-bag", "2", "-tree", "2", "-leaf", "10", "-fastleaf", "-save", m_rf]) == 0
    assert LambdaMART.fastLeaf is True
    assert evaluator.main(["-load", m_rf, "-test", data, "-metric2T", "NDCG@10"]) == 0
    assert LambdaMART.fastLeaf is False and open(m_rf).read().startswith("## Random Forests")
    assert os.path.getsize(m_rf) > 0
