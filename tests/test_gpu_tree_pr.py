"""-m gpu: LambdaMART, MART and Random Forests trained on P@k and RR@k against the literal restatement (tests/np_restatement.LambdaMART with the
scorers of tests/pr_restatement.py), bit patterns and no tolerances: the lambdas and weights of every round, every tree (features, thresholds,
outputs, counts), the float train and validation metric of every round, the finish() scores.

One synthetic set serves every case: list lengths on both sides of every length class of the lambda kernels (16 | 64 | 128 | 192 | 256), of every k
the cases use, one list of 600 documents (three tiles, two sweeps), labels 0 .. 4 with one in ten set to 0.5 (relevant as label > 0.0, non-relevant
as (int) label == 0: ReciprocalRankScorer.java:75,85), every fourth list with few relevant documents (RR without a firstRank or a secondRank).  The restatement's rounds are computed once per (ranker, metric, k) and shared.

The same rounds are compared under every mode of the trainer that touches these metrics: the ranking and stream knobs (RLHIP_RANK_SPLIT,
RLHIP_TINY_MIN, RLHIP_LAMBDA_SIDE, RLHIP_LAMBDA_COMPACT, RLHIP_LAMBDA_UNFUSED), RL_FLAG_JAVA_ORDER, RL_FLAG_FIRST_TIE, RL_FLAG_FAST_LEAF, MART, two
and three shards.  tests/test_gpu_tree_pr_branches.py reuses the comparison on data that reaches the swap changes' cases one by one.

No case may pass vacuously: in every compared round the restatement gives a non-zero lambda to at least a quarter of the documents and every tree
has a split (asserted where the restatement's rounds are recorded)."""
import functools
import logging

import numpy as np
import pytest

import np_restatement as R
import pr_cases
import test_gpu_dist as TD
import test_gpu_fast_leaf as TF
from pr_restatement import P, RR
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd.learning import FeatureHistogram, LambdaMART, RankerFactory, RFRanker, Sampler
from tree_equiv import assert_equivalent

pytestmark = pytest.mark.gpu

ARM = N.ARM
ROUNDS, LEAVES = 4, 6
SCORERS = {"P": P, "RR": RR}
_KS = (1, 3, 5, 10, 16, 20)                                              # every k of the cases below: lists of k - 1, k, k + 1 documents


def bits(a, kind):
    return np.ascontiguousarray(a).view(kind)


def _labels(rng, x0):
    """half of the documents 0, the others 1 .. 4 by the (noisy) first feature; one in ten 0.5"""
    s = x0 + rng.normal(0.0, 0.35, len(x0))
    cut = np.quantile(s, [0.5, 0.7, 0.85, 0.95])
    lab = np.searchsorted(cut, s).astype(np.float32)
    lab[rng.random(len(x0)) < 0.10] = 0.5
    return lab


def _make(rng, lengths, reverse_labels=False):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(qoff[-1])
    X = (rng.integers(0, 8, (n, 5)) / 8.0).astype(np.float32)           # few distinct values per column
    lab = _labels(rng, X[:, 0])
    for q in range(0, len(lengths), 4):                                  # every fourth list has few relevant documents: none, or one, among the top k of RR
        a, b = int(qoff[q]), int(qoff[q + 1])
        lab[a:b][rng.random(b - a) < 0.85] = 0.0
    if reverse_labels:                                                   # labels unrelated to the features: the validation metric wanders, the early stop fires
        lab = lab[::-1].copy()
    return X, lab, qoff


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(20)
    special = sorted({1, 2, 16, 17, 64, 65, 128, 129, 192, 193, 256, 257, 600} | {k + d for k in _KS for d in (-1, 0, 1) if k + d > 0})
    fill = []
    while sum(special) + sum(fill) < 4000:
        fill.append(int(rng.integers(3, 41)))
    lengths = np.array(special + fill)
    rng.shuffle(lengths)
    train = _make(rng, lengths)
    vl = []
    while sum(vl) < 500:
        vl.append(int(rng.integers(3, 41)))
    valid = _make(rng, np.array(vl))
    valid_mart = _make(rng, np.array(vl), reverse_labels=True)        # MART's cases: the early stop has to fire
    for a in train + valid + valid_mart:
        a.setflags(write=False)
    return train, valid, valid_mart


def flat(root):
    """pre-order (feature, threshold, output, count) of a restatement tree: the layout of FlatTree"""
    feat, thr, out, cnt = [], [], [], []

    def rec(n):
        feat.append(n.feature_id); thr.append(np.float32(n.threshold)); out.append(np.float32(n.output)); cnt.append(n.n)
        if n.feature_id != -1:
            rec(n.left); rec(n.right)
    rec(root)
    return np.array(feat, np.int32), np.array(thr, np.float32), np.array(out, np.float32), np.array(cnt, np.int64)


def _restatement(ranker, metric, k, rounds, leaves, early_stop, train, valid, cases=None):
    """cases: names of tests/pr_cases.py that the lists, in the ranked order every round makes its lambdas in, have to reach"""
    X, lab, qoff = train
    m = R.LambdaMART(X, lab, qoff, n_trees=rounds, n_leaves=leaves, k=k, early_stop=early_stop, metric="NDCG", ranker=ranker)
    m.scorer = SCORERS[metric](k)
    if valid is not None:
        m.set_validation(*valid)
    m.init()
    recs = []
    for r in range(rounds):
        if cases is not None:
            got = pr_cases.reached(metric, k, lab, qoff, m.model_scores)
            assert got >= cases, (metric, k, r, sorted(cases - got))
        root, tm, vm, stop = m.round()
        lam, w = np.array(m.pseudo, np.float64), np.array(m.weights, np.float64)
        # not vacuous: a quarter of the documents carry a lambda, the tree has a split
        assert np.count_nonzero(lam) >= len(lam) / 4, (ranker, metric, k, r, np.count_nonzero(lam), len(lam))
        assert root.feature_id != -1, (ranker, metric, k, r)
        recs.append(dict(root=root, tree=flat(root), lam=lam, w=w, tm=np.float32(tm), vm=None if vm is None else np.float32(vm), stop=bool(stop),
                         score=np.array(m.model_scores, np.float64)))
        if stop:
            break
    fin = m.finish()
    vfin = None
    if valid is not None:                                                # LambdaMART.java:260-264: the scorer on the ranked validation lists, a double mean
        Xv, lv, qv = valid
        sv = [float(v) for v in m.predict(Xv)]
        tot = 0.0
        for q in range(len(qv) - 1):
            a, b = int(qv[q]), int(qv[q + 1])
            tot += m.scorer.score([float(lv[a + i]) for i in R.stable_desc(sv[a:b])], "v%d" % q)
        vfin = tot / (len(qv) - 1)
    return dict(rounds=recs, fin=fin, vfin=vfin, kept=len(m.ensemble), model=m)


@functools.lru_cache(maxsize=None)
def reference(ranker, metric, k):
    train, valid, valid_mart = data()
    if ranker == "MART":
        return _restatement(ranker, metric, k, 10, LEAVES, 1, train, valid_mart)
    return _restatement(ranker, metric, k, ROUNDS, LEAVES, 100, train, valid)


def compare(g, ref, ctx0):
    """an initialised trainer against recorded rounds of the restatement, round by round; returns the launch arms and closes the trainer"""
    for r, want in enumerate(ref["rounds"]):
        tg, tm, vm, stop = g.boost_round()
        ctx = ctx0 + (r,)
        assert np.array_equal(bits(g.array("LAMBDA"), np.int64), bits(want["lam"], np.int64)), ctx
        assert np.array_equal(bits(g.array("WEIGHT"), np.int64), bits(want["w"], np.int64)), ctx
        t = tg.trimmed()
        feat, thr, out, cnt = want["tree"]
        assert np.array_equal(t["feature"], feat), ctx
        assert np.array_equal(bits(t["threshold"], np.uint32), bits(thr, np.uint32)), ctx
        assert np.array_equal(bits(t["output"], np.uint32), bits(out, np.uint32)), ctx
        assert np.array_equal(np.asarray(t["count"], np.int64), cnt), ctx
        assert np.array_equal(bits(g.array("SCORE"), np.int64), bits(want["score"], np.int64)), ctx
        assert bits(np.float32(tm), np.uint32) == bits(want["tm"], np.uint32), (ctx, tm, want["tm"])
        assert (vm is None) == (want["vm"] is None), ctx
        if vm is not None:
            assert bits(np.float32(vm), np.uint32) == bits(want["vm"], np.uint32), (ctx, vm, want["vm"])
        assert stop == want["stop"], ctx
    ts, vs = g.finish()
    assert ts == ref["fin"] and vs == ref["vfin"], (ctx0, ts, ref["fin"], vs, ref["vfin"])
    assert g.num_trees() == ref["kept"]
    arms = g.array("LAUNCH_ARMS")
    g.close()
    return arms


def run_gpu(ranker, metric, k, monkeypatch, env=None, flags=0):
    """the GPU trainer against reference(ranker, metric, k), round by round; returns the launch arms"""
    for name, v in (env or {}).items():
        monkeypatch.setenv("RLHIP_" + name, str(v))
    ref = reference(ranker, metric, k)
    mart = ranker == "MART"
    (X, lab, qoff), valid = data()[0], data()[2 if mart else 1]
    g = N.Trainer(n_trees=10 if mart else ROUNDS, n_leaves=LEAVES, metric=metric, metric_k=k, ranker=ranker, early_stop_rounds=1 if mart else 100, flags=flags)
    g.set_train(X, lab, qoff)
    g.set_validation(*valid)
    g.init()
    return compare(g, ref, (ranker, metric, k, env, flags))


def _fused_only(arms, rounds=ROUNDS):
    """the LDS-resident kernel ran, under no RL_ARM_LAM_* arm of another mode (the arm table has no slot for P / RR: DESIGN.md 21)"""
    for a in ("LAM_UNFUSED", "LAM_FUSED", "LAM_COMPACT", "LAM_ERR", "LAM_MAP", "LAM_TINY", "LAM_MART"):
        assert arms[ARM[a]] == 0, (a, arms[ARM[a]])
    assert arms[ARM["LAM_ON_MAIN"]] + arms[ARM["LAM_ON_SIDE"]] >= rounds


# ---- LambdaMART, one GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["P", "RR"])
@pytest.mark.parametrize("k", [1, 3, 10, 16, 17, 20])
def test_lambdamart_equals_the_restatement(metric, k, monkeypatch):
    arms = run_gpu("LAMBDAMART", metric, k, monkeypatch)
    if k <= 16:
        _fused_only(arms)
        assert arms[ARM["RANK_TINY"]] == 0                               # (the few lists of at most 16 documents join the 64-wide class)
    else:                                                                # beyond kLambdaFusedMaxK: the pair-term matrix
        assert arms[ARM["LAM_UNFUSED"]] == ROUNDS and arms[ARM["LAM_ON_MAIN"]] + arms[ARM["LAM_ON_SIDE"]] == 0


@pytest.mark.parametrize("metric", ["P", "RR"])
def test_unfused_knob(metric, monkeypatch):
    arms = run_gpu("LAMBDAMART", metric, 10, monkeypatch, {"LAMBDA_UNFUSED": 1})
    assert arms[ARM["LAM_UNFUSED"]] == ROUNDS and arms[ARM["LAM_ON_MAIN"]] + arms[ARM["LAM_ON_SIDE"]] == 0


@pytest.mark.parametrize("metric", ["P", "RR"])
def test_tiny_lists_in_their_own_launches(metric, monkeypatch):
    """RLHIP_TINY_MIN=1: the lists of at most 16 documents are ranked by k_rank_tiny and take k_lambda_fused<64, .> as a class of their own
    (k_lambda_tiny is NDCG / DCG only)"""
    arms = run_gpu("LAMBDAMART", metric, 10, monkeypatch, {"TINY_MIN": 1})
    _fused_only(arms)
    assert arms[ARM["RANK_TINY"]] > 0
    assert arms[ARM["LAM_ON_MAIN"]] + arms[ARM["LAM_ON_SIDE"]] == 5 * ROUNDS       # five length classes hold lists


# ---- modes of the trainer: other rank kernels, other streams, the flags -------------------------------------------------------------------------
def _rank_arms(arms):
    return {a: int(arms[ARM[a]]) for a in ("RANK_TINY", "RANK_MIXED", "RANK_WAVE_LONG", "RANK_WAVE_SHORT", "RANK_BLOCK", "RANK_HUGE") if arms[ARM[a]]}


# data(): lists in four length classes (64 | 128 | 192 | 256 wide), five with the lists of at most 16 documents apart; none beyond 5 000 documents
MODES = [
    ("RANK_SPLIT", {"RANK_SPLIT": 1}, lambda a: set(_rank_arms(a)) == {"RANK_WAVE_SHORT", "RANK_BLOCK"}),
    ("RANK_SPLIT,TINY_MIN=1", {"RANK_SPLIT": 1, "TINY_MIN": 1},
     lambda a: (set(_rank_arms(a)) == {"RANK_TINY", "RANK_WAVE_SHORT", "RANK_BLOCK"}
                and a[ARM["LAM_ON_SIDE"]] == ROUNDS and a[ARM["LAM_ON_MAIN"]] == 4 * ROUNDS)),
    ("LAMBDA_SIDE=0", {"LAMBDA_SIDE": 0}, lambda a: a[ARM["LAM_ON_SIDE"]] == 0 and a[ARM["LAM_ON_MAIN"]] == 4 * ROUNDS),
    ("LAMBDA_SIDE=1", {}, lambda a: a[ARM["LAM_ON_SIDE"]] == ROUNDS and a[ARM["LAM_ON_MAIN"]] == 3 * ROUNDS and "RANK_MIXED" in _rank_arms(a)),
    ("LAMBDA_SIDE=2", {"LAMBDA_SIDE": 2}, lambda a: a[ARM["LAM_ON_SIDE"]] == 2 * ROUNDS and a[ARM["LAM_ON_MAIN"]] == 2 * ROUNDS),
    ("LAMBDA_SIDE=3", {"LAMBDA_SIDE": 3}, lambda a: a[ARM["LAM_ON_SIDE"]] == 3 * ROUNDS and a[ARM["LAM_ON_MAIN"]] == ROUNDS),
    ("LAMBDA_COMPACT", {"LAMBDA_COMPACT": 1}, lambda a: a[ARM["LAM_ON_SIDE"]] == ROUNDS and a[ARM["LAM_ON_MAIN"]] == 3 * ROUNDS),      # NDCG's and DCG's: nothing may change
]


@pytest.mark.parametrize("metric", ["P", "RR"])
@pytest.mark.parametrize("name,env,check", MODES, ids=[m[0] for m in MODES])
def test_ranking_and_stream_knobs_keep_every_bit(name, env, check, metric, monkeypatch):
    arms = run_gpu("LAMBDAMART", metric, 10, monkeypatch, env)
    _fused_only(arms)                                                    # (LAM_COMPACT == 0 among them)
    assert check(arms), (name, _rank_arms(arms), int(arms[ARM["LAM_ON_SIDE"]]), int(arms[ARM["LAM_ON_MAIN"]]))


def test_rank_split_writes_first_and_second_for_the_pair_term_matrix(monkeypatch):
    """RR@20 is unfused: swap_change_abs reads firstRank / secondRank from the table k_rank_wave and k_rank_block wrote"""
    arms = run_gpu("LAMBDAMART", "RR", 20, monkeypatch, {"RANK_SPLIT": 1})
    assert arms[ARM["LAM_UNFUSED"]] == ROUNDS and arms[ARM["LAM_ON_MAIN"]] + arms[ARM["LAM_ON_SIDE"]] == 0
    assert set(_rank_arms(arms)) == {"RANK_WAVE_SHORT", "RANK_BLOCK"}


@pytest.mark.parametrize("metric", ["P", "RR"])
def test_java_order_flag(metric, monkeypatch):
    """RL_FLAG_JAVA_ORDER, the strict mode: split gains from the f64 histogram RankLib itself would hold; everything as in the default mode"""
    _fused_only(run_gpu("LAMBDAMART", metric, 10, monkeypatch, flags=N.RL_FLAG_JAVA_ORDER))


class _RefTree:
    """a restatement tree with the interface tree_equiv.assert_equivalent reads"""
    def __init__(self, root):
        feat, thr, out, cnt = flat(root)
        left, right = np.full(len(feat), -1, np.int32), np.full(len(feat), -1, np.int32)
        stack = []                                                       # pre-order: the left child follows its parent, the right one the left subtree
        for i in range(len(feat)):
            if stack:
                p = stack.pop()
                (left if left[p] == -1 else right)[p] = i
                if right[p] == -1:
                    stack.append(p)
            if feat[i] != -1:
                stack.append(i)
        self.n_nodes = len(feat)
        self._t = dict(feature=feat, threshold=thr, left=left, right=right, output=out, count=cnt)

    def trimmed(self):
        return self._t


def _trainer(metric, k, flags, valid=True):
    (X, lab, qoff), v = data()[0], data()[1]
    g = N.Trainer(n_trees=ROUNDS, n_leaves=LEAVES, metric=metric, metric_k=k, ranker="LAMBDAMART", early_stop_rounds=100, flags=flags)
    g.set_train(X, lab, qoff)
    if valid:
        g.set_validation(*v)
    g.init()
    return g


@pytest.mark.parametrize("metric", ["P", "RR"])
def test_first_tie_flag(metric):
    """RL_FLAG_FIRST_TIE: no tie is resolved the Java's way, so a stored (feature, threshold) may be another member of a tie; every tree is the
    reference's function and partition on the training set (tests/tree_equiv.py) and the lambdas, weights, scores and train metric of every
    round keep their bits.  Without a validation set: the other member of a tie may send a validation row the other way."""
    ref = reference("LAMBDAMART", metric, 10)
    X = data()[0][0]
    g = _trainer(metric, 10, N.RL_FLAG_FIRST_TIE, valid=False)
    for r, want in enumerate(ref["rounds"]):
        tg, tm, _, stop = g.boost_round()
        ctx = (metric, r)
        assert np.array_equal(bits(g.array("LAMBDA"), np.int64), bits(want["lam"], np.int64)), ctx
        assert np.array_equal(bits(g.array("WEIGHT"), np.int64), bits(want["w"], np.int64)), ctx
        assert_equivalent(_RefTree(want["root"]), tg, X, ctx)
        assert np.array_equal(bits(g.array("SCORE"), np.int64), bits(want["score"], np.int64)), ctx
        assert bits(np.float32(tm), np.uint32) == bits(want["tm"], np.uint32), (ctx, tm, want["tm"])
        assert not stop
    assert g.array("TIE_STATS")[0] == 0                                  # no resolution ran
    g.close()


@pytest.mark.parametrize("metric", ["P", "RR"])
def test_fast_leaf_flag(metric):
    """RL_FLAG_FAST_LEAF: round 1 has the reference's lambdas, weights and tree with leaf outputs within 1e-5 of the reference's (the mode's stated
    bound); every round is self-consistent as tests/test_gpu_fast_leaf.py has it (outputs are the restated f64 reduction of the
    round's own lambdas and weights over the leaf's members, the scores move by them)"""
    want = reference("LAMBDAMART", metric, 10)["rounds"][0]
    X = data()[0][0]
    g = _trainer(metric, 10, N.RL_FLAG_FAST_LEAF, valid=False)
    prev = g.array("SCORE")
    for r in range(ROUNDS):
        tg, _, _, _ = g.boost_round()
        rec = dict(tree=tg.trimmed(), lam=g.array("LAMBDA"), w=g.array("WEIGHT"), before=prev, after=g.array("SCORE"))
        prev = rec["after"]
        if r == 0:
            feat, thr, out, cnt = want["tree"]
            assert np.array_equal(bits(rec["lam"], np.int64), bits(want["lam"], np.int64))
            assert np.array_equal(bits(rec["w"], np.int64), bits(want["w"], np.int64))
            assert np.array_equal(rec["tree"]["feature"], feat) and np.array_equal(bits(rec["tree"]["threshold"], np.uint32), bits(thr, np.uint32))
            assert np.array_equal(np.asarray(rec["tree"]["count"], np.int64), cnt)
            assert np.max(np.abs(rec["tree"]["output"].astype(np.float64) - out.astype(np.float64))) <= 1e-5
        assert np.count_nonzero(rec["lam"]) >= len(rec["lam"]) / 4 and rec["tree"]["feature"][0] != -1, (metric, r)
        TF._check_round(X, rec, False, "%s round %d" % (metric, r + 1))
    g.close()


# ---- MART: the scorer only reports ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["P", "RR"])
def test_mart_with_validation_and_early_stop(metric, monkeypatch):
    ref = reference("MART", metric, 5)
    assert ref["rounds"][-1]["stop"] and len(ref["rounds"]) < 10 and ref["kept"] < len(ref["rounds"]), "the early stop did not fire"
    arms = run_gpu("MART", metric, 5, monkeypatch)
    assert arms[ARM["LAM_MART"]] == len(ref["rounds"]) and arms[ARM["LAM_UNFUSED"]] == 0


# ---- sharded: two ranks as processes on one GPU -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["P", "RR"])
def test_two_shards_equal_one(metric, tmp_path):
    TD.k_shards_against_one_shard(2, "LAMBDAMART", metric, 5, (6000, 16, "mslr", 5, 10, 3), tmp_path)


@pytest.mark.parametrize("world,ranker,metric", [(2, "MART", "P"), (3, "LAMBDAMART", "RR")])
def test_mart_sharded_and_three_shards(world, ranker, metric, tmp_path):
    TD.k_shards_against_one_shard(world, ranker, metric, 5, (6000, 16, "mslr", 5, 10, 3), tmp_path)


# ---- command line -------------------------------------------------------------------------------------------------------------------------------
def _write(path, X, lab, qoff, qid0=0):
    """a LETOR file that keeps fractional labels"""
    with open(path, "w") as f:
        for q in range(len(qoff) - 1):
            for i in range(int(qoff[q]), int(qoff[q + 1])):
                f.write("%r qid:%d %s\n" % (float(lab[i]), qid0 + q, " ".join("%d:%r" % (j + 1, float(X[i, j])) for j in range(X.shape[1]))))


@functools.lru_cache(maxsize=None)
def cli_data():
    rng = np.random.default_rng(21)
    train = _make(rng, np.array([int(rng.integers(2, 25)) for _ in range(40)]))
    valid = _make(rng, np.array([int(rng.integers(2, 25)) for _ in range(15)]))
    return train, valid


def _keep_statics(monkeypatch):
    for cls, names in ((LambdaMART, ("nTrees", "nTreeLeaves", "learningRate", "nThreshold", "minLeafSupport", "nRoundToStopEarly")),
                       (RFRanker, ("nTrees", "nTreeLeaves", "nBag", "learningRate", "minLeafSupport", "nThreshold", "subSamplingRate", "featureSamplingRate", "rType", "seed")),
                       (FeatureHistogram, ("samplingRate", "seed"))):
        for nm in names:
            monkeypatch.setattr(cls, nm, getattr(cls, nm))                # restored when the test ends


def _rows(X):
    rows = np.zeros((X.shape[0], X.shape[1] + 1), np.float32)            # column = feature id
    rows[:, 1:] = X
    return rows


@pytest.mark.parametrize("ranker,flag,metric", [("LAMBDAMART", "6", "P"), ("MART", "0", "RR")])
def test_command_line_trains_saves_and_loads(ranker, flag, metric, tmp_path, caplog, monkeypatch):
    _keep_statics(monkeypatch)
    train, valid = cli_data()
    f, v, m = (str(tmp_path / n) for n in ("train.txt", "valid.txt", "model.txt"))
    _write(f, *train)
    _write(v, *valid, qid0=1000)
    name = "%s@5" % metric
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        assert evaluator.main(["-train", f, "-validate", v, "-ranker", flag, "-metric2t", name, "-tree", "3", "-leaf", "4", "-estop", "100", "-save", m]) == 0
    log = "\n".join(rec.getMessage() for rec in caplog.records)
    assert name + "-T" in log and name + "-V" in log
    ref = _restatement(ranker, metric, 5, 3, 4, 100, train, valid)
    assert all(np.count_nonzero(r["lam"]) for r in ref["rounds"])
    loaded = RankerFactory().loadRankerFromFile(m)
    assert loaded._model.num_trees() == ref["kept"]
    got = loaded._model.predict_rows(_rows(train[0]))
    assert np.array_equal(bits(np.float32(got), np.uint32), bits(ref["model"].predict(train[0]), np.uint32))


def test_command_line_random_forests_on_p(tmp_path, monkeypatch):
    """every bag is a LambdaMART run on the bag's sample (Sampler under -seed, with replacement); -frate 1.0: every feature at every split"""
    _keep_statics(monkeypatch)
    (X, lab, qoff), _ = cli_data()
    f, m = str(tmp_path / "train.txt"), str(tmp_path / "rf.txt")
    _write(f, X, lab, qoff)
    assert evaluator.main(["-train", f, "-ranker", "8", "-rtype", "6", "-bag", "2", "-frate", "1.0", "-seed", "3", "-metric2t", "P@5", "-tree", "2", "-leaf", "4",
                           "-save", m]) == 0
    loaded = RankerFactory().loadRankerFromFile(m)
    assert len(loaded._models) == 2
    nq = len(qoff) - 1
    for b in range(2):
        picks = Sampler(RFRanker.bag_seed(3, b)).doSampling(list(range(nq)), 1.0, True)
        idx = np.concatenate([np.arange(qoff[q], qoff[q + 1]) for q in picks])
        bag = (X[idx], lab[idx], np.concatenate([[0], np.cumsum([qoff[q + 1] - qoff[q] for q in picks])]).astype(np.int32))
        ref = _restatement("LAMBDAMART", "P", 5, 2, 4, 100, bag, None)
        got = loaded._models[b].predict_rows(_rows(X))
        assert np.array_equal(bits(np.float32(got), np.uint32), bits(ref["model"].predict(X), np.uint32)), b


def test_command_line_refusals_that_remain(tmp_path, monkeypatch):
    _keep_statics(monkeypatch)
    (X, lab, qoff), _ = cli_data()
    f = str(tmp_path / "train.txt")
    _write(f, X, lab, qoff)
    with pytest.raises(N.RankLibError) as e:                             # plain RR: k = 0 scores 0 everywhere
        evaluator.main(["-train", f, "-ranker", "6", "-metric2t", "RR", "-tree", "2", "-leaf", "4"])
    assert "metric k out of range" in str(e.value)
    with pytest.raises(N.RankLibError) as e:
        evaluator.main(["-train", f, "-ranker", "6", "-metric2t", "Best@3", "-tree", "2", "-leaf", "4"])
    assert "train metric must be one of NDCG, DCG, MAP, ERR, P, RR (got Best@3)" in str(e.value)
    for metric in ("P", "RR"):                                           # the library's own refusal of k < 1
        with pytest.raises(N.RankLibError) as e:
            N.Trainer(n_trees=1, metric=metric, metric_k=0)
        assert "metric k out of range" in str(e.value)
