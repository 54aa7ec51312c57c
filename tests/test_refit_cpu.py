"""Refit without a device: the NumPy restatement of a refit (tests/refit_restatement.py) against a table worked out by hand and
against the CPU oracles -- the premise of the identity: the documents of a grown leaf, taken in ascending document index, are the leaf's samples
in the order the trainer summed them, so a refit of a model on the data and parameters it was trained with gives the model back bit for bit --
then the command line's refusals, the log of a refit run through a stub trainer, the statics' reset and the exported symbols.

The C oracle (oracle/rl_oracle.c) trains on NDCG, DCG, MAP and ERR and as MART; for P@k and RR@k the oracle is the Python transcription
np_restatement.LambdaMART with the scorers of tests/pr_restatement.py, as in the tests of those two metrics.
"""
import ctypes as C
import logging
import math
import os
import re

import numpy as np
import pytest

import np_restatement as R
import oracle_ffi as O
import pr_restatement as PR
import refit_restatement as RF
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning, synth
from ranklib_amd.learning import LambdaMART, MART

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the table worked out by hand ------------------------------------------------------------------------------------------------------------
# 4 documents in 2 lists, learning rate 0.5; MART, so lambda = label - score, w = 0 and a leaf's value is s1 / count: every number is dyadic
#          f1   f2   label
#   d0     1    5    2      list 0
#   d1     3    1    0      list 0
#   d2     2    2    0      list 1
#   d3     4    6    1      list 1
HAND_X = np.array([[1, 5], [3, 1], [2, 2], [4, 6]], F32)
HAND_LAB = np.array([2, 0, 0, 1], F32)
HAND_QOFF = np.array([0, 2, 4], np.int32)
HAND_TREES = [
    # stump: f1 <= 2 ? L : R            L = {d0, d2} (2 <= 2 goes LEFT), R = {d1, d3}; old outputs -1, +1
    dict(feature=[1, -1, -1], threshold=[2.0, 0, 0], left=[1, -1, -1], right=[2, -1, -1], output=[0, -1.0, 1.0]),
    # stump: f2 <= 2 ? L : R            L = {d1, d2}, R = {d0, d3}; old outputs +2, -0.5
    dict(feature=[2, -1, -1], threshold=[2.0, 0, 0], left=[1, -1, -1], right=[2, -1, -1], output=[0, 2.0, -0.5]),
    # two levels: f1 <= 2 ? (f2 <= 0.5 ? A : B) : C      A = {} (no f2 is <= 0.5), B = {d0, d2}, C = {d1, d3}; old outputs -4, +4, -1
    dict(feature=[1, 2, -1, -1, -1], threshold=[2.0, 0.5, 0, 0, 0], left=[1, 2, -1, -1, -1], right=[4, 3, -1, -1, -1], output=[0, 0, -4.0, 4.0, -1.0]),
]
HAND = {
    0.0: dict(
        # round 0: scores 0, lambda = (2, 0, 0, 1).  L: s1 = 2 + 0 = 2, / 2 = 1;  R: 0 + 1 = 1, / 2 = 0.5.  scores += 0.5 * (1, .5, 1, .5)
        # round 1: lambda = (1.5, -.25, -.5, .75).  L = {d1, d2}: -.75 / 2 = -.375;  R = {d0, d3}: 2.25 / 2 = 1.125
        # round 2: lambda = (.9375, -.0625, -.3125, .1875).  A empty: keeps -4;  B: .625 / 2 = .3125;  C: .125 / 2 = .0625
        lambdas=[[2, 0, 0, 1], [1.5, -0.25, -0.5, 0.75], [0.9375, -0.0625, -0.3125, 0.1875]],
        sums=[[2.0, 1.0], [-0.75, 2.25], [None, 0.625, 0.125]],
        outputs=[[1.0, 0.5], [-0.375, 1.125], [-4.0, 0.3125, 0.0625]],
        scores=[[0.5, 0.25, 0.5, 0.25], [1.0625, 0.0625, 0.3125, 0.8125], [1.21875, 0.09375, 0.46875, 0.84375]],
        counts=[[4, 2, 2], [4, 2, 2], [4, 2, 0, 2, 2]]),
    0.5: dict(
        # round 0: new (1, .5); stored .5 * -1 + .5 * 1 = 0 and .5 * 1 + .5 * .5 = .75.  scores += .5 * (0, .75, 0, .75)
        # round 1: lambda = (2, -.375, 0, .625).  L: -.375 / 2 = -.1875, stored .5 * 2 + .5 * -.1875 = .90625;  R: 2.625 / 2 = 1.3125, stored
        #          .5 * -.5 + .5 * 1.3125 = .40625.  scores += .5 * (.40625, .90625, .90625, .40625)
        # round 2: lambda = (1.796875, -.828125, -.453125, .421875).  A keeps -4 (no blend either);  B: 1.34375 / 2 = .671875, stored
        #          .5 * 4 + .5 * .671875 = 2.3359375;  C: -.40625 / 2 = -.203125, stored .5 * -1 + .5 * -.203125 = -.6015625
        lambdas=[[2, 0, 0, 1], [2, -0.375, 0, 0.625], [1.796875, -0.828125, -0.453125, 0.421875]],
        sums=[[2.0, 1.0], [-0.375, 2.625], [None, 1.34375, -0.40625]],
        outputs=[[0.0, 0.75], [0.90625, 0.40625], [-4.0, 2.3359375, -0.6015625]],
        scores=[[0, 0.375, 0, 0.375], [0.203125, 0.828125, 0.453125, 0.578125], [1.37109375, 0.52734375, 1.62109375, 0.27734375]],
        counts=[[4, 2, 2], [4, 2, 2], [4, 2, 0, 2, 2]]),
}
D1 = 1.0 / (math.log(3) / math.log(2))   # the discount of rank 2; gain(2) = 3, gain(1) = 1, gain(0) = 0


def _hand_mean(a, b):
    s = F32(0)
    s = F32(float(s) + a)
    s = F32(float(s) + b)
    return F32(s / F32(2))


@pytest.mark.parametrize("decay", [0.0, 0.5])
def test_the_restatement_gives_the_hand_table(decay):
    want = HAND[decay]
    got = RF.refit(HAND_TREES, 0.5, "NDCG", 2, HAND_X, HAND_LAB, HAND_QOFF, decay=decay, ranker="MART", valid=(HAND_X, HAND_LAB, HAND_QOFF), early_stop=0)
    for r in range(3):
        assert np.array_equal(_u64(got["lambdas"][r]), _u64(want["lambdas"][r])) and not got["weights"][r].any(), r
        leaves = RF.leaf_order(HAND_TREES[r])
        assert leaves == ([1, 2] if r < 2 else [2, 3, 4])
        assert np.array_equal(_u32(got["trees"][r]["output"][leaves]), _u32(want["outputs"][r])), r
        assert list(got["trees"][r]["count"]) == want["counts"][r], r
        assert np.array_equal(_u64(got["stages"][r]), _u64(want["scores"][r])) and np.array_equal(_u64(got["vstages"][r]), _u64(want["scores"][r])), r
        for li, s1 in enumerate(want["sums"][r]):       # the sums themselves: s1 / count is the new value the outputs were blended from
            if s1 is not None:
                new = F32(F32(s1) / F32(2))
                assert _u32(RF.blend(decay, HAND_TREES[r]["output"][leaves[li]], new)) == _u32(want["outputs"][r][li]), (r, li)
    assert got["empty"] == 1                               # leaf A of the third tree
    # NDCG@2 after each tree, decay 0: (.5, .25 | .5, .25): list 0 ranks d0 (2) first: 1; list 1 ranks d2 (0), d3 (1): DCG D1, ideal 1.  Then
    # (1.0625, .0625 | .3125, .8125) and (1.21875, .09375 | .46875, .84375): both lists ideal.  decay .5: (0, .375 | 0, .375): list 0 ranks d1 (0),
    # d0 (2): 3 D1 / 3; list 1 ranks d3 (1) first: 1.  (.203125, .828125 | .453125, .578125): D1 and 1.  (1.37, .53 | 1.62, .28): 1 and d2 (0), d3: D1
    ndcg = {0.0: [(1.0, D1), (1.0, 1.0), (1.0, 1.0)], 0.5: [(D1, 1.0), (D1, 1.0), (1.0, D1)]}[decay]
    for r in range(3):
        assert _u32(got["metrics"][r]) == _u32(_hand_mean(*ndcg[r])) == _u32(got["vmetrics"][r]), r
    # best / stop with early_stop 0, by the strict > over the hand values: decay 0: .815 at round 0, 1.0 at round 1 is better, round 2 is no
    # better: 2 - 1 > 0 stops
    best, best_round = 0.0, None
    for r in range(3):
        if float(_hand_mean(*ndcg[r])) > best:
            best, best_round = float(_hand_mean(*ndcg[r])), r
    assert (got["best_round"], got["best_score"], got["stop"]) == (best_round, best, True) and (decay != 0 or best_round == 1)


def test_a_lambdamart_leaf_by_hand():
    """round 0 of the first stump under DCG@2: all scores 0, so rho = 1 / (1 + exp(0)) = 1/2 for every pair and the ranked order is the file's.
    list 0: d0 (2) above d1 (0): delta = |(3 - 0) (1 - D1)|; list 1: d3 (1) below d2 (0): delta' = |(1 - 0) (D1 - 1)|.  lambda = +- delta / 2,
    w = delta / 4 on both documents of a pair.  L = {d0, d2}, R = {d1, d3}: two float sums each, then s1 / s2"""
    got = RF.refit(HAND_TREES[:1], 0.5, "DCG", 2, HAND_X, HAND_LAB, HAND_QOFF)
    d, dp = abs(3.0 * (1.0 - D1)), abs(1.0 * (D1 - 1.0))
    lam, w = [d / 2, -d / 2, -dp / 2, dp / 2], [d / 4, d / 4, dp / 4, dp / 4]
    assert np.allclose(got["lambdas"][0], lam, rtol=1e-15, atol=0) and np.allclose(got["weights"][0], w, rtol=1e-15, atol=0)
    lam, w = got["lambdas"][0], got["weights"][0]          # (the last bit of a product is the restated scorer's: the sums below are the test)
    outs = []
    for a, b in ((0, 2), (1, 3)):
        s1 = F32(float(F32(float(F32(0)) + lam[a])) + lam[b])
        s2 = F32(float(F32(float(F32(0)) + w[a])) + w[b])
        outs.append(F32(s1 / s2))
    assert np.array_equal(_u32(got["trees"][0]["output"][[1, 2]]), _u32(outs))
    assert outs[0] > 0 > outs[1]


def test_a_leaf_whose_weights_are_all_zero_gets_zero_not_its_old_value():
    lab = np.array([1, 1, 0, 0], F32)                      # equal labels inside each list: no pair, lambda = w = 0 everywhere
    got = RF.refit(HAND_TREES[:1], 0.5, "NDCG", 2, HAND_X, lab, HAND_QOFF)
    assert got["empty"] == 0 and list(got["trees"][0]["output"][[1, 2]]) == [0.0, 0.0]
    half = RF.refit(HAND_TREES[:1], 0.5, "NDCG", 2, HAND_X, lab, HAND_QOFF, decay=0.5)
    assert list(half["trees"][0]["output"][[1, 2]]) == [-0.5, 0.5]


def test_decay_zero_replaces_an_infinite_output_and_a_blend_keeps_it():
    tree = dict(HAND_TREES[0], output=[0, np.inf, 1.0])
    got = RF.refit([tree], 0.5, "NDCG", 2, HAND_X, HAND_LAB, HAND_QOFF, ranker="MART")
    assert list(got["trees"][0]["output"][[1, 2]]) == [1.0, 0.5]
    half = RF.refit([tree], 0.5, "NDCG", 2, HAND_X, HAND_LAB, HAND_QOFF, ranker="MART", decay=0.5)
    assert half["trees"][0]["output"][1] == np.inf and half["trees"][0]["output"][2] == 0.75


# ---- 2. the identity on the CPU oracles ---------------------------------------------------------------------------------------------------------------
def _same_as_trained(trees, tms, vms, scores, vscores, got):
    for r, t in enumerate(trees):
        assert np.array_equal(_u32(got["trees"][r]["output"]), _u32(t["output"])), ("outputs of tree", r)
        if "count" in t:
            assert np.array_equal(got["trees"][r]["count"], t["count"]), ("counts of tree", r)
    assert np.array_equal(_u64(got["stages"][-1]), _u64(scores)) and np.array_equal(_u64(got["vstages"][-1]), _u64(vscores))
    assert np.array_equal(_u32(got["metrics"]), _u32(tms)) and np.array_equal(_u32(got["vmetrics"]), _u32(vms))
    assert got["empty"] == 0


@pytest.mark.parametrize("kind,n_docs,n_feat,n_threshold,metric,k,ranker", [
    ("ns", 900, 6, 256, "NDCG", 10, "LAMBDAMART"), ("mslr", 1200, 5, 3, "NDCG", 10, "LAMBDAMART"), ("mslr", 1200, 5, 16, "MAP", 0, "LAMBDAMART"),
    ("ns", 900, 4, 16, "ERR", 10, "LAMBDAMART"), ("ns", 900, 4, 3, "DCG", 10, "LAMBDAMART"), ("mslr", 1200, 5, 256, "DCG", 10, "LAMBDAMART"),
    ("ns", 900, 6, 256, "NDCG", 10, "MART"), ("mslr", 1200, 5, 16, "NDCG", 10, "MART"), ("mslr", 1200, 5, 3, "NDCG", 10, "MART")])
def test_refitting_the_c_oracles_trees_on_its_own_data_gives_them_back(kind, n_docs, n_feat, n_threshold, metric, k, ranker):
    T0 = 4
    X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind, seed_offset=41)
    Xv, lv, qv = synth.make_dataset(n_docs // 3, n_feat, kind, seed_offset=42)
    o = O.Oracle(X, lab, qoff, n_trees=T0, n_leaves=8, n_threshold=n_threshold, k=k, metric=metric, ranker=ranker, early_stop=1)
    o.set_validation(Xv, lv, qv)
    o.init()
    trees, tms, vms = [], [], []
    for _ in range(T0):
        t, tm, vm, _ = o.round()
        trees.append(t.trimmed()); tms.append(tm); vms.append(vm)
    scores, vscores, best = o.scores(), o.valid_scores(), o.best_valid()
    o.close()
    assert all(len(t["feature"]) >= 3 for t in trees)
    got = RF.refit(trees, 0.1, metric, k, X, lab, qoff, ranker=ranker, valid=(Xv, lv, qv), early_stop=1)
    _same_as_trained(trees, tms, vms, scores, vscores, got)
    assert (got["best_round"], got["best_score"]) == best
    moved = RF.refit(trees, 0.1, metric, k, Xv, lv, qv, ranker=ranker)       # (and on other data the values do move: the identity is no tautology)
    assert any(not np.array_equal(_u32(a["output"]), _u32(b["output"])) for a, b in zip(moved["trees"], trees))


@pytest.mark.parametrize("kind,n_threshold,metric,k", [("ns", 16, "P", 3), ("mslr", 3, "P", 3), ("mslr", 256, "RR", 5), ("ns", 3, "RR", 5)])
def test_refitting_the_python_oracles_trees_under_p_and_rr(kind, n_threshold, metric, k):
    T0 = 3
    X, lab, qoff = synth.make_dataset(260, 4, kind, seed_offset=43)
    Xv, lv, qv = synth.make_dataset(120, 4, kind, seed_offset=44)
    m = R.LambdaMART(X, lab, qoff, n_trees=T0, n_leaves=5, n_threshold=n_threshold, k=k, metric="NDCG")
    m.scorer = RF.make_scorer(metric, k)
    m.set_validation(Xv, lv, qv)
    m.init()
    trees, tms, vms = [], [], []
    for _ in range(T0):
        root, tm, vm, _ = m.round()
        feat, thr, left, right, out = R.flatten_tree(root)
        trees.append(dict(feature=np.array(feat), threshold=np.array(thr, F32), left=np.array(left), right=np.array(right), output=np.array(out, F32)))
        tms.append(tm); vms.append(vm)
    got = RF.refit(trees, 0.1, metric, k, X, lab, qoff, valid=(Xv, lv, qv))
    _same_as_trained(trees, tms, vms, np.array(m.model_scores), np.array(m.valid_scores), got)


# ---- 3. the refit run's log, through a stub trainer ------------------------------------------------------------------------------------------------------
class _Scorer:
    def name(self):
        return "NDCG@10"

    def getK(self):
        return 10


class _StubTrainer:
    """counts rounds; a refit makes `model_trees` rounds at once"""
    has_valid = False

    def __init__(self, model_trees=0):
        self.rounds, self.calls, self.model_trees, self.refits = 0, 0, model_trees, []

    def refit_model_text(self, text, decay=0.0):
        self.refits.append((text, decay))
        self.rounds = self.model_trees
        return False

    def boost_round(self, want_tree=True):
        self.rounds += 1
        self.calls += 1
        return None, F32(self.rounds / 100.0), None, False

    def round_metrics(self, r):
        return F32((r + 1) / 100.0), None

    def model_text(self):
        return "## stub\n" + "".join("<tree id=\"%d\">\n" % (i + 1) for i in range(self.rounds))

    def finish(self):
        return 0.5, None

    def num_trees(self):
        return self.rounds

    def get_tree(self, i):
        return i

    def init(self):
        pass


class _Log(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _run(monkeypatch, cls, trainer):
    """init() and learn() of a ranker whose native trainer is `trainer`"""
    monkeypatch.setattr(learning.N, "Model", lambda text, device: None)
    monkeypatch.setattr(learning.N, "Trainer", lambda **kw: trainer)
    monkeypatch.setattr(learning.N, "set_err_max", lambda m: None)
    monkeypatch.setattr(learning, "flatten", lambda lists, features: None)
    monkeypatch.setattr(learning, "feed_trainer", lambda *a, **kw: None)
    monkeypatch.setattr(learning, "metric_name", lambda scorer: "NDCG")
    r = cls(samples=[], features=[1, 2], scorer=_Scorer())
    h = _Log()
    lg = logging.getLogger("ranklib_amd")
    old = lg.level
    lg.addHandler(h); lg.setLevel(logging.INFO)
    try:
        r.init()
        r.learn()
    finally:
        lg.removeHandler(h); lg.setLevel(old)
    return h.lines


@pytest.mark.parametrize("cls", [LambdaMART, MART])
def test_a_refit_run_prints_the_refit_rounds_and_trains_on_behind_them(cls, monkeypatch, tmp_path):
    monkeypatch.setattr(LambdaMART, "nTrees", 6)           # MART inherits the statics
    whole = _StubTrainer()
    log_whole = _run(monkeypatch, cls, whole)
    assert whole.calls == 6 and whole.refits == []
    monkeypatch.setattr(LambdaMART, "refitFrom", "the text")
    monkeypatch.setattr(LambdaMART, "refitDecay", 0.25)
    part = _StubTrainer(model_trees=4)
    log_part = _run(monkeypatch, cls, part)
    assert part.refits == [("the text", 0.25)] and part.calls == 2 and part.rounds == 6          # -tree stays the total
    assert log_part == log_whole and sum(" | " in ln for ln in log_whole) == 7                   # the header and six rounds
    only = _StubTrainer(model_trees=6)
    log_only = _run(monkeypatch, cls, only)
    assert only.calls == 0 and log_only == log_whole                                             # equal to the model's tree count: only the refit
    ck = str(tmp_path / "ck.txt")
    monkeypatch.setattr(LambdaMART, "checkpointFile", ck)
    monkeypatch.setattr(LambdaMART, "checkpointEvery", 5)
    _run(monkeypatch, cls, _StubTrainer(model_trees=4))
    assert open(ck).read().count("<tree id=") == 5                                               # -checkpoint works in the rounds behind a refit


def test_refit_and_resume_together_are_refused_by_the_class_too(monkeypatch):
    monkeypatch.setattr(LambdaMART, "refitFrom", "a")
    monkeypatch.setattr(LambdaMART, "resumeFrom", "b")
    t = _StubTrainer(model_trees=2)
    t.adopt_model_text = lambda text: False
    with pytest.raises(N.RankLibError, match="refitFrom together with resumeFrom"):
        _run(monkeypatch, LambdaMART, t)


def test_random_forests_refuse_the_static(monkeypatch):
    monkeypatch.setattr(LambdaMART, "refitFrom", "<ensemble>\n</ensemble>\n")
    with pytest.raises(N.RankLibError, match="-refit recomputes the leaf values of one.*bags of Random Forests"):
        learning.RFRanker(features=[1], scorer=_Scorer()).init()


# ---- 4. the command line ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,match", [
    (["-refit", "m.txt", "-load", "m.txt", "-test", "t.txt"], "-refit recomputes a model's leaf values on training data: it needs -train"),
    (["-train", "t.txt", "-ranker", "4", "-refit", "m.txt"], "-refit is built for the tree trainers.*not for -ranker 4"),
    (["-train", "t.txt", "-ranker", "2", "-refit", "m.txt", "-decay", "0.5"], "-refit is built for the tree trainers.*not for -ranker 2"),
    (["-train", "t.txt", "-ranker", "8", "-refit", "m.txt"], "bags of Random Forests.*trainers of their own"),
    (["-train", "t.txt", "-ranker", "6", "-kcv", "3", "-refit", "m.txt"], "-refit with -kcv"),
    (["-train", "t.txt", "-ranker", "0", "-refit", "m.txt", "-resume", "m.txt"], "-refit together with -resume"),
    (["-train", "t.txt", "-ranker", "6", "-decay", "0.5"], "-decay x belongs to -refit"),
    (["-train", "t.txt", "-ranker", "6", "-refit", "m.txt", "-decay", "1"], r"-decay must be in \[0, 1\) \(got 1.0\)"),
    (["-train", "t.txt", "-ranker", "6", "-refit", "m.txt", "-decay", "-0.25"], r"-decay must be in \[0, 1\) \(got -0.25\)"),
    (["-train", "t.txt", "-ranker", "6", "-refit", "m.txt", "-decay", "nan"], r"-decay must be in \[0, 1\) \(got nan\)"),
    (["-train", "t.txt", "-ranker", "6", "-refit"], "Missing value for -refit"),
])
def test_the_command_line_refuses(args, match):
    with pytest.raises(N.RankLibError, match=match):
        evaluator.main(args)
    assert LambdaMART.refitFrom is None and LambdaMART.refitDecay == 0.0 and LambdaMART.resumeFrom is None


def test_a_refit_file_that_cannot_be_read_is_refused_like_the_rest(tmp_path):
    missing, binary = str(tmp_path / "none.txt"), tmp_path / "binary.txt"
    binary.write_bytes(b"## LambdaMART\n<ensemble>\n\xff\xfe</ensemble>\n")
    for path, why in ((missing, "No such file"), (str(binary), "ascii")):
        with pytest.raises(N.RankLibError, match="-refit .* cannot be read as a model text.*" + why):
            evaluator.main(["-train", "t.txt", "-ranker", "6", "-refit", path, "-decay", "0.5"])
        assert LambdaMART.refitFrom is None and LambdaMART.refitDecay == 0.0


def test_the_statics_end_with_their_command_line(tmp_path, monkeypatch):
    """main() reads the model and the decay into the statics, hands them to the run and resets them when it returns -- here the run fails on
    its training file, behind the point where the statics were set"""
    model = tmp_path / "m.txt"
    model.write_text("## LambdaMART\n<ensemble>\n</ensemble>\n", encoding="ascii")
    seen = []
    real = evaluator.Evaluator.__init__

    def spy(self, *a, **kw):
        seen.append((LambdaMART.refitFrom, LambdaMART.refitDecay))
        return real(self, *a, **kw)
    monkeypatch.setattr(evaluator.Evaluator, "__init__", spy)
    with pytest.raises(Exception):
        evaluator.main(["-train", str(tmp_path / "no_such_train.txt"), "-ranker", "6", "-refit", str(model), "-decay", "0.5"])
    assert seen == [("## LambdaMART\n<ensemble>\n</ensemble>\n", 0.5)]
    assert LambdaMART.refitFrom is None and LambdaMART.refitDecay == 0.0


def test_the_usage_text_names_the_flags(capsys):
    assert evaluator.main([]) == 0
    out = capsys.readouterr().out
    assert "[-resume model] [-checkpoint file [-every n]] [-refit model [-decay x]]" in out and "-refit model [-decay x] is an rlhip extension" in out


# ---- 5. the boundary ------------------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_declared_and_check_their_handle_first():
    L = N.lib()
    header = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    for name in ("rl_refit_model_text", "rl_debug_refit_stats"):
        assert hasattr(C.CDLL(N.LIB_PATH), name) and name in N.ABI_SYMBOLS
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert "int rl_refit_model_text(rl_trainer *t, const char *text, float decay, int32_t *stop);" in header
    assert L.rl_abi_version() == 5
    stop = C.c_int32(7)
    assert L.rl_refit_model_text(None, b"<ensemble>\n</ensemble>\n", 0.0, C.byref(stop)) == -1
    assert b"null trainer handle" in L.rl_last_error() and stop.value == 7
    out = (C.c_int64 * 3)(5, 5, 5)
    assert L.rl_debug_refit_stats(None, out) == -1 and list(out) == [5, 5, 5]
    assert N.ARM["COUNT_"] == 66                           # the launch-arm table did not grow: which arm ran is rl_debug_refit_stats'
