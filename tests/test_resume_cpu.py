"""Resume without a device: the NumPy restatement of the replay (tests/resume_restatement.py) against a table worked out by
hand and against the CPU oracle -- the premise of the identity: walking the raw rows through a model's trees gives the scores the trainer
that grew them holds, which it got from its bin partition -- then the checkpoint file, the command line's refusals and the exported symbol.
"""
import ctypes as C
import logging
import math
import os

import numpy as np
import pytest

import np_restatement as R
import oracle_ffi as O
import resume_restatement as RR
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning, synth
from ranklib_amd.learning import LambdaMART, MART

F32 = np.float32


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the table worked out by hand ------------------------------------------------------------------------------------------------------------
# 4 documents in 2 lists, learning rate 0.5 (outputs and products are dyadic: every sum below is exact)
#          f1   f2   label
#   d0     1    5    2      list 0
#   d1     3    1    0      list 0
#   d2     2    2    0      list 1
#   d3     4    6    1      list 1
HAND_X = np.array([[1, 5], [3, 1], [2, 2], [4, 6]], F32)
HAND_LAB = np.array([2, 0, 0, 1], F32)
HAND_QOFF = np.array([0, 2, 4], np.int32)
HAND_TREES = [
    # stump: f1 <= 2 ? -1 : +1        d0 -1, d1 +1, d2 -1 (2 <= 2 goes LEFT), d3 +1
    dict(feature=[1, -1, -1], threshold=[2.0, 0, 0], left=[1, -1, -1], right=[2, -1, -1], output=[0, -1.0, 1.0]),
    # stump: f2 <= 2 ? +2 : -0.5      d0 -0.5, d1 +2, d2 +2, d3 -0.5
    dict(feature=[2, -1, -1], threshold=[2.0, 0, 0], left=[1, -1, -1], right=[2, -1, -1], output=[0, 2.0, -0.5]),
    # two levels: f1 <= 2 ? (f2 <= 3 ? -4 : +4) : -1        d0 +4, d1 -1, d2 -4, d3 -1
    dict(feature=[1, 2, -1, -1, -1], threshold=[2.0, 3.0, 0, 0, 0], left=[1, 2, -1, -1, -1], right=[4, 3, -1, -1, -1], output=[0, 0, -4.0, 4.0, -1.0]),
]
HAND_SCORES = [
    [-0.5, 0.5, -0.5, 0.5],            # 0.5 * (-1, +1, -1, +1)
    [-0.75, 1.5, 0.5, 0.25],           # + 0.5 * (-0.5, +2, +2, -0.5)
    [1.25, 1.0, -1.5, -0.25],          # + 0.5 * (+4, -1, -4, -1)
]
D1 = 1.0 / (math.log(3) / math.log(2))   # the discount of rank 2; gain(2) = 3, gain(1) = 1, gain(0) = 0
# NDCG@2 per list after each tree:
#   tree 1: list 0 ranks d1 (label 0), d0 (2): DCG 3 D1, ideal 3 -> D1;   list 1 ranks d3 (1), d2 (0): DCG 1, ideal 1 -> 1
#   tree 2: list 0 ranks d1, d0 again -> D1;                               list 1 ranks d2 (0), d3 (1): DCG D1, ideal 1 -> D1
#   tree 3: list 0 ranks d0 (2), d1 (0) -> 1;                              list 1 ranks d3 (1), d2 (0) -> 1
HAND_NDCG = [(3 * D1 / 3, 1.0), (3 * D1 / 3, 1 * D1 / 1.0), (1.0, 1.0)]


def _hand_mean(a, b):
    s = F32(0)
    s = F32(float(s) + a)
    s = F32(float(s) + b)
    return F32(s / F32(2))


def test_the_restatement_gives_the_hand_table():
    got = RR.replay(HAND_TREES, 0.5, R.NDCG(2), HAND_X, HAND_LAB, HAND_QOFF, valid=(HAND_X, HAND_LAB, HAND_QOFF), early_stop=0)
    for r in range(3):
        assert np.array_equal(_u64(got["stages"][r]), _u64(HAND_SCORES[r])), r
        assert np.array_equal(_u64(got["vstages"][r]), _u64(HAND_SCORES[r])), r
        assert _u32(got["metrics"][r]) == _u32(_hand_mean(*HAND_NDCG[r])) == _u32(got["vmetrics"][r]), r
    assert [float(m) for m in got["metrics"]] == pytest.approx([0.81546488, 0.63092975, 1.0], abs=1e-7)
    # best / stop: 0.815 > 0 at round 0, 0.631 is no better, 1.0 is: the best round is 2 and 2 - 2 > 0 is false
    assert (got["best_round"], got["best_score"], got["stop"]) == (2, 1.0, False)
    two = RR.replay(HAND_TREES[:2], 0.5, R.NDCG(2), HAND_X, HAND_LAB, HAND_QOFF, valid=(HAND_X, HAND_LAB, HAND_QOFF), early_stop=0)
    assert (two["best_round"], two["stop"]) == (0, True) and two["best_score"] == float(_hand_mean(*HAND_NDCG[0]))      # 1 - 0 > 0
    none = RR.replay(HAND_TREES, 0.5, R.NDCG(2), HAND_X, HAND_LAB, HAND_QOFF)
    assert (none["best_round"], none["best_score"], none["stop"]) == (RR.BEST_ROUND_INIT, 0.0, False)                    # no validation set: never


def test_the_product_is_the_double_product():
    """lr = 0.1f and an output whose float product with it rounds: (double)lr * (double)out is another number than (double)(lr * out)"""
    out = np.array([F32(0.3)], F32)
    s = RR.chain_step(np.zeros(1), 0.1, out)
    assert s[0] == float(F32(0.1)) * float(F32(0.3)) != float(F32(0.1) * F32(0.3))
    assert s[0] != 0.1 * float(F32(0.3))                   # and lr is the FLOAT 0.1


# ---- 2. the CPU oracle: walking the raw rows is the bin partition -------------------------------------------------------------------------------------
def _with_infinities(X, lab, mode):
    """feature 2 = +Infinity on a third of the best documents, -Infinity on a fifth of the worst: a column worth splitting on.  "three": the
    rest of the column is 0.5 (three distinct values, the table holds them all from n_threshold = 3 on); "dense": the rest keeps its values
    (more distinct values than thresholds: the Java's step (max - min) / n is Infinity there and the table NaN behind its first entry --
    whatever that table splits, the walk must follow it)"""
    if mode is None:
        return X
    X = X.copy()
    i = np.arange(len(lab))
    if mode == "three":
        X[:, 1] = 0.5
    X[(lab >= 3) & (i % 3 == 0), 1] = np.inf
    X[(lab == 0) & (i % 5 == 0), 1] = -np.inf
    return X


# (n_threshold = 1 and 2 run WITHOUT the column, and must stay so: with fewer thresholds than the column has values AND an infinite range the
# Java's step (max - min) / n is Infinity and its table NaN behind the first entry; binning against that table the CPU oracle writes outside its
# arrays and CORRUPTS ITS HEAP -- the process aborts with "free(): invalid next size" -- and oracle/ is not this change's to mend)
@pytest.mark.parametrize("kind,n_docs,n_feat,n_threshold,metric,inf", [
    ("ns", 1200, 6, 256, "NDCG", "dense"), ("ns", 1200, 6, 1, "NDCG", None), ("mslr", 1500, 5, 3, "NDCG", "three"), ("mslr", 1500, 5, 256, "MAP", "three"),
    ("ns", 900, 4, 16, "ERR", "dense"), ("ns", 900, 4, 2, "DCG", None)])
def test_replaying_the_oracles_trees_gives_the_oracles_state(kind, n_docs, n_feat, n_threshold, metric, inf):
    T0 = 5
    X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind, seed_offset=31)
    Xv, lv, qv = synth.make_dataset(n_docs // 3, n_feat, kind, seed_offset=32)
    X, Xv = _with_infinities(X, lab, inf), _with_infinities(Xv, lv, inf)
    k = 0 if metric == "MAP" else 10
    o = O.Oracle(X, lab, qoff, n_trees=T0, n_leaves=8, n_threshold=n_threshold, k=k, metric=metric, early_stop=1)
    o.set_validation(Xv, lv, qv)
    o.init()
    trees, tms, vms, stops = [], [], [], []
    for _ in range(T0):
        t, tm, vm, stop = o.round()
        trees.append(t.trimmed()); tms.append(tm); vms.append(vm); stops.append(stop)
    assert inf != "three" or any((t["feature"] == 2).any() for t in trees), "the column with the infinities is split on"
    want_s, want_v, want_best = o.scores(), o.valid_scores(), o.best_valid()
    o.close()
    got = RR.replay(trees, 0.1, R.SCORERS[metric](k), X, lab, qoff, valid=(Xv, lv, qv), early_stop=1)
    assert np.array_equal(_u64(got["stages"][-1]), _u64(want_s))
    assert np.array_equal(_u64(got["vstages"][-1]), _u64(want_v))
    assert np.array_equal(_u32(got["metrics"]), _u32(tms)) and np.array_equal(_u32(got["vmetrics"]), _u32(vms))
    assert (got["best_round"], got["best_score"]) == want_best and got["stop"] == stops[-1]
    for r in range(1, T0):                                 # the stop rule round by round: a prefix's replay ends as the oracle's round did
        assert RR.replay(trees[:r], 0.1, R.SCORERS[metric](k), X, lab, qoff, valid=(Xv, lv, qv), early_stop=1)["stop"] == stops[r - 1]


# ---- 3. checkpoints and the resumed loop, through a stub trainer --------------------------------------------------------------------------------------
class _Scorer:
    def name(self):
        return "NDCG@10"


class _StubTrainer:
    """counts rounds; its model text names them"""
    has_valid = False

    def __init__(self, adopted=0, fail_text_at=None):
        self.rounds, self.calls, self.fail_text_at = adopted, 0, fail_text_at

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


class _Log(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _learn(monkeypatch, cls, trainer, resumed=0, resume_stop=False):
    monkeypatch.setattr(learning.N, "Model", lambda text, device: None)
    r = cls(features=[1, 2], scorer=_Scorer())
    r.impacts = np.zeros(2)
    r._trainer, r._resumed, r._resume_stop = trainer, resumed, resume_stop
    h = _Log()
    lg = logging.getLogger("ranklib_amd")
    old = lg.level
    lg.addHandler(h); lg.setLevel(logging.INFO)
    try:
        r.learn()
    finally:
        lg.removeHandler(h); lg.setLevel(old)
    return h.lines


@pytest.mark.parametrize("cls", [LambdaMART, MART])
def test_checkpoints_are_whole_files_moved_into_place(cls, monkeypatch, tmp_path):
    ck = str(tmp_path / "ck.txt")
    monkeypatch.setattr(LambdaMART, "nTrees", 7)
    monkeypatch.setattr(LambdaMART, "checkpointFile", ck)          # MART inherits the statics
    monkeypatch.setattr(LambdaMART, "checkpointEvery", 3)
    moves = []
    real = os.replace

    def replace(src, dst):
        moves.append((src, dst, open(src).read().count("<tree id="), os.path.exists(dst) and open(dst).read().count("<tree id=")))
        real(src, dst)
    monkeypatch.setattr(learning.os, "replace", replace)
    _learn(monkeypatch, cls, _StubTrainer())
    # after rounds 3 and 6, each time the complete text beside the file, then one rename over it; the old file is whole until then
    assert moves == [(ck + ".tmp", ck, 3, False), (ck + ".tmp", ck, 6, 3)]
    assert open(ck).read().count("<tree id=") == 6 and not os.path.exists(ck + ".tmp")


def test_a_failing_write_leaves_the_last_checkpoint(monkeypatch, tmp_path):
    ck = str(tmp_path / "ck.txt")
    monkeypatch.setattr(LambdaMART, "nTrees", 7)
    monkeypatch.setattr(LambdaMART, "checkpointFile", ck)
    monkeypatch.setattr(LambdaMART, "checkpointEvery", 2)
    real_open = open
    opened = []

    def failing_open(path, *a, **kw):
        if str(path).endswith(".tmp"):
            opened.append(path)
            if len(opened) == 2:
                raise OSError(28, "No space left on device")
        return real_open(path, *a, **kw)
    monkeypatch.setattr("builtins.open", failing_open)
    t = _StubTrainer()
    with pytest.raises(OSError, match="No space left"):
        _learn(monkeypatch, LambdaMART, t)
    monkeypatch.undo()
    assert t.rounds == 4 and open(ck).read().count("<tree id=") == 2          # the checkpoint of round 2, whole


def test_no_checkpoint_file_no_writes(monkeypatch, tmp_path):
    monkeypatch.setattr(LambdaMART, "nTrees", 4)
    monkeypatch.setattr(learning.os, "replace", lambda *a: pytest.fail("a run without -checkpoint writes nothing"))
    assert LambdaMART.checkpointFile is None and LambdaMART.resumeFrom is None and LambdaMART.checkpointEvery == 100
    _learn(monkeypatch, LambdaMART, _StubTrainer())


def test_a_resumed_loop_prints_the_adopted_rounds_and_goes_on_behind_them(monkeypatch):
    monkeypatch.setattr(LambdaMART, "nTrees", 6)
    whole = _StubTrainer()
    log_whole = _learn(monkeypatch, LambdaMART, whole)
    part = _StubTrainer(adopted=4)
    log_part = _learn(monkeypatch, LambdaMART, part, resumed=4)
    assert whole.calls == 6 and part.calls == 2 and part.rounds == 6          # -tree stays the total
    assert log_part == log_whole and sum(" | " in ln for ln in log_whole) == 7
    stopped = _StubTrainer(adopted=4)
    log_stopped = _learn(monkeypatch, LambdaMART, stopped, resumed=4, resume_stop=True)
    assert stopped.calls == 0 and log_stopped[:6] == log_whole[:6] and "Finished sucessfully." in log_stopped


# ---- 4. the command line's refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,match", [
    (["-resume", "m.txt", "-load", "m.txt", "-test", "t.txt"], "-resume continues or saves a training run: it needs -train"),
    (["-checkpoint", "c.txt", "-test", "t.txt"], "-checkpoint continues or saves a training run: it needs -train"),
    (["-train", "t.txt", "-ranker", "4", "-resume", "m.txt"], "-resume is built for the tree trainers.*not for -ranker 4"),
    (["-train", "t.txt", "-ranker", "2", "-checkpoint", "c.txt"], "-checkpoint is built for the tree trainers.*not for -ranker 2"),
    (["-train", "t.txt", "-ranker", "8", "-resume", "m.txt"], "bags of Random Forests.*trainers of their own"),
    (["-train", "t.txt", "-ranker", "8", "-checkpoint", "c.txt"], "bags of Random Forests.*trainers of their own"),
    (["-train", "t.txt", "-ranker", "6", "-kcv", "3", "-resume", "m.txt"], "-resume with -kcv"),
    (["-train", "t.txt", "-ranker", "0", "-kcv", "3", "-checkpoint", "c.txt"], "-checkpoint with -kcv"),
    (["-train", "t.txt", "-ranker", "6", "-checkpoint", "c.txt", "-every", "0"], "-every must be >= 1"),
    (["-train", "t.txt", "-ranker", "6", "-checkpoint", "c.txt", "-every", "-5"], "-every must be >= 1"),
    (["-train", "t.txt", "-ranker", "6", "-every", "5"], "-every n belongs to -checkpoint"),
    (["-train", "t.txt", "-ranker", "6", "-resume"], "Missing value for -resume"),
])
def test_the_command_line_refuses(args, match):
    with pytest.raises(N.RankLibError, match=match):
        evaluator.main(args)
    assert LambdaMART.resumeFrom is None and LambdaMART.checkpointFile is None and LambdaMART.checkpointEvery == 100


def test_a_resume_file_that_cannot_be_read_is_refused_like_the_rest(tmp_path):
    missing, binary = str(tmp_path / "none.txt"), tmp_path / "binary.txt"
    binary.write_bytes(b"## LambdaMART\n<ensemble>\n\xff\xfe</ensemble>\n")
    for path, why in ((missing, "No such file"), (str(binary), "ascii")):
        with pytest.raises(N.RankLibError, match="-resume .* cannot be read as a model text.*" + why):
            evaluator.main(["-train", "t.txt", "-ranker", "6", "-resume", path])
        assert LambdaMART.resumeFrom is None


def test_random_forests_refuse_the_statics_too(monkeypatch):
    monkeypatch.setattr(LambdaMART, "resumeFrom", "<ensemble>\n</ensemble>\n")
    with pytest.raises(N.RankLibError, match="bags of Random Forests"):
        learning.RFRanker(features=[1], scorer=_Scorer()).init()


def test_the_usage_text_names_the_flags(capsys):
    assert evaluator.main([]) == 0
    out = capsys.readouterr().out
    assert "[-fastleaf] [-resume model] [-checkpoint file [-every n]]" in out and "rlhip extensions of a -train -ranker 6|0 run" in out


# ---- 5. the boundary ------------------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_checks_its_handle_first():
    L = N.lib()
    assert hasattr(C.CDLL(N.LIB_PATH), "rl_adopt_model_text") and "rl_adopt_model_text" in N.ABI_SYMBOLS
    assert L.rl_abi_version() == 5
    stop = C.c_int32(7)
    assert L.rl_adopt_model_text(None, b"<ensemble>\n</ensemble>\n", 0, C.byref(stop)) == -1
    assert b"null trainer handle" in L.rl_last_error() and stop.value == 7
    assert N.ARM["REPLAY_TILED"] == 64 and N.ARM["REPLAY_DIRECT"] == 65 and N.ARM["COUNT_"] == 66
