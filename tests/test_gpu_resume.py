"""-m gpu: resume (rl_adopt_model_text, k_replay_scores).  A run that is stopped, saved and resumed is the run that was never
stopped, bit for bit: everything here is compared with == on bit views.

Run A trains T rounds and is held at round T0 to be read; run B trains T0 rounds, gives its model text and is destroyed; run C is a fresh
trainer on the same data that adopts the text and trains the rest.  Shapes: 3 000 x 12 `mslr` synth (lists of 1 .. 300 documents), 8 leaves,
T = 12, T0 = 6 unless a case says otherwise.
"""
import logging
import os
import re

import numpy as np
import pytest

import oracle_ffi as O
from ranklib_amd import _native as N
from ranklib_amd import evaluator, synth
from ranklib_amd.learning import LambdaMART, RFRanker
from tree_equiv import assert_equivalent, node_members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "letor")
ARM = N.ARM
T, T0, LEAVES = 12, 6, 8
VALID_SEED = 102
ESTOP_SEED = 105          # on this validation set, with early_stop_rounds = 2, the CPU oracle's best round is 7 and it stops at round 10 (0-based)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


_DATA = {}


def _data(n=3000, f=12, kind="mslr", seed=0):
    key = (n, f, kind, seed)
    if key not in _DATA:
        _DATA[key] = synth.make_dataset(n, f, kind, seed_offset=seed)
    return _DATA[key]


def _trainer(cfg, train=None, valid=None, feature_ids=None):
    X, lab, qoff = train if train is not None else _data()
    g = N.Trainer(**cfg)
    g.set_train(X, lab, qoff, feature_ids=feature_ids)
    if valid is not None:
        g.set_validation(*valid)
    g.init()
    return g


def _state(g, rounds):
    """what a round leaves behind that the next one reads, and what a caller can ask for"""
    s = dict(score=g.array("SCORE"), metrics=[g.round_metrics(r) for r in range(rounds)], best=g.best_validation())
    if g.has_valid:
        s["vscore"] = g.array("VALID_SCORE")
    return s


def _same_state(a, b, ctx):
    assert np.array_equal(_u64(a["score"]), _u64(b["score"])), (ctx, "SCORE")
    if "vscore" in a:
        assert np.array_equal(_u64(a["vscore"]), _u64(b["vscore"])), (ctx, "VALID_SCORE")
    assert len(a["metrics"]) == len(b["metrics"])
    for r, (ma, mb) in enumerate(zip(a["metrics"], b["metrics"])):
        assert _u32(ma[0]) == _u32(mb[0]), (ctx, "train metric of round %d" % r, ma, mb)
        assert (ma[1] is None) == (mb[1] is None) and (ma[1] is None or _u32(ma[1]) == _u32(mb[1])), (ctx, "validation metric of round %d" % r, ma, mb)
    assert a["best"][0] == b["best"][0] and _u64(a["best"][1]) == _u64(b["best"][1]), (ctx, "best_validation", a["best"], b["best"])


def _same_tree(a, b, ctx):
    a, b = a.trimmed(), b.trimmed()
    for k in ("feature", "left", "right"):
        assert np.array_equal(a[k], b[k]), (ctx, k)
    for k in ("threshold", "output"):
        assert np.array_equal(_u32(a[k]), _u32(b[k])), (ctx, k)


def _train(g, first, last):
    """rounds first .. last - 1; -> the round whose stop flag ended them, or None"""
    for m in range(first, last):
        _, _, _, stop = g.boost_round(want_tree=False)
        if stop:
            return m
    return None


def _end(g):
    """finish() and everything a finished trainer shows"""
    n_rounds = g.num_trees()                  # before the rollback
    fin = g.finish()
    return dict(fin=fin, trees=[g.get_tree(i) for i in range(g.num_trees())], metrics=[g.round_metrics(r) for r in range(n_rounds)], text=g.model_text(),
                best=g.best_validation())


def _same_end(a, c, ctx):
    assert _u64(a["fin"][0]) == _u64(c["fin"][0]), (ctx, "final train score")
    assert (a["fin"][1] is None) == (c["fin"][1] is None) and (a["fin"][1] is None or _u64(a["fin"][1]) == _u64(c["fin"][1])), (ctx, "final validation score")
    assert len(a["trees"]) == len(c["trees"]), ctx
    for i, (ta, tc) in enumerate(zip(a["trees"], c["trees"])):
        _same_tree(ta, tc, (ctx, "tree %d" % i))
    _same_state(dict(score=np.zeros(1), metrics=a["metrics"], best=a["best"]), dict(score=np.zeros(1), metrics=c["metrics"], best=c["best"]), ctx)
    assert a["text"] == c["text"], (ctx, "model text")


def _abc(cfg, t0=T0, t=T, train=None, valid=None, scratch=0, feature_ids=None):
    """-> (A's state at t0, C's state after adoption, A's end, C's end, C's stop flag of the adoption, the arms C counted)"""
    cfg = dict(n_trees=t, n_leaves=LEAVES, **cfg)
    a = _trainer(cfg, train, valid, feature_ids)
    assert _train(a, 0, t0) is None
    a_mid = _state(a, t0)
    a_stop = _train(a, t0, t)
    a_end = _end(a)
    a.close()
    b = _trainer(cfg, train, valid, feature_ids)
    assert _train(b, 0, t0) is None
    text = b.model_text()
    b.close()
    assert text.count("<tree id=") == t0
    c = _trainer(cfg, train, valid, feature_ids)
    stop = c.adopt_model_text(text, scratch)
    assert c.num_trees() == t0
    c_mid = _state(c, t0)
    for r in range(t0):
        tr = c.get_tree(r).trimmed()
        assert np.all(tr["count"] == -1) and np.all(np.isnan(tr["deviance"])), "adopted trees carry no diagnostics"
    c_stop = None if stop else _train(c, t0, t)
    c_end = _end(c)
    arms = c.array("LAUNCH_ARMS")
    c.close()
    assert a_stop == c_stop
    return a_mid, c_mid, a_end, c_end, stop, arms


def _valid():
    return _data(1000, 12, "mslr", VALID_SEED)


IDENTITY = {
    "ndcg10": dict(metric="NDCG", metric_k=10),
    "map": dict(metric="MAP", metric_k=0),
    "err10": dict(metric="ERR", metric_k=10),
    "p3": dict(metric="P", metric_k=3),
    "rr5": dict(metric="RR", metric_k=5),
    "mart": dict(ranker="MART"),
    "sampled": dict(feature_sampling_rate=0.5, seed=20240614),
    "fast_leaf": dict(flags=N.RL_FLAG_FAST_LEAF),
}


@pytest.mark.parametrize("with_valid", [False, True], ids=["train_only", "with_validation"])
@pytest.mark.parametrize("name", sorted(IDENTITY))
def test_a_resumed_run_is_the_uninterrupted_run(name, with_valid):
    a_mid, c_mid, a_end, c_end, stop, arms = _abc(IDENTITY[name], valid=_valid() if with_valid else None)
    assert not stop
    _same_state(a_mid, c_mid, (name, "after adoption"))
    assert len(a_end["metrics"]) == T and len(a_end["trees"]) == (a_end["best"][0] + 1 if with_valid else T)      # (finish() rolls back to the best validation round)
    _same_end(a_end, c_end, (name, "at the end"))
    launches = 2 if with_valid else 1                      # one chunk holds the six trees at the default scratch: one launch per data set
    assert arms[ARM["REPLAY_TILED"]] == launches and arms[ARM["REPLAY_DIRECT"]] == 0


@pytest.mark.parametrize("with_valid", [False, True], ids=["train_only", "with_validation"])
def test_the_strict_java_order_resumes_too(with_valid):
    a_mid, c_mid, a_end, c_end, stop, _ = _abc(dict(flags=N.RL_FLAG_JAVA_ORDER), t0=3, t=6, valid=_valid() if with_valid else None)
    assert not stop
    _same_state(a_mid, c_mid, "java order, after adoption")
    _same_end(a_end, c_end, "java order, at the end")


# ---- early stopping -------------------------------------------------------------------------------------------------------------------------
def _estop_cfg():
    return dict(early_stop_rounds=2), _data(1000, 12, "mslr", ESTOP_SEED)


def test_a_checkpoint_before_the_best_round_stops_where_the_run_stopped():
    cfg, valid = _estop_cfg()
    a_mid, c_mid, a_end, c_end, stop, _ = _abc(cfg, valid=valid)          # _abc asserts that A and C stop at the same round
    assert not stop
    _same_state(a_mid, c_mid, "early stop, after adoption")
    assert len(a_end["metrics"]) < T, "A must stop before round 12 on this data (the seed was picked on the CPU oracle for it)"
    assert a_end["best"][0] >= T0, "the checkpoint is taken before the best round"
    assert len(a_end["trees"]) == a_end["best"][0] + 1 < len(a_end["metrics"])      # rolled back
    _same_end(a_end, c_end, "early stop, at the end")


def test_a_model_whose_replay_meets_the_stop_rule_reports_stop():
    cfg, valid = _estop_cfg()
    cfg = dict(n_trees=T, n_leaves=LEAVES, **cfg)
    a = _trainer(cfg, valid=valid)
    stopped = _train(a, 0, T)
    assert stopped is not None and stopped < T - 1
    text = a.model_text()                                  # all trees so far, not rolled back: what a checkpoint holds
    a_mid = _state(a, stopped + 1)
    a_end = _end(a)
    a.close()
    c = _trainer(cfg, valid=valid)
    assert c.adopt_model_text(text) is True
    _same_state(a_mid, _state(c, stopped + 1), "stop at adoption")
    _same_end(a_end, _end(c), "stop at adoption, finished")
    c.close()


# ---- the oracle: A and C cannot be wrong together -----------------------------------------------------------------------------------------------
def test_the_resumed_trees_are_the_cpu_oracles():
    X, lab, qoff = _data()
    _, _, _, c_end, _, _ = _abc(dict())
    o = O.Oracle(X, lab, qoff, n_trees=T, n_leaves=LEAVES)
    o.init()
    for r in range(T):
        to, tm, _, _ = o.round()
        tc = c_end["trees"][r]
        if r < T0:      # an adopted tree carries count = -1 (the text does not hold it): what `count` means is taken from a replay on the training rows
            mem = node_members(tc.trimmed(), X)
            for n in range(tc.n_nodes):
                tc.count[n] = len(mem[n])
        assert assert_equivalent(to, tc, X, ctx="round %d" % r) == 0
        assert _u32(tm) == _u32(c_end["metrics"][r][0]), r
    o.close()


# ---- a kernel that did nothing cannot pass ----------------------------------------------------------------------------------------------------
def test_every_adopted_tree_moves_scores_and_rounds_without_adoption_differ():
    cfg = dict(n_trees=T, n_leaves=LEAVES)
    a = _trainer(cfg)
    prev = a.array("SCORE")
    assert not prev.any()
    trees_a, mets_a = [], []
    for r in range(T):
        t, tm, _, _ = a.boost_round()
        trees_a.append(t); mets_a.append(tm)
        cur = a.array("SCORE")
        step = cur - prev
        assert len(np.unique(step)) >= 2 and np.count_nonzero(step) >= 2, "tree %d moves the scores of at least two leaves" % r
        prev = cur
    a.close()
    d = _trainer(cfg)                                      # no adoption: its rounds are A's rounds 0 .. 5, not 6 .. 11
    for r in range(T0):
        t, tm, _, _ = d.boost_round()
        _same_tree(trees_a[r], t, r)
        later = trees_a[T0 + r].trimmed()
        assert t.n_nodes != trees_a[T0 + r].n_nodes or not np.array_equal(_u32(t.trimmed()["output"]), _u32(later["output"])), r
        assert _u32(tm) != _u32(mets_a[T0 + r]), r
    d.close()


# ---- chunking and edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trees_per_chunk", [1, 2, T0])
def test_the_chunk_size_cannot_change_a_bit(trees_per_chunk):
    valid = _valid()
    per_tree = 8 * (3000 + 1000)
    a_mid, c_mid, a_end, c_end, _, arms = _abc(dict(), valid=valid, scratch=per_tree * trees_per_chunk + 7)
    _same_state(a_mid, c_mid, ("chunks of", trees_per_chunk))
    _same_end(a_end, c_end, ("chunks of", trees_per_chunk))
    assert arms[ARM["REPLAY_TILED"]] == 2 * -(-T0 // trees_per_chunk)


def _small(n_docs, n_feat, n_lists, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_docs, n_feat)).astype(np.float32)
    X[:, 0] = np.round(X[:, 0], 1)                         # ties
    lab = rng.integers(0, 5, n_docs).astype(np.float32)
    cuts = np.sort(rng.choice(np.arange(1, n_docs), n_lists - 1, replace=False)) if n_lists > 1 else np.zeros(0, np.int64)
    qoff = np.concatenate([[0], cuts, [n_docs]]).astype(np.int32)
    return X, lab, qoff


@pytest.mark.parametrize("n_docs,n_feat,n_lists", [(65, 12, 2), (63, 12, 3), (64, 12, 3), (129, 5, 4), (700, 1, 9), (700, 40, 9)])
def test_sizes_around_the_tile_and_narrow_and_wide_rows(n_docs, n_feat, n_lists):
    train = _small(n_docs, n_feat, n_lists, 7 * n_docs + n_feat)
    valid = _small(n_docs + 1, n_feat, n_lists, 11 * n_docs + n_feat)
    a_mid, c_mid, a_end, c_end, _, _ = _abc(dict(), train=train, valid=valid)
    _same_state(a_mid, c_mid, (n_docs, n_feat))
    _same_end(a_end, c_end, (n_docs, n_feat))


def test_a_tree_that_is_a_single_split():
    cfg = dict(n_trees=T, n_leaves=2)
    a = _trainer(cfg)
    _train(a, 0, T0)
    text, a_mid = a.model_text(), _state(a, T0)
    assert a.get_tree(0).n_nodes == 3
    _train(a, T0, T)
    a_end = _end(a)
    a.close()
    c = _trainer(cfg)
    assert c.adopt_model_text(text) is False
    _same_state(a_mid, _state(c, T0), "stumps, after adoption")
    _train(c, T0, T)
    _same_end(a_end, _end(c), "stumps")
    c.close()


def test_one_adopted_tree():
    a_mid, c_mid, a_end, c_end, _, _ = _abc(dict(), t0=1, t=4)
    _same_state(a_mid, c_mid, "T0 = 1")
    _same_end(a_end, c_end, "T0 = 1")


def test_every_tree_adopted_leaves_no_round_but_finish_works():
    valid = _valid()
    cfg = dict(n_trees=T0, n_leaves=LEAVES)
    a = _trainer(cfg, valid=valid)
    _train(a, 0, T0)
    text, a_mid = a.model_text(), _state(a, T0)
    a_end = _end(a)
    a.close()
    c = _trainer(cfg, valid=valid)
    c.adopt_model_text(text)
    _same_state(a_mid, _state(c, T0), "T0 = n_trees")
    with pytest.raises(N.RankLibError, match="all n_trees rounds are done"):
        c.boost_round()
    _same_end(a_end, _end(c), "T0 = n_trees")
    c.close()


def test_both_kernel_arms_are_bit_equal(monkeypatch):
    valid = _valid()
    tiled = _abc(dict(), valid=valid)
    assert tiled[5][ARM["REPLAY_TILED"]] == 2 and tiled[5][ARM["REPLAY_DIRECT"]] == 0
    monkeypatch.setenv("RLHIP_REPLAY_DIRECT", "1")         # a trainer reads its knobs when it is created
    direct = _abc(dict(), valid=valid)
    assert direct[5][ARM["REPLAY_TILED"]] == 0 and direct[5][ARM["REPLAY_DIRECT"]] == 2
    _same_state(tiled[1], direct[1], "tiled against direct")
    _same_state(tiled[0], direct[1], "A against direct")
    _same_end(tiled[3], direct[3], "tiled against direct, at the end")


@pytest.mark.parametrize("n_feat,arm", [(300, "REPLAY_TILED"), (640, "REPLAY_TILED"), (641, "REPLAY_DIRECT")])
def test_rows_wider_than_64_kib_of_tile_and_the_fallback_beyond_the_lds(n_feat, arm, monkeypatch):
    """a tile of 64 documents is 256 F bytes: 75 KiB at F = 300 (past the 64 KiB a kernel gets unasked), all 160 KiB of a CU at F = 640, and at
    F = 641 no tile fits: the direct arm is taken without the knob.  Both arms, bit for bit, where the tile fits"""
    train, valid = _small(130, n_feat, 5, n_feat), _small(70, n_feat, 3, n_feat + 1)
    own = _abc(dict(), t0=2, t=4, train=train, valid=valid)
    assert own[5][ARM[arm]] == 2 and own[5][ARM["REPLAY_TILED"]] + own[5][ARM["REPLAY_DIRECT"]] == 2
    _same_state(own[0], own[1], (n_feat, "after adoption"))
    _same_end(own[2], own[3], (n_feat, "at the end"))
    used = set(int(f) for t in own[3]["trees"] for f in t.trimmed()["feature"] if f != -1)
    assert max(used) > 64, "a column beyond the first 64 is split on"
    if arm == "REPLAY_TILED":
        monkeypatch.setenv("RLHIP_REPLAY_DIRECT", "1")
        direct = _abc(dict(), t0=2, t=4, train=train, valid=valid)
        assert direct[5][ARM["REPLAY_DIRECT"]] == 2 and direct[5][ARM["REPLAY_TILED"]] == 0
        _same_state(own[1], direct[1], (n_feat, "tiled against direct"))
        _same_end(own[3], direct[3], (n_feat, "tiled against direct, at the end"))


def test_feature_ids_are_mapped_to_the_trainers_columns():
    """the text names feature ids, the trainer's rows have columns: ids that are no 1 .. F are found through feature_ids"""
    fid = np.array([40, 3, 17, 5, 90, 2, 8, 61, 33, 12, 7, 25], np.int32)
    a_mid, c_mid, a_end, c_end, _, _ = _abc(dict(), feature_ids=fid)
    assert set(int(f) for t in c_end["trees"] for f in t.trimmed()["feature"] if f != -1) <= set(int(f) for f in fid)
    _same_state(a_mid, c_mid, "feature ids")
    _same_end(a_end, c_end, "feature ids")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six_trees():
    g = _trainer(dict(n_trees=T, n_leaves=LEAVES))
    _train(g, 0, T0)
    text = g.model_text()
    g.close()
    return text


def _refused(g, text, match, scratch=0, status=-1):
    rounds = g.num_trees()
    before = _state(g, rounds)
    with pytest.raises(N.RankLibError, match=match) as e:
        g.adopt_model_text(text, scratch)
    assert "(rlhip status %d)" % status in str(e.value), str(e.value)
    assert g.num_trees() == rounds                         # a refusal leaves the trainer as it was
    _same_state(before, _state(g, rounds), ("refused", match))


def test_refusals_name_their_cause(six_trees):
    g = _trainer(dict(n_trees=T, n_leaves=LEAVES))
    _refused(g, None, "null text")
    _refused(g, "<ensemble>\n<tree id=\"1\" weight=\"0.1\">\n<split>\n<feature> x </feature>", "Emsemble.*bad feature id")
    _refused(g, "## LambdaMART\n<ensemble>\n</ensemble>\n", "no trees")
    _refused(g, six_trees + six_trees, "more than one <ensemble>")
    _refused(g, six_trees, "scratch_bytes must be >= 0", scratch=-1)
    used = re.search(r"<feature>(\d+) </feature>", six_trees).group(0)
    _refused(g, six_trees.replace(used, "<feature>77 </feature>", 1), "tree 0 splits on feature 77, which is not among the trainer's feature_ids")
    assert six_trees.count('weight="0.1"') == T0
    _refused(g, six_trees.replace('weight="0.1"', 'weight="0.25"', 1), "tree 0 has weight 0.25.*learning_rate is 0.1")
    assert g.adopt_model_text(six_trees) is False          # after all that the same handle still adopts
    _refused(g, six_trees, "before the first round", status=-3)
    g.close()
    g = _trainer(dict(n_trees=T0 - 1, n_leaves=LEAVES))
    _refused(g, six_trees, "6 trees.*n_trees is 5")
    g.close()
    g = _trainer(dict(n_trees=T, n_leaves=4))
    _refused(g, six_trees, r"has \d+ nodes.*capacity is 7.*-leaf")
    g.boost_round()
    _refused(g, six_trees, "before the first round", status=-3)
    g.finish()
    _refused(g, six_trees, "rl_finish has been called", status=-3)
    g.close()
    g = _trainer(dict(n_trees=T, n_leaves=LEAVES, learning_rate=0.3))
    _refused(g, six_trees, "tree 0 has weight 0.1.*learning_rate is 0.3")
    g.close()


def test_refused_before_init_and_on_a_sharded_trainer(six_trees):
    X, lab, qoff = _data()
    g = N.Trainer(n_trees=T, n_leaves=LEAVES)
    g.set_train(X, lab, qoff)
    with pytest.raises(N.RankLibError, match="rl_init has not been called"):
        g.adopt_model_text(six_trees)
    g.close()
    g = N.Trainer(n_trees=T, n_leaves=LEAVES)
    g.set_train(X, lab, qoff)
    g.dist_init_callback(0, 1, lambda arr, op: None, lambda src: src.copy())
    g.init()
    with pytest.raises(N.RankLibError, match="sharded") as e:
        g.adopt_model_text(six_trees)
    assert "(rlhip status -4)" in str(e.value)
    g.close()


# ---- Python and the command line ------------------------------------------------------------------------------------------------------------------
class _Log(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _cli(args):
    h = _Log()
    lg = logging.getLogger("ranklib_amd")
    lg.addHandler(h)
    old = lg.level
    lg.setLevel(logging.INFO)
    try:
        assert evaluator.main(args) == 0
    finally:
        lg.removeHandler(h)
        lg.setLevel(old)
    a = h.lines.index("Training starts...")
    b = h.lines.index("Finished sucessfully.")
    return h.lines[a:b + 3]                                # the table and the final scores


@pytest.mark.parametrize("case", ["mart", "lambdamart_validation"])
def test_checkpoint_and_resume_from_the_command_line(case, tmp_path, monkeypatch):
    for cls, names in ((LambdaMART, ("nTrees", "nTreeLeaves", "learningRate", "nThreshold", "minLeafSupport", "nRoundToStopEarly")),
                       (RFRanker, ("nTrees", "nTreeLeaves", "learningRate", "minLeafSupport"))):
        for nm in names:
            monkeypatch.setattr(cls, nm, getattr(cls, nm))          # -tree / -leaf / -shrinkage write both sets of statics: restored when the test ends
    if case == "mart":
        common = ["-train", os.path.join(GOLDEN, "mart_ndcg.train.txt"), "-ranker", "0", "-metric2t", "NDCG@10", "-leaf", "7"]
    else:
        common = ["-train", os.path.join(GOLDEN, "valid_estop.train.txt"), "-validate", os.path.join(GOLDEN, "valid_estop.valid.txt"), "-ranker", "6",
                  "-metric2t", "NDCG@10", "-leaf", "6", "-shrinkage", "0.3"]
    common += ["-tree", "12"]
    one, ck, two = (str(tmp_path / n) for n in ("one.txt", "ck.txt", "two.txt"))
    log_one = _cli(common + ["-save", one])
    log_ck = _cli(common + ["-checkpoint", ck, "-every", "6", "-save", str(tmp_path / "with_ck.txt")])
    assert log_ck == log_one and open(str(tmp_path / "with_ck.txt")).read() == open(one).read()       # writing checkpoints changes nothing
    assert not os.path.exists(ck + ".tmp")
    held = open(ck).read()
    assert held.count("<tree id=") == 12                   # the last complete checkpoint: all trees after round 12 ...
    _cli(common[:-1] + ["6", "-checkpoint", ck, "-every", "6"])
    assert open(ck).read().count("<tree id=") == 6         # ... and the one a run killed behind round 6 would have left
    assert LambdaMART.checkpointFile is None and LambdaMART.resumeFrom is None                          # the flags end with their command line
    log_two = _cli(common + ["-resume", ck, "-save", two])
    assert log_two == log_one
    assert open(two).read() == open(one).read()
