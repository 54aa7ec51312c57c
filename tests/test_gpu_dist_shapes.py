"""-m gpu: the sharded tree trainer on every data shape that changes its kernels (tests/dist_shapes.py), against the CPU oracle.

tests/test_gpu_dist.py holds k ranks to one rank on small dense data.  Here 2 and 3 ranks (separate processes on the one GPU, host-callback transport
over gloo) train on the shapes that select the other kernels -- sparse columns, columns in runs, tables wider than the LDS row stride, thousands of
columns, 300 leaves, one list longer than every other shard, infinite values -- and are compared round by round with the Java-exact oracle ON THE
UNSHARDED DATA, which shares no code with the GPU path: trees with their stored (feature, threshold) pairs, leaf outputs, the per-round and the final
train metric, the concatenated scores, bit for bit; and with the one-GPU run through test_gpu_dist.same().

A case that passes on the default kernel proves nothing about the kernel it names, so every case asserts, from the launch counters and decisions
that EVERY rank reports (RL_ARR_LAUNCH_ARMS, gathered by tests/dist_worker.py), which arm ran on which rank.  Several decisions are rank-local
(any_runs, the compact rows: DESIGN.md 6), so two ranks of one job may run different kernels in the same step: split_decision and split_crows build
that on purpose.

The oracle's rounds and the one-GPU run are computed once per shape (module-scoped cache), not per world size.
"""
import os

import numpy as np
import pytest

import dist_shapes
import oracle_ffi as O
from ranklib_amd import _native as N
from ranklib_amd import dist as D
from test_gpu_dist import CFG, launch_workers, same, saved_run
from tree_equiv import assert_equivalent

pytestmark = pytest.mark.gpu

ARM, HARM = N.ARM, N.HARM
THREADS = min(16, os.cpu_count() or 8)
PART_TILE = 2048              # RL_PART_TILE (rl_internal.h): documents of one partition tile
DENSE_ROOT = {"FQ_PACKED", "FQ_ROWS16", "PACKED", "ROWS16"}


class SavedTree:
    """a tree of a worker's .npz with the interface assert_equivalent reads"""

    def __init__(self, t):
        self.t, self.n_nodes = t, len(t["feature"])

    def trimmed(self):
        return self.t


class Reference:
    """one shape: the unsharded arrays, the oracle's rounds, the one-GPU run"""

    def __init__(self, name=None, data=None, leaves=None, rounds=None):
        self.s = dist_shapes.SHAPES[name] if name else dist_shapes.Shape(data[0].shape[0], data[0].shape[1], leaves, rounds)
        s = self.s
        self.X, self.lab, self.qoff = dist_shapes.make(name) if name else data
        o = O.Oracle(self.X, self.lab, self.qoff, n_trees=s.rounds, n_leaves=s.leaves, metric=s.metric, k=s.k, n_threshold=s.tc, n_threads=THREADS)
        o.init()
        self.rounds = []
        for _ in range(s.rounds):
            t, tm, _, _ = o.round()
            self.rounds.append((t, tm))
        self.scores = o.scores()
        self.final = o.finish()[0]
        o.close()
        # a shape whose sharded runs keep the first tied candidate is held to the one-GPU run that does the same (RL_FLAG_FIRST_TIE)
        g = N.Trainer(n_trees=s.rounds, n_leaves=s.leaves, metric=s.metric, metric_k=s.k, n_threshold=s.tc, flags=0 if s.tie_on else N.RL_FLAG_FIRST_TIE)
        g.set_train(self.X, self.lab, self.qoff)
        g.init()
        trees, mets = [], []
        for _ in range(s.rounds):
            t, tm, _, _ = g.boost_round()
            trees.append(t.trimmed()); mets.append(float(tm))
        final, _ = g.finish()
        self.one_gpu = (trees, mets, g.array("SCORE"), final)
        g.close()

    def check(self, z, ctx):
        """the sharded run `z` against the oracle and against one GPU; returns the per-rank launch arms"""
        s = self.s
        run = saved_run(z, s.rounds)
        arms = z["arms_all"]
        tie = arms[:, ARM["SET_TIE_ON"]]
        assert ((tie != 0) if s.tie_on else (tie == 0)).all(), (ctx, "SET_TIE_ON per rank", tie)
        for r, (to, tm) in enumerate(self.rounds):
            ties = assert_equivalent(to, SavedTree(run[0][r]), self.X, "%s round %d" % (ctx, r))
            assert not s.tie_on or ties == 0, "%d split(s) store another (feature, threshold) than the oracle's (%s round %d)" % (ties, ctx, r)
            assert np.float32(run[1][r]).view(np.uint32) == np.float32(tm).view(np.uint32), (ctx, r, run[1][r], tm)
        assert run[3] == self.final, (ctx, run[3], self.final)
        assert np.array_equal(np.ascontiguousarray(run[2]).view(np.int64), self.scores.view(np.int64)), ctx
        same(self.one_gpu, run)
        return arms


class Cache:
    def __init__(self):
        self.refs = {}

    def get(self, name):
        if name not in self.refs:
            self.refs[name] = Reference(name)
        return self.refs[name]


@pytest.fixture(scope="module")
def refs():
    return Cache()


def launch(name, world, tmp_path, worker_env=None):
    s = dist_shapes.SHAPES[name]
    return launch_workers(world, 29581 + world, str(tmp_path / "shape.npz"), (s.docs, s.feat, "shape", 0, s.leaves, s.rounds), "LAMBDAMART", s.metric, s.k,
                          opts="shape=" + name, worker_env=worker_env)


def passes(a, base):
    """{arm: launches} of one rank's root (HIST_ROOT) or child (HIST_CHILD) histogram passes"""
    return {k: int(a[ARM[base] + v]) for k, v in HARM.items() if k != "COUNT_" and a[ARM[base] + v]}


def regrown(z):
    return int(z["tie_stats"][9])          # trees grown a second time: one more root pass, leaf exchange and plan each (the same on every rank)


# ---- what each shape requires of the arms, per rank ---------------------------------------------------------------------------------------
def _sparse(ref, z, arms, world):
    for r, a in enumerate(arms):
        assert a[ARM["SET_CROWS"]] == 1 and a[ARM["SET_ANY_RUNS"]] == 0, (r, a)
        assert list(passes(a, "HIST_CHILD")) == ["COMPACT"], (r, passes(a, "HIST_CHILD"))
        root = passes(a, "HIST_ROOT")
        assert root and set(root) <= DENSE_ROOT and sum(root.values()) == ref.s.rounds + regrown(z), (r, root)
    info = z["sparse_all"]
    assert (info[:, 0] == 0).all() and (info[:, 1] == 0).all(), info          # no group has entry lists: the sparse root pass is off under sharding
    assert (info[:, 4] >= 3).all() and (info[:, 4] < 6).all(), info           # compact rows for the sparse groups, not for the 20 dense columns' groups


def _runs(ref, z, arms, world):
    for r, a in enumerate(arms):
        assert a[ARM["SET_ANY_RUNS"]] == 1 and a[ARM["SET_CROWS"]] == 0, (r, a)
        assert a[ARM["QUANTIZE"]] == ref.s.rounds, (r, a[ARM["QUANTIZE"]])          # (the RUNS root pass does not quantise; a regrown tree keeps q)
        root, child = passes(a, "HIST_ROOT"), passes(a, "HIST_CHILD")
        assert root and child and all(k.endswith("_RUNS") for k in list(root) + list(child)), (r, root, child)


def _split_decision(ref, z, arms, world):
    runs = arms[:, ARM["SET_ANY_RUNS"]]
    assert runs[0] == 1 and runs[world - 1] == 0, runs          # the ranks of ONE job decided differently
    for r, a in enumerate(arms):
        root, child = passes(a, "HIST_ROOT"), passes(a, "HIST_CHILD")
        if runs[r]:       # k_quantize, then a root pass that folds runs
            assert a[ARM["QUANTIZE"]] == ref.s.rounds and all(k.endswith("_RUNS") for k in list(root) + list(child)), (r, a[ARM["QUANTIZE"]], root, child)
        else:             # the root pass quantised the lambdas itself
            assert a[ARM["QUANTIZE"]] == 0 and root and set(root) <= {"FQ_PACKED", "FQ_ROWS16"} | ({"PACKED"} if regrown(z) else set()), (r, a[ARM["QUANTIZE"]], root)
            assert child and not any(k.endswith("_RUNS") for k in child), (r, child)
    steps = arms[:, ARM["STEPS_ENQUEUED"]]
    assert (steps == steps[0]).all() and steps[0] > 0, steps          # different kernels, the same growth steps


def _split_crows(ref, z, arms, world):
    crows = arms[:, ARM["SET_CROWS"]]
    assert crows[0] == 0 and crows[world - 1] == 1 and not arms[:, ARM["SET_ANY_RUNS"]].any(), (crows, arms[:, ARM["SET_ANY_RUNS"]])
    for r, a in enumerate(arms):          # one rank reads compact rows in every child pass of the job, another the 32-byte rows
        assert list(passes(a, "HIST_CHILD")) == (["COMPACT"] if crows[r] else ["ROWS16"]), (r, passes(a, "HIST_CHILD"))
        root = passes(a, "HIST_ROOT")
        assert a[ARM["QUANTIZE"]] == 0 and root and set(root) <= {"FQ_PACKED"} | ({"PACKED"} if regrown(z) else set()), (r, a[ARM["QUANTIZE"]], root)
    assert (z["sparse_all"][:, 4] > 0).tolist() == (crows == 1).tolist(), z["sparse_all"]
    steps = arms[:, ARM["STEPS_ENQUEUED"]]
    assert (steps == steps[0]).all() and steps[0] > 0, steps


def _stride(ref, z, arms, world):
    for r, a in enumerate(arms):
        assert list(passes(a, "HIST_ROOT")) == ["STRIDE"] and list(passes(a, "HIST_CHILD")) == ["STRIDE"], (r, passes(a, "HIST_ROOT"), passes(a, "HIST_CHILD"))


def _deep(ref, z, arms, world):
    plans = ref.s.rounds + regrown(z)
    for r, a in enumerate(arms):
        assert a[ARM["XPLAN_HOST"]] == plans and a[ARM["XPLAN_DEVICE"]] == 0, (r, a[ARM["XPLAN_HOST"]], a[ARM["XPLAN_DEVICE"]])
    assert z["dist_stats"][4] > 0 and not z["piece_stats"].any(), (z["dist_stats"], z["piece_stats"])          # the leaf-owner exchange, no piece mode
    leaves = [int((t["feature"] == -1).sum()) for t in saved_run(z, ref.s.rounds)[0]]
    assert max(leaves) > 256, leaves


def _one_long_list(ref, z, arms, world):
    docs = z["shard_docs"]
    assert docs[0] == dist_shapes.LONG_LIST and docs[1:].max() < PART_TILE, docs          # rank 0 holds the long list alone; no other rank fills a partition tile
    assert world < 3 or docs.min() < 256, docs                                             # ... and of three ranks one has less than the smallest histogram chunk
    assert list(docs) == [D.shard(ref.X, ref.lab, ref.qoff, r, world)[0].shape[0] for r in range(world)]
    long_list = arms[:, ARM["RANK_HUGE"]] + arms[:, ARM["RANK_BLOCK"]]
    assert long_list[0] > 0 and (long_list[1:] == 0).all(), long_list


def _nothing(ref, z, arms, world):
    pass


# world = 3 everywhere: a case is seconds, most of them the start of the ranks
SHAPE_CASES = [("sparse", _sparse), ("runs", _runs), ("split_decision", _split_decision), ("split_crows", _split_crows), ("dead_here", _nothing), ("wide_table", _stride),
               ("wide_table_tie_off", _stride), ("wide", _nothing), ("deep", _deep), ("one_long_list", _one_long_list),
               ("one_long_list_map", _one_long_list), ("inf_and_wrapped", _nothing)]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,arms_of", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_sharded_shape_equals_the_oracle(name, arms_of, world, refs, tmp_path):
    ref = refs.get(name)
    z = launch(name, world, tmp_path)
    assert "init_refused" not in z, z["init_refused"]          # (no shape is unsupported when sharded; a refusal by rl_init would arrive here, from every rank)
    arms = ref.check(z, "%s, %d ranks" % (name, world))
    assert arms.shape[0] == world
    arms_of(ref, z, arms, world)


# ---- the child-pass knobs that tests/test_gpu_kernel_variants.py keeps alive on one GPU, in the workers' environment ----------------------------
@pytest.fixture(scope="module")
def plain_ref():
    from ranklib_amd import synth
    n, f, kind, seed, leaves, rounds = CFG
    return Reference(data=synth.make_dataset(n, f, kind, seed_offset=seed), leaves=leaves, rounds=rounds)


KNOBS = [("SUB_CHILD", "8", "SUB8"), ("SUB_CHILD", "4", "SUB4"), ("HIST_NT", "512", "NT512"), ("P8", "2", "PACKED"), ("P8", "0", "ROWS16")]


def knob_arm(r, a, knob, value, arm):
    """rank r's child passes took the named arm and no other (P8=0 names the default child arm: the setting and the root arm tell it from the default)"""
    assert list(passes(a, "HIST_CHILD")) == [arm], (r, passes(a, "HIST_CHILD"))
    if knob == "P8":
        root = passes(a, "HIST_ROOT")
        assert a[ARM["SET_P8"]] == int(value) and root and set(root) <= ({"FQ_PACKED", "PACKED"} if value == "2" else {"FQ_ROWS16", "ROWS16"}), (r, a[ARM["SET_P8"]], root)


@pytest.mark.parametrize("knob,value,arm", KNOBS, ids=["%s=%s" % k[:2] for k in KNOBS])
def test_child_pass_knobs_on_plain_data_under_sharding(knob, value, arm, plain_ref, tmp_path):
    z = launch_workers(2, 29586, str(tmp_path / "knob.npz"), CFG, "LAMBDAMART", "NDCG", 10, worker_env={"RLHIP_" + knob: value})
    for r, a in enumerate(plain_ref.check(z, "%s=%s" % (knob, value))):
        knob_arm(r, a, knob, value, arm)


@pytest.mark.parametrize("knob,value,arm", KNOBS, ids=["%s=%s" % k[:2] for k in KNOBS])
def test_child_pass_knobs_on_sparse_data_under_sharding(knob, value, arm, refs, tmp_path):
    """launch_hist takes the compact rows before it looks at any of these knobs, so on sparse data the named arm is reachable only with RLHIP_CROWS=0
    beside the knob (the "rows" mode of test_sparse_700_feature_shape_matches_the_oracle): mostly-zero columns, a quarter of them dead, through every
    dense-row child arm"""
    ref = refs.get("sparse")
    z = launch("sparse", 2, tmp_path, worker_env={"RLHIP_" + knob: value, "RLHIP_CROWS": "0"})
    for r, a in enumerate(ref.check(z, "sparse %s=%s" % (knob, value))):
        assert a[ARM["SET_CROWS"]] == 0, (r, a[ARM["SET_CROWS"]])
        knob_arm(r, a, knob, value, arm)
