"""-m gpu: every kept kernel variant of the tree trainer (the RLHIP_* knobs that select "alternatives that were built, measured and
kept") against the CPU oracle, and the default paths that only large data reaches brought down to a few thousand documents.

A knob that is silently ignored would let a case pass on the default kernel, so every case also asserts WHICH variant ran: the host counts its
launches per variant (RL_ARR_LAUNCH_ARMS, `Trainer.array("LAUNCH_ARMS")`, indices `_native.ARM` / `_native.HARM`), and what is decided on the
device -- the chunks of a growth step -- is restated here from the step log (RLHIP_STEPLOG=1, RL_ARR_STEP_LOG) and the knob values the case set.

The oracle's rounds are computed once per data set (module-scoped fixtures); a case runs the GPU trainer only.  Compared with the oracle, bit for
bit: lambdas, weights, scores, the per-round training and validation metric, the trees with their stored (feature, threshold) pairs.
"""
import os

import numpy as np
import pytest

import oracle_ffi as O
from dist_shapes import duplicate_columns as _duplicate_columns, query_level_columns as _query_level_columns
from ranklib_amd import _native as N
from ranklib_amd import synth
from tree_equiv import assert_equivalent

pytestmark = pytest.mark.gpu

ARM, HARM = N.ARM, N.HARM
THREADS = min(16, os.cpu_count() or 8)
ROW_LDS = 16 * 264 * 12          # dynamic LDS of a 16-feature child-pass block: int64 sums + int32 counts over the 264-bin row stride


def bits(a, kind):
    return np.ascontiguousarray(a).view(kind)


def same_f32(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- data sets ------------------------------------------------------------------------------------------------------------------------------
# _duplicate_columns: two columns repeat two others (one rescaled: other thresholds, the same cuts): exact ties over several features, so the lazy
# tie-break stalls or defers and re-enters the growth bookkeeping.  _query_level_columns: five columns with one value per query (as
# test_query_level_columns_take_the_quad_folded_histogram_path): rl_init flags them, any_runs holds.  Both live in tests/dist_shapes.py, whose shape
# `runs` is set B below for the sharded cases of tests/test_gpu_dist_shapes.py


def _oracle_rounds(X, lab, qoff, valid, rounds, leaves, metric="NDCG", k=10, per_query=False):
    o = O.Oracle(X, lab, qoff, n_trees=rounds, n_leaves=leaves, metric=metric, k=k, n_threads=THREADS)
    if valid is not None:
        o.set_validation(*valid)
    o.init()
    out = []
    for _ in range(rounds):
        t, tm, vm, _ = o.round()
        rec = dict(tree=t, tm=tm, vm=vm, lam=o.lambdas(), w=o.weights(), score=o.scores())
        if per_query:
            rec["per_query"] = np.array([O.query_score(metric, rec["score"][a:b], lab[a:b], k) for a, b in zip(qoff[:-1], qoff[1:])])
        for v in rec.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(rec)
    return out


class DataSet:
    def __init__(self, X, lab, qoff, valid, rounds, leaves):
        self.X, self.lab, self.qoff, self.valid, self.rounds, self.leaves = X, lab, qoff, valid, rounds, leaves
        self.N = X.shape[0]
        self.oracle = _oracle_rounds(X, lab, qoff, valid, rounds, leaves)


@pytest.fixture(scope="module")
def set_a():
    """12 000 x 24, a 1 500-document validation set, two duplicated columns; 4 rounds of 20 leaves"""
    X, lab, qoff = synth.make_dataset(12000, 24, "mslr", seed_offset=61)
    Xv, lv, qv = synth.make_dataset(1500, 24, "mslr", seed_offset=62)
    return DataSet(_duplicate_columns(X), lab, qoff, (_duplicate_columns(Xv), lv, qv), 4, 20)


@pytest.fixture(scope="module")
def set_b():
    """set A plus five query-level columns"""
    X, lab, qoff = synth.make_dataset(12000, 24, "mslr", seed_offset=61)
    Xv, lv, qv = synth.make_dataset(1500, 24, "mslr", seed_offset=62)
    return DataSet(_query_level_columns(_duplicate_columns(X), qoff, 5), lab, qoff, (_query_level_columns(_duplicate_columns(Xv), qv, 6), lv, qv), 4, 20)


# ---- one GPU run against the recorded oracle -------------------------------------------------------------------------------------------------
def run_gpu(ds, monkeypatch, env, flags=0, ties_allowed=False, steplog=False):
    """the GPU trainer under `env`, compared round by round with ds.oracle; returns (launch arms, step log, per-round records)"""
    for k, v in env.items():
        monkeypatch.setenv("RLHIP_" + k, str(v))
    if steplog:
        monkeypatch.setenv("RLHIP_STEPLOG", "1")
    g = N.Trainer(n_trees=ds.rounds, n_leaves=ds.leaves, flags=flags)
    g.set_train(ds.X, ds.lab, ds.qoff)
    if ds.valid is not None:
        g.set_validation(*ds.valid)
    g.init()
    recs = []
    for r, ref in enumerate(ds.oracle):
        tg, tm, vm, _ = g.boost_round()
        ctx = "%s round %d" % (env, r)
        assert np.array_equal(bits(g.array("LAMBDA"), np.int64), bits(ref["lam"], np.int64)), ctx
        assert np.array_equal(bits(g.array("WEIGHT"), np.int64), bits(ref["w"], np.int64)), ctx
        ties = assert_equivalent(ref["tree"], tg, ds.X, ctx)
        assert ties_allowed or ties == 0, "%d split(s) store another (feature, threshold) than the oracle's (%s)" % (ties, ctx)
        score = g.array("SCORE")
        assert np.array_equal(bits(score, np.int64), bits(ref["score"], np.int64)), ctx
        assert same_f32(tm, ref["tm"]), ctx
        if ds.valid is not None:
            assert same_f32(vm, ref["vm"]), ctx
        recs.append(dict(tree=tg.trimmed(), score=score, tm=tm, vm=vm))
    arms = g.array("LAUNCH_ARMS")
    log = g.array("STEP_LOG") if steplog else None
    tie_stats = g.array("TIE_STATS")
    g.close()
    return arms, log, recs, tie_stats


def child(arms, name):
    return int(arms[ARM["HIST_CHILD"] + HARM[name]])


def root(arms, name):
    return int(arms[ARM["HIST_ROOT"] + HARM[name]])


def only(arms, base, name):
    """the named k_hist arm was launched, and no other arm of the same pass: the arm replaces the default outright"""
    got = {k: int(arms[ARM[base] + v]) for k, v in HARM.items() if k != "COUNT_" and arms[ARM[base] + v]}
    assert list(got) == [name], (base, name, got)


def root_only(arms, name, ds, regrown, again):
    """the root pass of every round took the named arm; a tree grown a second time (RL_ARR_TIE_STATS[9]) reads the q the first pass stored, so its
    root pass is the arm `again`, which does not quantise"""
    got = {k: int(arms[ARM["HIST_ROOT"] + v]) for k, v in HARM.items() if k != "COUNT_" and arms[ARM["HIST_ROOT"] + v]}
    want = {name: ds.rounds}
    if regrown:
        want[again] = want.get(again, 0) + regrown
    assert got == want, (name, got, want)


# ---- the step log and the device's chunk rules, restated --------------------------------------------------------------------------------------
def growth_steps(log):
    """[(tree, step, [documents of the accumulated child, by slot])] from RL_ARR_STEP_LOG's growth-step entries"""
    n = int(log[0])
    assert 0 < n <= 8192, "the step log is empty or has overflowed: %d entries" % n
    e = log[8:8 + 8 * n].reshape(n, 8)
    e = e[e[:, 1] == 0]
    steps = {}
    for tree, _, step, slot, _, cnt, _, nsel in e:
        steps.setdefault((int(tree), int(step)), {})[int(slot)] = (int(cnt), int(nsel))
    out = []
    for (tree, step), slots in sorted(steps.items()):
        assert sorted(slots) == list(range(len(slots))) and all(ns == len(slots) for _, ns in slots.values()), (tree, step, slots)
        out.append((tree, step, [slots[j][0] for j in range(len(slots))]))
    return out


def without_last_steps(steps):
    """the split that fills a tree's leaf budget accumulates no child (RLHIP_SKIP_LAST, the default) and the log does not say which step that was:
    the last logged step of every tree is left out of what the cases below conclude"""
    last = {}
    for tree, step, _ in steps:
        last[tree] = max(last.get(tree, -1), step)
    return [s for s in steps if s[1] != last[s[0]]]


def root_steps(recs):
    """the step that accumulates the smaller child of a tree's root is the root finish's own and writes no log entry: its one slot, from the
    trees the trainer returned (one per round; nodes in pre-order, the root's left child is node 1)"""
    out = []
    for rec in recs:
        t = rec["tree"]
        out.append((None, 0, [int(min(t["count"][int(t["left"][0])], t["count"][int(t["right"][0])]))]))
    return out


def up256(v):
    return (v + 255) & ~255


def chunk_docs(cnt, node_div, node_min, node_chunk):
    """chunk_docs<false> (rl_k_hist.inc): documents per histogram chunk of a child node of cnt documents"""
    return min(node_chunk, max(max(node_min, 256), up256((cnt + node_div - 1) // node_div)))


def node_chunks(cnt, node_div, node_min, node_chunk):
    cs = chunk_docs(cnt, node_div, node_min, node_chunk)
    return 0 if cnt <= 0 else (cnt + cs - 1) // cs


def balance_slots(cnts, node_div, node_min, node_chunk, target, bmin, cap, max_chunks):
    """balance_slots (rl_k_select.inc): None when the step keeps chunk_docs' rule, else (k, chunk size, chunks of the step)"""
    legacy = sum(node_chunks(c, node_div, node_min, node_chunk) for c in cnts)
    D = sum(cnts)
    if legacy <= bmin:
        return None
    k = -(-D // (target * cap))
    want = k * target
    cs = up256(-(-D // want))
    while True:
        cs = min(cs, cap)
        tot = sum((c + cs - 1) // cs for c in cnts)
        if tot <= want or cs >= cap:
            break
        cs += 256
    tot = sum((c + cs - 1) // cs for c in cnts)
    return None if tot > max_chunks else (k, cs, tot)


def node_chunk_of(n_docs, n_feat):
    return 4096 if n_docs <= (2 << 20) and n_feat <= 256 else 8192        # rl_init.inc init_shape


# ---- growth-step variants on set A -------------------------------------------------------------------------------------------------------------
def _a_default(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16"); root_only(arms, "FQ_PACKED", ds, regrown, "PACKED")
    assert arms[ARM["QUANTIZE"]] == 0 and arms[ARM["CHILD_LDS"]] == ROW_LDS and arms[ARM["CHILD_GRID_X"]] == 2
    assert (arms[ARM["SET_P8"]], arms[ARM["SET_DM_ROOT"]], arms[ARM["SET_DM_DIV"]], arms[ARM["SET_STEP_AHEAD"]], arms[ARM["SET_BALANCE"]]) == (1, 0, 1, 1, 1)
    assert arms[ARM["SET_TIE_ON"]] != 0 and arms[ARM["SET_NODE_MIN"]] == 256 and arms[ARM["SET_NODE_CHUNK"]] == node_chunk_of(ds.N, 24)


def _a_sub_child(sub):
    def check(arms, steps, ds, regrown):
        only(arms, "HIST_CHILD", "SUB%d" % sub)
        # a group's 16 features over 16 / sub blocks: the grid is that many times as wide, and a block's LDS holds `sub` rows
        assert arms[ARM["CHILD_GRID_X"]] == 2 * (16 // sub) and arms[ARM["CHILD_LDS"]] == sub * 264 * 12
    return check


def _a_hist_nt(arm):
    def check(arms, steps, ds, regrown):
        only(arms, "HIST_CHILD", arm)
        assert arms[ARM["CHILD_GRID_X"]] == 2 and arms[ARM["CHILD_LDS"]] == ROW_LDS
    return check


def _a_ldspad(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["CHILD_LDS"]] == ROW_LDS + 28672


def _a_p8_0(arms, steps, ds, regrown):
    root_only(arms, "FQ_ROWS16", ds, regrown, "ROWS16"); only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_P8"]] == 0


def _a_p8_2(arms, steps, ds, regrown):
    root_only(arms, "FQ_PACKED", ds, regrown, "PACKED"); only(arms, "HIST_CHILD", "PACKED")
    assert arms[ARM["SET_P8"]] == 2


def _a_dm_root(arms, steps, ds, regrown):
    root_only(arms, "FQ_PACKED", ds, regrown, "PACKED")
    assert arms[ARM["SET_DM_ROOT"]] == 1


def _a_dm_div_0(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_DM_DIV"]] == 0          # k_hist: dm = dm_div > 0 && ... -- group-major rows for every child


def _a_dm_div_4(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_DM_DIV"]] == 4
    # k_hist takes document-major rows for a child of cnt documents when cnt * dm_div <= N: both kinds inside one tree
    for tree in sorted({s[0] for s in steps}):
        cnts = [c for t, _, slots in steps if t == tree for c in slots]
        if any(c * 4 <= ds.N for c in cnts) and any(c * 4 > ds.N for c in cnts):
            return
    raise AssertionError("no tree accumulated children on both sides of N / 4: %s" % steps)


def _a_fused_quant_0(arms, steps, ds, regrown):
    root_only(arms, "PACKED", ds, regrown, "PACKED"); only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["QUANTIZE"]] == ds.rounds          # k_quantize once a round (a regrown tree keeps the first pass's q)


def _a_node_div_1(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_NODE_DIV"]] == 1
    nc = node_chunk_of(ds.N, 24)
    # one chunk holds what the default rule (24 chunks a node) cuts into several
    assert any(256 < c <= nc and node_chunks(c, 1, 256, nc) == 1 and node_chunks(c, 24, 256, nc) > 1 for _, _, slots in steps for c in slots)


def _a_node_div_64_grid_8(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_NODE_DIV"]] == 64 and arms[ARM["CHILD_GRID_Y"]] == 8
    nc = node_chunk_of(ds.N, 24)
    per_step = [sum(node_chunks(c, 64, 256, nc) for c in slots) for _, _, slots in without_last_steps(steps)]
    # (no step is re-cut: a step has far fewer chunks than the default balance_min of 128 at two feature groups)
    assert max(per_step) <= int(arms[ARM["SET_BALANCE_MIN"]])
    assert max(per_step) > 8, "no step had more chunks than the grid has rows: no block walked two chunks (%s)" % per_step


def _a_node_min(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_NODE_MIN"]] == 1024
    nc = node_chunk_of(ds.N, 24)
    assert any(node_chunks(c, 24, 1024, nc) < node_chunks(c, 24, 256, nc) for _, _, slots in steps for c in slots)


def _a_balance_0(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_BALANCE"]] == 0


def _a_step_ahead_3(arms, steps, ds, regrown):
    only(arms, "HIST_CHILD", "ROWS16")
    assert arms[ARM["SET_STEP_AHEAD"]] == 3
    assert arms[ARM["STEPS_ENQUEUED"]] >= len(steps)          # every step that ran was enqueued; up to three empty ones behind a finished tree


CASES_A = [
    ("default", {}, _a_default),
    ("SUB_CHILD=8", {"SUB_CHILD": 8}, _a_sub_child(8)),
    ("SUB_CHILD=4", {"SUB_CHILD": 4}, _a_sub_child(4)),
    ("HIST_NT=512", {"HIST_NT": 512}, _a_hist_nt("NT512")),
    ("HIST_NT=1024", {"HIST_NT": 1024}, _a_hist_nt("NT1024")),
    ("HIST_LDSPAD=28672", {"HIST_LDSPAD": 28672}, _a_ldspad),
    ("P8=0", {"P8": 0}, _a_p8_0),
    ("P8=2", {"P8": 2}, _a_p8_2),
    ("DM_ROOT=1", {"DM_ROOT": 1}, _a_dm_root),
    ("DM_DIV=0", {"DM_DIV": 0}, _a_dm_div_0),
    ("DM_DIV=4", {"DM_DIV": 4}, _a_dm_div_4),
    ("FUSED_QUANT=0", {"FUSED_QUANT": 0}, _a_fused_quant_0),
    ("NODE_DIV=1", {"NODE_DIV": 1}, _a_node_div_1),
    ("NODE_DIV=64,HIST_GRID=8", {"NODE_DIV": 64, "HIST_GRID": 8}, _a_node_div_64_grid_8),
    ("NODE_MIN=1024", {"NODE_MIN": 1024}, _a_node_min),
    ("BALANCE=0", {"BALANCE": 0}, _a_balance_0),
    ("STEP_AHEAD=3", {"STEP_AHEAD": 3}, _a_step_ahead_3),
]


@pytest.mark.parametrize("name,env,check", CASES_A, ids=[c[0] for c in CASES_A])
def test_growth_step_variants_on_set_a(name, env, check, set_a, monkeypatch):
    arms, log, _, tie_stats = run_gpu(set_a, monkeypatch, env, steplog=True)
    steps = growth_steps(log)
    assert len({s[0] for s in steps}) >= set_a.rounds, steps
    assert tie_stats[0] > 0, "the duplicated columns never tied: the lazy tie-break did not re-enter the bookkeeping"
    regrown = int(tie_stats[9])
    assert sum(root(arms, k) for k in HARM if k != "COUNT_") == set_a.rounds + regrown
    check(arms, steps, set_a, regrown)


# ---- set B: query-level columns, the RUNS instantiations ----------------------------------------------------------------------------------------
def _b_default(arms, ds):
    only(arms, "HIST_ROOT", "PACKED_RUNS"); only(arms, "HIST_CHILD", "ROWS16_RUNS")


def _b_p8_0(arms, ds):
    only(arms, "HIST_ROOT", "ROWS16_RUNS"); only(arms, "HIST_CHILD", "ROWS16_RUNS")
    assert arms[ARM["SET_P8"]] == 0


def _b_p8_2(arms, ds):
    only(arms, "HIST_ROOT", "PACKED_RUNS"); only(arms, "HIST_CHILD", "PACKED_RUNS")
    assert arms[ARM["SET_P8"]] == 2


def _b_sub_child_8(arms, ds):
    # the 8-feature blocks have no instantiation that folds runs: the knob is read (SET_SUB_CHILD) and must be ignored
    assert arms[ARM["SET_SUB_CHILD"]] == 8 and child(arms, "SUB8") == 0
    only(arms, "HIST_CHILD", "ROWS16_RUNS")
    assert arms[ARM["CHILD_GRID_X"]] == 2 and arms[ARM["CHILD_LDS"]] == ROW_LDS


CASES_B = [("default", {}, _b_default), ("P8=0", {"P8": 0}, _b_p8_0), ("P8=2", {"P8": 2}, _b_p8_2), ("SUB_CHILD=8", {"SUB_CHILD": 8}, _b_sub_child_8)]


@pytest.mark.parametrize("name,env,check", CASES_B, ids=[c[0] for c in CASES_B])
def test_growth_step_variants_with_columns_in_runs(name, env, check, set_b, monkeypatch):
    arms, _, _, _ = run_gpu(set_b, monkeypatch, env)
    assert arms[ARM["SET_ANY_RUNS"]] == 1
    assert arms[ARM["QUANTIZE"]] == set_b.rounds          # (the root pass of the RUNS instantiation does not quantise)
    check(arms, set_b)


def test_tie_off_keeps_the_first_candidate_as_first_tie_does(set_a, monkeypatch):
    """RLHIP_TIE_OFF: no lazy tie-break, the first candidate of an exact tie in scan order.  The oracle's trees up to such ties (assert_equivalent),
    everything else bit for bit; and bit for bit -- stored (feature, threshold) pairs included -- the run that asks for the same with RL_FLAG_FIRST_TIE"""
    arms_f, _, flag, ts_f = run_gpu(set_a, monkeypatch, {}, flags=N.RL_FLAG_FIRST_TIE, ties_allowed=True)
    arms_e, _, env, ts_e = run_gpu(set_a, monkeypatch, {"TIE_OFF": 1}, ties_allowed=True)
    assert arms_e[ARM["SET_TIE_ON"]] == 0 and arms_f[ARM["SET_TIE_ON"]] == 0
    assert not ts_e[:4].any() and not ts_f[:4].any(), (ts_e, ts_f)
    for a, b in zip(flag, env):
        for key in ("feature", "left", "right", "count"):
            assert np.array_equal(a["tree"][key], b["tree"][key]), key
        assert np.array_equal(bits(a["tree"]["threshold"], np.uint32), bits(b["tree"]["threshold"], np.uint32))
        assert np.array_equal(bits(a["tree"]["output"], np.uint32), bits(b["tree"]["output"], np.uint32))
        assert np.array_equal(bits(a["tree"]["deviance"], np.int64), bits(b["tree"]["deviance"], np.int64))


# ---- balanced chunks ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def set_balanced():
    X, lab, qoff = synth.make_dataset(30000, 24, "mslr", seed_offset=63)
    return DataSet(X, lab, qoff, None, 3, 31)


def test_balanced_chunks_forced_down_to_small_steps(set_balanced, monkeypatch):
    """balance_slots re-cuts a step of more than balance_min chunks into k x balance_target chunks of one size.  By default that takes steps of more
    than 128 chunks at 24 features (28 at 136): RLHIP_BALANCE_TARGET=8, _MIN=1, _CAP=1024 bring it to 30 000 documents.  The step log says what every
    step accumulated; which steps were re-cut, and how, is restated from the knob values set here.  (The chunk size the device chose is not in the
    log: every consumer reads it from the slot, so a size that is merely not the restated one changes no sum and is not seen here.  What the case
    holds is that trees, scores and metrics stay the oracle's when steps of one and of several slots are re-cut.)"""
    ds = set_balanced
    knobs = dict(BALANCE_TARGET=8, BALANCE_MIN=1, BALANCE_CAP=1024, NODE_DIV=24)
    arms, log, recs, _ = run_gpu(ds, monkeypatch, knobs, steplog=True)
    only(arms, "HIST_CHILD", "ROWS16")
    assert (arms[ARM["SET_BALANCE"]], arms[ARM["SET_BALANCE_TARGET"]], arms[ARM["SET_BALANCE_MIN"]], arms[ARM["SET_BALANCE_CAP"]], arms[ARM["SET_NODE_DIV"]]) == (1, 8, 1, 1024, 24)
    assert arms[ARM["CHILD_GRID_Y"]] == 8          # exactly balance_target rows of blocks: row r works through the chunks r, r + 8, ..
    nc, maxc = node_chunk_of(ds.N, 24), int(arms[ARM["SET_MAX_CHUNKS"]])
    assert nc == arms[ARM["SET_NODE_CHUNK"]]
    cut = [(slots, balance_slots(slots, 24, 256, nc, 8, 1, 1024, maxc)) for _, _, slots in root_steps(recs) + without_last_steps(growth_steps(log))]
    recut = [(slots, b) for slots, b in cut if b is not None]
    print("\n[balanced, forced] steps %d, re-cut %d; (slots, (k, chunk, chunks)): %s" % (len(cut), len(recut), recut[:12]))
    assert any(b[0] >= 2 and sum(slots) > 8 * 1024 for slots, b in recut), "no re-cut step of k >= 2 rounds of chunks"
    assert any(len(slots) >= 2 for slots, b in recut), "no re-cut step of two or more slots"
    assert any(b is None for _, b in cut), "no step was left alone"
    assert all(b[2] <= b[0] * 8 or b[1] == 1024 for _, b in recut)


@pytest.fixture(scope="module")
def set_balanced_default():
    X, lab, qoff = synth.make_dataset(BALANCED_DEFAULT_DOCS, 136, "mslr", seed_offset=64)
    return DataSet(X, lab, qoff, None, 2, 31)


BALANCED_DEFAULT_DOCS = 40000


def test_balanced_chunks_with_the_default_knobs_at_136_features(set_balanced_default, monkeypatch):
    """the default rule at the benchmark's width: 9 feature groups, balance_target 56, steps of more than 28 chunks are re-cut.  A node is cut into
    at most 24 chunks, so it takes a step of two or more nodes.  40 000 documents, the first size tried: five of its 24 logged steps have 30 to 43
    chunks and are re-cut, and a case takes a fraction of a second, so it was not shrunk further"""
    ds = set_balanced_default
    arms, log, recs, _ = run_gpu(ds, monkeypatch, {"NODE_DIV": 24}, steplog=True)
    only(arms, "HIST_CHILD", "ROWS16")
    assert (arms[ARM["SET_BALANCE"]], arms[ARM["SET_BALANCE_TARGET"]], arms[ARM["SET_BALANCE_MIN"]], arms[ARM["SET_BALANCE_CAP"]]) == (1, 56, 28, 16384)
    nc, maxc = node_chunk_of(ds.N, 136), int(arms[ARM["SET_MAX_CHUNKS"]])
    cut = [(slots, balance_slots(slots, 24, 256, nc, 56, 28, 16384, maxc)) for _, _, slots in root_steps(recs) + without_last_steps(growth_steps(log))]
    recut = [(slots, b) for slots, b in cut if b is not None]
    print("\n[balanced, default] steps %d, re-cut %d: %s" % (len(cut), len(recut), recut[:12]))
    assert recut and all(len(slots) >= 2 for slots, _ in recut), "no step above 28 chunks"
    assert any(b is None for _, b in cut)


# ---- lambdas and ranking --------------------------------------------------------------------------------------------------------------------------
class ListData:
    """the mixed list lengths of test_fused_lambda_kernel_of_every_metric_on_mixed_list_lengths (1 .. 700 documents, the kernels' boundary lengths, a
    list without a relevant document, a list of equal labels) and one list just above the block kernel's cap of 5000, for k_rank_huge"""
    ROUNDS = 3

    def __init__(self):
        rng = np.random.default_rng(50)
        k = 10
        sizes = np.concatenate([rng.integers(1, 17, 200), rng.integers(17, 65, 60), rng.integers(65, 129, 30), rng.integers(129, 193, 12),
                                rng.integers(193, 300, 8), [k, k + 1, k + 2, 5, 6, 16, 17, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 700, 5001]])
        rng.shuffle(sizes)
        self.qoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        n = int(self.qoff[-1])
        self.X = rng.random((n, 6)).astype(np.float32)
        self.lab = np.floor(3 * self.X[:, 0] * self.X[:, 1] + 2 * rng.random(n)).astype(np.float32)
        self.lab[self.qoff[5]:self.qoff[6]] = 0
        self.lab[self.qoff[7]:self.qoff[8]] = 2
        self.sizes = sizes
        self._oracle = {}

    def oracle(self, metric, k):
        if (metric, k) not in self._oracle:
            self._oracle[(metric, k)] = _oracle_rounds(self.X, self.lab, self.qoff, None, self.ROUNDS, 6, metric=metric, k=k, per_query=True)
        return self._oracle[(metric, k)]


@pytest.fixture(scope="module")
def lists():
    return ListData()


def _fused(arms):
    return {k: int(arms[ARM[k]]) for k in ("LAM_TINY", "LAM_FUSED", "LAM_COMPACT", "LAM_ERR", "LAM_MAP", "LAM_UNFUSED", "LAM_MART") if arms[ARM[k]]}


def _rank(arms):
    return {k: int(arms[ARM[k]]) for k in ("RANK_TINY", "RANK_MIXED", "RANK_WAVE_LONG", "RANK_WAVE_SHORT", "RANK_BLOCK", "RANK_HUGE") if arms[ARM[k]]}


R = ListData.ROUNDS
# four length classes hold lists (the few lists of at most 16 documents join the 64-wide class unless RLHIP_TINY_MIN lets them have their own kernels):
# four fused launches a round, `side` of them on side streams.  launch_rank runs once in rl_init and once a round.
CASES_L = [
    ("default", {}, "NDCG", 10, lambda a: (_rank(a) == {"RANK_MIXED": R + 1, "RANK_HUGE": R + 1} and _fused(a) == {"LAM_FUSED": 4 * R}
                                         and a[ARM["LAM_ON_SIDE"]] == R and a[ARM["LAM_ON_MAIN"]] == 3 * R)),
    ("RANK_SPLIT", {"RANK_SPLIT": 1}, "NDCG", 10, lambda a: _rank(a) == {"RANK_WAVE_SHORT": R + 1, "RANK_BLOCK": R + 1, "RANK_HUGE": R + 1}),
    ("RANK_SPLIT,TINY_MIN=1", {"RANK_SPLIT": 1, "TINY_MIN": 1}, "NDCG", 10,
     lambda a: (_rank(a) == {"RANK_TINY": R + 1, "RANK_WAVE_SHORT": R + 1, "RANK_BLOCK": R + 1, "RANK_HUGE": R + 1} and _fused(a) == {"LAM_TINY": R, "LAM_FUSED": 4 * R})),
    ("LAMBDA_SIDE=0", {"LAMBDA_SIDE": 0}, "NDCG", 10, lambda a: a[ARM["LAM_ON_SIDE"]] == 0 and a[ARM["LAM_ON_MAIN"]] == 4 * R),
    ("LAMBDA_SIDE=2", {"LAMBDA_SIDE": 2}, "NDCG", 10, lambda a: a[ARM["LAM_ON_SIDE"]] == 2 * R and a[ARM["LAM_ON_MAIN"]] == 2 * R),
    ("LAMBDA_SIDE=3", {"LAMBDA_SIDE": 3}, "NDCG", 10, lambda a: a[ARM["LAM_ON_SIDE"]] == 3 * R and a[ARM["LAM_ON_MAIN"]] == R),
    ("LAMBDA_COMPACT,NDCG@10", {"LAMBDA_COMPACT": 1}, "NDCG", 10, lambda a: _fused(a) == {"LAM_COMPACT": 4 * R}),
    ("LAMBDA_COMPACT,DCG@5", {"LAMBDA_COMPACT": 1}, "DCG", 5, lambda a: _fused(a) == {"LAM_COMPACT": 4 * R}),
    ("LAMBDA_COMPACT,ERR@10", {"LAMBDA_COMPACT": 1}, "ERR", 10, lambda a: _fused(a) == {"LAM_ERR": 4 * R}),          # the lists of active pairs are NDCG's and DCG's: nothing may change
]


@pytest.mark.parametrize("name,env,metric,k,check", CASES_L, ids=[c[0] for c in CASES_L])
def test_lambda_and_ranking_variants_on_mixed_list_lengths(name, env, metric, k, check, lists, monkeypatch):
    for kk, v in env.items():
        monkeypatch.setenv("RLHIP_" + kk, str(v))
    g = N.Trainer(n_trees=R, n_leaves=6, metric=metric, metric_k=k)
    g.set_train(lists.X, lists.lab, lists.qoff)
    g.init()
    for r, ref in enumerate(lists.oracle(metric, k)):
        _, tm, _, _ = g.boost_round()
        ctx = "%s round %d" % (name, r)
        assert np.array_equal(bits(g.array("LAMBDA"), np.int64), bits(ref["lam"], np.int64)), ctx
        assert np.array_equal(bits(g.array("WEIGHT"), np.int64), bits(ref["w"], np.int64)), ctx
        assert np.array_equal(bits(g.array("SCORE"), np.int64), bits(ref["score"], np.int64)), ctx
        assert np.array_equal(bits(g.array("NDCG_PER_QUERY"), np.int64), bits(ref["per_query"], np.int64)), ctx
        assert same_f32(tm, ref["tm"]), ctx
    arms = g.array("LAUNCH_ARMS")
    g.close()
    assert check(arms), (name, _rank(arms), _fused(arms), int(arms[ARM["LAM_ON_SIDE"]]), int(arms[ARM["LAM_ON_MAIN"]]))
