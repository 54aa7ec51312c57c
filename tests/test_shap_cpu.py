"""Exact TreeSHAP contributions without a GPU: the computed form of tests/shap_restatement.py in exact arithmetic against
Shapley values enumerated from the definition, its f64 run against its own exact run, hand cases, the properties the definitions imply,
the host side of librlhip.so (rl_shap_host.h) through tools/shap_host_check.cpp, the exported symbols and the command line's flag."""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import contrib_restatement as CR
import shap_restatement as SR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, BOUND = SR.U, SR.BOUND                        # (b): 8 x the worst gap measured here, which shap_restatement.py records


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bit1(x):
    return int(np.float64(x).view(np.uint64))


@pytest.fixture(autouse=True)
def _restore_statics():
    """the command line writes the evaluator's statics, as every command line here does"""
    from ranklib_amd.evaluator import Evaluator
    saved = (Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile)
    yield
    Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile = saved


# ---- the small random models of (a) and (b) -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_models():
    """100 models of 3 random trees over the features 1 .. 6, up to 9 leaves (depth <= 8), with backgrounds of 0, 1, 3 and 12 rows (so
    nodes the background never reached, and reached nodes with an empty child, are common) and 5 rows of width 6: NaN and +-Infinity
    cells, and feature 6 beyond row_stride"""
    rng = np.random.default_rng(27)
    g = TM.Gen(rng, features=range(1, 7))
    out = []
    for k in range(100):
        trees = [TM.random_tree(g, int(rng.integers(1, 10))) for _ in range(3)]
        w = TM.WEIGHTS[rng.integers(0, len(TM.WEIGHTS), 3)]
        bg = CR.grid_rows(rng, (0, 1, 3, 12)[k % 4], 7, special=0.1)
        rows = CR.grid_rows(rng, 5, 6, special=0.25)
        feats = CR.model_features(trees)
        cols = feats if k % 2 == 0 else [9] + feats[::2]
        out.append((trees, w, CR.covers(trees, bg), rows, cols))
    return out


@functools.lru_cache(maxsize=None)
def small_exact():
    return [SR.shap(t, w, cov, rows, cols, SR.frac) for t, w, cov, rows, cols in small_models()]


def test_the_small_models_hold_what_they_are_for():
    repeated = empty = one_side = deep = special = 0
    for trees, w, cov, rows, cols in small_models():
        special += int(np.isnan(rows).any()) + int(np.isinf(rows).any())
        for t, c in zip(trees, cov):
            assert TM.depth_of(t) <= 8 and len(CR.model_features([t])) <= 6
            deep += TM.depth_of(t) >= 5
            for leaf, els in SR.leaf_elements(t, c, SR.f64):
                repeated += any(len(e[2]) > 1 for e in els)
            for j in range(len(t["feature"])):
                if t["feature"][j] != -1:
                    a, b = int(c[t["left"][j]]), int(c[t["right"][j]])
                    empty += a + b == 0
                    one_side += (a == 0) != (b == 0)
        assert any(f >= rows.shape[1] for f in CR.model_features(trees)) or max(CR.model_features(trees), default=0) < 6
    assert min(repeated, empty, one_side, deep, special) > 20
    assert sum(6 in CR.model_features(m[0]) for m in small_models()) > 50       # a column beyond row_stride


# ---- (a) the algorithm is the definition --------------------------------------------------------------------------------------------------
def test_the_computed_form_in_exact_arithmetic_is_the_shapley_value():
    for k, ((trees, w, cov, rows, cols), got) in enumerate(zip(small_models(), small_exact())):
        want = SR.brute(trees, w, cov, rows, cols)
        assert got.shape == want.shape == (5, len(cols) + 2)
        assert (got == want).all(), (k, np.argwhere(got != want)[0])                # Fractions: no tolerance


# ---- (b) the f64 restatement is accurate --------------------------------------------------------------------------------------------------
def gap_of(trees, w, cov, rows, cols, exact=None):
    """the gap of a row is the sum over its slots of |f64 - exact| (so that it bounds every slot's error AND, by the triangle
    inequality, how far the f64 slots' sum can be from the exact one: local accuracy is held to the same bound); the worst row's, over
    sum over trees of sum over leaves of |W out|, in units of 2^-52; and the pieces"""
    mag = []
    got = SR.shap(trees, w, cov, rows, cols, SR.f64, abs_leaf=mag)
    if exact is None:
        exact = SR.shap(trees, w, cov, rows, cols, SR.frac)
    assert np.isfinite(got).all()
    gap = max((sum(abs(Fraction(float(g)) - e) for g, e in zip(gr, er)) for gr, er in zip(got, exact)), default=Fraction(0))
    total = sum(mag)
    return (float(gap) / total / U if total else float(gap)), got, exact, total


def finite_trees(name):
    c = TM.case(name)[0]
    keep = [i for i, t in enumerate(c.trees) if np.isfinite(t["output"]).all()]
    return [c.trees[i] for i in keep], c.weights[keep], c.rows


@functools.lru_cache(maxsize=None)
def named_case(name):
    """trees, weights, covers of a 150-row grid background, 12 rows, the model's features"""
    if name in ("chain_left", "chain_right"):
        trees, w = CR.chain_model(name[6:], seed=5 if name == "chain_left" else 6)
        rows, width = CR.grid_rows(np.random.default_rng(2), 12), 13
    elif name == "distinct_30":
        # a row that agrees with the chain down to some level and then leaves it cancels the most in the unwind: one that goes left
        # everywhere, one that leaves at the root, and of the 257 grid rows tests/test_gpu_shap.py walks (the same generator calls,
        # background included) the first row of each of the ten longest walk lengths
        trees, w = SR.distinct_chain(30)
        rows, width = CR.grid_rows(np.random.default_rng(42), 257, 35), 35
        first = {}
        for i, r in enumerate(rows):
            first.setdefault(len(CR.walk(trees[0], r)), i)
        rows = np.concatenate([np.full((1, 35), -2.0, np.float32), np.full((1, 35), 2.0, np.float32), rows[[first[k] for k in sorted(first)[-10:]]]])
    else:
        trees, w, rows = finite_trees(name)
        rows, width = rows[:12], rows.shape[1]
    bg = CR.grid_rows(np.random.default_rng(41), 5000, width) if name == "distinct_30" else CR.grid_rows(np.random.default_rng(3), 150, width)
    return trees, w, CR.covers_np(trees, bg), rows, CR.model_features(trees)


NAMED = ["count_37", "nodes_81", "nan_leaf", "chain_left", "chain_right", "distinct_30"]


@functools.lru_cache(maxsize=None)
def named_gap(name):
    return gap_of(*named_case(name))


def test_the_f64_run_is_close_to_its_exact_run_on_the_small_models():
    worst = 0.0
    for m, exact in zip(small_models(), small_exact()):
        worst = max(worst, gap_of(*m, exact=exact)[0])
    print("small models: worst gap %.3f x 2^-52 x sum |W out|" % worst)
    assert worst * U <= BOUND


@pytest.mark.parametrize("name", NAMED)
def test_the_f64_run_is_close_to_its_exact_run(name):
    trees, w, cov, rows, feats = named_case(name)
    if name == "distinct_30":
        assert SR.max_path(trees) == 30 and all(int(c) > 0 for c in cov[0])         # no z is 0: every leaf's unwind cancels for real
    if name == "nan_leaf":
        assert len(trees) == 32
    gap = named_gap(name)[0]
    print("%s: worst gap %.3f x 2^-52 x sum |W out|" % (name, gap))
    assert gap * U <= BOUND


# ---- (c) hand cases -----------------------------------------------------------------------------------------------------------------------
def test_the_hand_derived_stump():
    trees, w, bg = CR.hand_stump()
    cov = CR.covers(trees, bg)
    rows = np.array([[0, -3.0], [0, 0.0], [0, 7.0], [0, np.nan]], np.float32)
    want = np.array([[-0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 0.0, 0.0]])      # feature 1, rest, bias: z is 3/4 or 1/4
    assert bits(SR.shap(trees, w, cov, rows, [1])).tolist() == bits(want).tolist()


def test_the_and_tree_credits_both_features_alike_where_saabas_does_not():
    trees, w, bg = SR.and_tree()
    cov = CR.covers(trees, bg)
    assert cov[0].tolist() == [4, 2, 2, 1, 1]
    rows = np.array([[0, 1.0, 1.0]], np.float32)
    got = SR.shap(trees, w, cov, rows, [1, 2])
    assert abs(got[0, 0] - 0.375) <= 1e-15 and abs(got[0, 1] - 0.375) <= 1e-15 and got[0, 2] == 0.0 and got[0, 3] == 0.25
    assert SR.shap(trees, w, cov, rows, [1, 2], SR.frac)[0].tolist() == [Fraction(3, 8), Fraction(3, 8), 0, Fraction(1, 4)]
    saabas = CR.contribs(trees, w, CR.node_values(trees, cov), rows, [1, 2])
    assert saabas[0].tolist() == [0.25, 0.5, 0.0, 0.25]


# ---- (d) local accuracy, (e) the bias slot, (f) the slots ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMED)
def test_local_accuracy(name):
    trees, w, cov, rows, feats = named_case(name)
    _, got, _, total = named_gap(name)
    leaf = CR.leaf_sums(trees, w, rows)
    for i in range(len(rows)):
        s = np.float64(0.0)
        for v in got[i]:
            s = s + v
        assert abs(float(s) - float(leaf[i])) <= BOUND * total, (name, i, float(s), float(leaf[i]), BOUND * total)


@pytest.mark.parametrize("name", NAMED)
def test_the_bias_slot_has_the_bits_of_the_saabas_bias_slot(name):
    trees, w, cov, rows, feats = named_case(name)
    saabas = CR.contribs(trees, w, CR.node_values(trees, cov), rows, feats)
    assert bits(named_gap(name)[1][:, -1]).tolist() == bits(saabas[:, -1]).tolist()


@pytest.mark.parametrize("name", ["count_37", "nodes_81"])
def test_the_slots(name):
    trees, w, cov, rows, feats = named_case(name)
    full = named_gap(name)[1]
    assert not bits(full[:, len(feats)]).any()                                   # every feature has its slot: rest is +0.0, the bits
    some = feats[1::2]
    cols = [max(feats) + 7] + some
    part = SR.shap(trees, w, cov, rows, cols)
    assert not bits(part[:, 0]).any()                                            # an id the model never splits on: +0.0
    assert bits(part[:, 1:1 + len(some)]).tolist() == bits(full[:, [feats.index(f) for f in some]]).tolist()
    assert bits(part[:, -1]).tolist() == bits(full[:, -1]).tolist() and part[:, len(cols)].all()


def test_a_single_leaf_adds_to_the_bias_only():
    g = TM.Gen(np.random.default_rng(31))
    trees, w = [TM.single_leaf(g) for _ in range(3)], np.array([0.1, -0.25, 3.0], np.float32)
    cov = CR.covers(trees, np.zeros((4, 3), np.float32))
    got = SR.shap(trees, w, cov, np.zeros((2, 3), np.float32), [2])
    assert not bits(got[:, :2]).any() and got[0, 2] != 0.0 and SR.max_path(trees) == 0


# ---- (g) the host side of the library -----------------------------------------------------------------------------------------------------
def test_the_host_side_on_a_six_tree_model(tmp_path):
    """tools/shap_host_check.cpp: rl_shap_host.h's path tables on hand-set leaf covers against the restatement (z as bit patterns), the
    factor tables, the argument checks and the path limit by message, and the kernel's LDS plan"""
    exe = str(tmp_path / "shap_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "shap_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    f32 = lambda h: np.array([int(h, 16)], np.uint32).view(np.float32)[0]         # noqa: E731
    trees, leaf, got = [], [], []
    for ln in out:
        p = ln.split()
        if p[0] == "tree":
            trees.append(dict(feature=[], threshold=[], left=[], right=[], output=[]))
            leaf.append([])
            got.append([])
        elif p[0] == "node":
            t = trees[-1]
            t["feature"].append(int(p[2])); t["left"].append(int(p[4])); t["right"].append(int(p[5]))
            t["threshold"].append(f32(p[3])); t["output"].append(f32(p[6]))
            leaf[-1].append(int(p[7]))
        elif p[0] in ("leaf", "elem", "max"):
            got[-1].append(ln)
    assert len(trees) == 6
    n_leaves = n_elems = n_conds = 0
    for t, lc, g in zip(trees, leaf, got):
        t = {k: np.array(v, np.float32 if k in ("threshold", "output") else np.int32) for k, v in t.items()}
        cov = np.array(lc, np.uint64)
        for j in range(len(lc) - 1, -1, -1):
            if t["feature"][j] != -1:
                cov[j] = cov[t["left"][j]] + cov[t["right"][j]]
        assert int(cov[0]) == 40
        want, longest = [], (-1, 0, 0)
        for k, (node, els) in enumerate(SR.leaf_elements(t, cov, SR.f64)):
            want.append("leaf %d %016x %d" % (node, bit1(t["output"][node]), len(els)))
            for f, z, conds in els:
                want.append("elem %d %d %016x %s" % (f, {7: 0, 2: 1}.get(f, 2), bit1(z), " ".join(
                    "%08x:%d" % (np.array([thr], np.float32).view(np.uint32)[0], int(gl)) for thr, gl in conds)))
                n_elems += 1
                n_conds += len(conds)
            if len(els) > longest[0]:
                longest = (len(els), k, node)
            n_leaves += 1
        want.append("max %d %d %d" % longest)
        assert g == want
    assert "all %d %d %d" % (n_leaves, n_elems, n_conds) in out and "P %d" % SR.P_LIMIT in out
    tabs = [ln.split() for ln in out if ln.startswith("table ")]
    assert len(tabs) == 19
    for _, l, i, *h in tabs:
        assert [int(x, 16) for x in h] == [bit1(tb[int(l), int(i)]) for tb in SR.tables(SR.f64)]
    who = "rl_model_predict_shap: "
    rcs = [ln for ln in out if ln.startswith("rc ")]
    assert rcs == ["rc 0 "] + ["rc -1 " + who + m for m in ("null model", "null X", "n_docs must be >= 0", "row_stride must be >= 1",
                                                             "the model has no trees")] + \
        ["rc 0 ", "rc -4 " + who + "more than 2^31 documents per call", "rc 0 ", "rc 0 "] + \
        ["rc -1 " + who + m for m in ("null output", "n_columns must be >= 0", "n_columns must be >= 1 with columns given",
                                      "columns[1] = -2 is negative", "columns[3] = 2 is listed twice", "scratch_bytes must be >= 0")] + \
        ["rc 0 ", "rc 0 ", "rc -4 " + who + "the path to leaf 32 (node 65) of tree 1 holds 33 distinct features, more than 32", "rc 0 "]
    assert [ln for ln in out if ln.startswith("longest ")] == ["longest 32", "longest 33", "longest 30"]
    plans = [tuple(int(x) for x in m.groups()) for m in (re.match(r"plan wd (\d+) slots (\d+): (\d) docs (\d+) per_pass (\d+) limit64 (\d+)", ln)
                                                        for ln in out) if m]
    assert len(plans) == 12
    for wd, slots, ok, docs, per, limit in plans:
        assert ok == 1 and limit == SR.slot_limit(wd, 64) and docs in (64, 128, 256)
        assert (per * (docs + 1) + wd * docs) * 8 <= 160 * 1024
        assert per == slots <= SR.slot_limit(wd, docs) or (docs == 64 and per == limit < slots)
        assert docs == 256 or slots > SR.slot_limit(wd, docs * 2)                # the widest block that holds every slot
    assert SR.slot_limit(33, 64) >= 1                                             # the longest w[] leaves room: no model is refused for the LDS


# ---- (h) symbols, the flag, the refusals that need no device ------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return N.lib()


def test_the_entry_points_are_declared_exported_and_named():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = C.CDLL(_lib()._name)
    for n in ("rl_model_predict_shap", "rl_model_shap_limits", "rl_debug_shap_times", "rl_debug_shap_passes"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in N.ABI_SYMBOLS
    assert lib.rl_abi_version() == 5 and re.search(r"RL_MODEL_PATH_SHAP = %d\b" % N.MODEL_PATH_SHAP, hdr) and N.MODEL_PATH_SHAP == 6


def test_the_refusals_that_need_no_device():
    lib = _lib()
    rows, out, a, b = np.zeros((4, 3), np.float32), np.zeros((4, 4)), C.c_int32(0), C.c_int32(0)
    for call, msg in ((lambda: lib.rl_model_predict_shap(None, rows.ctypes.data, 4, 3, None, 0, 0, out.ctypes.data), "rl_model_predict_shap: null model"),
                      (lambda: lib.rl_model_shap_limits(None, C.byref(a), C.byref(b)), "rl_model_shap_limits: null argument"),
                      (lambda: lib.rl_debug_shap_times(None), "rl_debug_shap_times: null argument"),
                      (lambda: lib.rl_debug_shap_passes(None), "rl_debug_shap_passes: null argument")):
        assert call() == -1 and lib.rl_last_error().decode() == msg
    assert N.shap_times() >= 0.0 and N.shap_passes() >= 0


def test_the_exact_flag_and_the_refusals(tmp_path, capsys):
    assert CL.main([]) == 0
    assert "[-exact]" in capsys.readouterr().out
    for argv, msg in ((["-exact", "-background", "b", "-test", "t"], "exactly one -load model"),
                      (["-load", "m", "-exact", "-test", "t"], "needs a -background file"),
                      (["-load", "m", "-background", "b", "-EXACT"], "needs a -test file"),
                      (["-load", "m", "-background", "b", "-test", "t", "-exact", "1"], "Unknown command-line parameter: 1")):
        with pytest.raises(N.RankLibError, match=msg):
            CL.main(argv)
    lin = tmp_path / "ca.txt"
    lin.write_text("## Coordinate Ascent\n## Restart = 5\n## MaxIteration = 25\n## StepBase = 0.05\n## StepScale = 2.0\n## Tolerance = 0.001\n"
                   "## Regularized = false\n## Slack = 0.001\n1:0.5 2:0.5\n")
    with pytest.raises(N.RankLibError, match="needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        CL.main(["-load", str(lin), "-background", "b", "-test", "t", "-exact"])


def test_a_forest_and_a_linear_model_are_refused_with_exact_too():
    from ranklib_amd.learning import CoorAscent, RFRanker
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Random Forests model has no trees of one ensemble: "
                                             "a forest is several ensembles averaged"):
        RFRanker().contributions([], [], exact=True)
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        CoorAscent().contributions([], [], exact=True)
