"""SHAP interaction values without a GPU: the computed form of tests/interact_restatement.py in exact arithmetic against
the Shapley interaction index enumerated from the definition, its f64 run against its own exact run, hand cases, the slot rules, the host
side of librlhip.so (rl_interact_host.h) through tools/interact_host_check.cpp, the exported symbols and the command line's flag."""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import contrib_restatement as CR
import interact_restatement as IR
import shap_restatement as SR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL
from test_shap_cpu import named_case, small_exact, small_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = IR.U


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(autouse=True)
def _restore_statics():
    """the command line writes the evaluator's statics, as every command line here does"""
    from ranklib_amd.evaluator import Evaluator
    saved = (Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile)
    yield
    Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile = saved


@functools.lru_cache(maxsize=None)
def small_exact_interactions():
    return [IR.interactions(t, w, cov, rows, cols, IR.frac) for t, w, cov, rows, cols in small_models()]


# ---- (a) the algorithm is the definition --------------------------------------------------------------------------------------------------
def test_the_computed_form_in_exact_arithmetic_is_the_interaction_index():
    pairs = 0
    for k, ((trees, w, cov, rows, cols), got, phi) in enumerate(zip(small_models(), small_exact_interactions(), small_exact())):
        want = IR.brute(trees, w, cov, rows, cols)
        S_ = len(cols) + 2
        assert got.shape == want.shape == (5, S_, S_)
        assert (got == want).all(), (k, np.argwhere(got != want)[0])                # Fractions: no tolerance
        assert (got == got.transpose(0, 2, 1)).all(), k                             # exactly symmetric
        assert (got.sum(axis=2) == phi).all(), k                                    # the rows sum to the SHAP values
        leaf = [sum(SR.frac(np.float64(np.float32(wt))) * SR.value_of_set(t, c, row, frozenset(int(f) for f in t["feature"] if f != -1))
                    for t, wt, c in zip(trees, w, cov)) for row in rows]
        assert got.sum(axis=(1, 2)).tolist() == leaf, k                             # the cells sum to the leaf sum
        pairs += int((got[:, :S_ - 1, :S_ - 1][:, ~np.eye(S_ - 1, dtype=bool)] != 0).sum())
    assert pairs > 2000                                                             # (the models do pair features)


# ---- (b) the f64 restatement is accurate --------------------------------------------------------------------------------------------------
def asymmetry(got):
    with np.errstate(all="ignore"):
        return float(np.abs(got - got.transpose(0, 2, 1)).max(initial=0.0))


def gaps_of(trees, w, cov, rows, cols, exact=None):
    """(the worst row's gap, the worst asymmetry), both in units of 2^-52 x (sum over trees of sum over leaves of |W out|).  A row's gap
    is the sum over ALL cells of its matrix of |f64 - exact|"""
    mag = []
    got = IR.interactions(trees, w, cov, rows, cols, IR.f64, abs_leaf=mag)
    if exact is None:
        exact = IR.interactions(trees, w, cov, rows, cols, IR.frac)
    assert np.isfinite(got).all()
    gap = max((sum(abs(Fraction(float(g)) - e) for g, e in zip(gr.ravel(), er.ravel())) for gr, er in zip(got, exact)), default=Fraction(0))
    total = sum(mag)
    return (float(gap) / total / U, asymmetry(got) / total / U) if total else (float(gap), asymmetry(got))


def test_the_f64_run_is_close_to_its_exact_run_on_the_small_models():
    worst = [0.0, 0.0]
    for m, exact in zip(small_models(), small_exact_interactions()):
        worst = [max(a, b) for a, b in zip(worst, gaps_of(*m, exact=exact))]
    print("small models: worst gap %.3f, worst asymmetry %.3f x 2^-52 x sum |W out|" % tuple(worst))
    assert worst[0] * U <= IR.BOUND_GAP and worst[1] * U <= IR.BOUND_ASYM


NAMED = ["count_37", "nodes_81", "nan_leaf", "chain_left", "chain_right", "distinct_30"]
# test_shap_cpu.named_case's rows of the 30-feature chain whose exact run is made here: the one that goes left everywhere, the one that
# leaves at the root, and the two of the longest walks that were the worst of the twelve (all twelve: 57 s of Fraction arithmetic;
# the others' gaps were 1 396 to 4 055)
D30_ROWS = [0, 1, 6, 10]


@pytest.mark.parametrize("name", NAMED)
def test_the_f64_run_is_close_to_its_exact_run(name):
    trees, w, cov, rows, feats = named_case(name)
    if name == "distinct_30":
        rows = rows[D30_ROWS]
    gap, asym = gaps_of(trees, w, cov, rows, feats)
    print("%s: worst gap %.3f, worst asymmetry %.3f x 2^-52 x sum |W out|" % (name, gap, asym))
    assert gap * U <= IR.BOUND_GAP and asym * U <= IR.BOUND_ASYM


def test_the_asymmetry_of_the_30_feature_chain_on_the_rows_of_the_gpu_test():
    """the asymmetry needs no exact run, so it is measured on all 257 rows tests/test_gpu_interact.py walks (the same generator calls,
    background included), where the gap is measured on four"""
    trees, w = SR.distinct_chain(30)
    bg = CR.grid_rows(np.random.default_rng(41), 5000, 35)
    rows = CR.grid_rows(np.random.default_rng(42), 257, 35)
    mag = []
    got = IR.interactions(trees, w, CR.covers_np(trees, bg), rows, CR.model_features(trees), abs_leaf=mag)
    asym = asymmetry(got) / sum(mag) / U
    print("distinct_30, 257 rows: worst asymmetry %.3f x 2^-52 x sum |W out|" % asym)
    assert asym * U <= IR.BOUND_ASYM


# ---- (c) hand cases -----------------------------------------------------------------------------------------------------------------------
def test_the_and_tree():
    trees, w, bg = SR.and_tree()
    cov = CR.covers(trees, bg)
    rows = np.array([[0, 1.0, 1.0]], np.float32)                       # the row that goes right twice
    want = [[0.25, 0.125, 0.0, 0.0], [0.125, 0.25, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.25]]
    assert bits(IR.interactions(trees, w, cov, rows, [1, 2])[0]).tolist() == bits(want).tolist()
    exact = IR.interactions(trees, w, cov, rows, [1, 2], IR.frac)[0]
    assert exact.tolist() == [[Fraction(1, 4), Fraction(1, 8), 0, 0], [Fraction(1, 8), Fraction(1, 4), 0, 0], [0, 0, 0, 0], [0, 0, 0, Fraction(1, 4)]]


def test_the_stump():
    trees, w, bg = CR.hand_stump()
    cov = CR.covers(trees, bg)
    rows = np.array([[0, -3.0], [0, 0.0], [0, 7.0], [0, np.nan]], np.float32)
    got = IR.interactions(trees, w, cov, rows, [1])
    phi = SR.shap(trees, w, cov, rows, [1])
    want = np.zeros((4, 3, 3))
    want[:, 0, 0] = phi[:, 0]                                          # the diagonal is the SHAP value, every off-diagonal cell +0.0
    want[:, 2, 2] = phi[:, 2]
    assert bits(got).tolist() == bits(want).tolist() and phi[:, 0].tolist() == [-0.5, -0.5, 1.5, 1.5]


def test_a_single_leaf_model_fills_the_bias_cell_only():
    g = TM.Gen(np.random.default_rng(31))
    trees, w = [TM.single_leaf(g) for _ in range(3)], np.array([0.1, -0.25, 3.0], np.float32)
    cov = CR.covers(trees, np.zeros((4, 3), np.float32))
    rows = np.zeros((2, 3), np.float32)
    got = IR.interactions(trees, w, cov, rows, [2])
    want = np.zeros((2, 3, 3))
    want[:, 2, 2] = SR.shap(trees, w, cov, rows, [2])[:, 2]
    assert bits(got).tolist() == bits(want).tolist() and got[0, 2, 2] != 0.0


# ---- (d) the slot rules, by bit pattern ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["count_37", "nodes_81"])
def test_the_slots(name):
    trees, w, cov, rows, feats = named_case(name)
    C_ = len(feats)
    full = IR.interactions(trees, w, cov, rows, feats)
    phi = SR.shap(trees, w, cov, rows, feats)
    assert not bits(full[:, C_, :]).any() and not bits(full[:, :, C_]).any()           # columns == NULL: rest is +0.0, row and column
    assert not bits(full[:, C_ + 1, :C_ + 1]).any() and not bits(full[:, :C_ + 1, C_ + 1]).any()      # the bias row and column
    assert bits(full[:, C_ + 1, C_ + 1]).tolist() == bits(phi[:, C_ + 1]).tolist() and full[:, C_ + 1, C_ + 1].all()
    some = feats[1::2]
    cols = [max(feats) + 7] + some
    part = IR.interactions(trees, w, cov, rows, cols)
    K = len(cols)
    assert not bits(part[:, 0, :]).any() and not bits(part[:, :, 0]).any()             # an id the model never splits on
    at = [feats.index(f) for f in some]
    off = ~np.eye(len(some), dtype=bool)
    assert bits(part[:, 1:K, 1:K][:, off]).tolist() == bits(full[:, at][:, :, at][:, off]).tolist()    # requested cells keep their bits
    assert part[:, K, 1:K].any() and part[:, 1:K, K].any() and part[:, K, K].any()     # the other features are in rest
    assert bits(part[:, K + 1, K + 1]).tolist() == bits(full[:, C_ + 1, C_ + 1]).tolist()


def test_two_features_that_both_fall_into_rest_add_to_no_cell_but_the_diagonal_of_rest():
    trees, w, bg = SR.and_tree()
    cov = CR.covers(trees, bg)
    rows = np.array([[0, 1.0, 1.0], [0, 1.0, -1.0], [0, -1.0, 1.0]], np.float32)
    got = IR.interactions(trees, w, cov, rows, [5])                    # features 1 and 2 are both in rest: their pair is not walked
    phi = SR.shap(trees, w, cov, rows, [5])
    want = np.zeros((3, 3, 3))
    want[:, 1, 1] = phi[:, 1]                                          # out[rest][rest] moves through phi_rest alone
    want[:, 2, 2] = phi[:, 2]
    assert bits(got).tolist() == bits(want).tolist() and got[:, 1, 1].all()
    assert all(not x[3].all() for x in IR.pair_terms(trees, w, cov, rows)[0])      # (the pair has terms: they are left out by the slot rule)


# ---- (e) the host side of the library -----------------------------------------------------------------------------------------------------
def test_the_host_side(tmp_path):
    """tools/interact_host_check.cpp: rl_interact_host.h's per-slot leaf lists on hand-built trees, the LDS plan at its edges, the
    row-chunk rule and every argument check by message"""
    exe = str(tmp_path / "interact_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "interact_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for tag, n_slots in (("some", 4), ("all", 6), ("leaf", 2)):
        leaves = [[int(x) for x in ln.split()[2:]] for ln in out if ln.startswith(tag + " leaf ")]
        assert ["%s leaves %d" % (tag, len(leaves))] == [ln for ln in out if ln.startswith(tag + " leaves")]
        want = []
        for s in range(n_slots):                                       # ascending leaves with an element in the slot and at least two elements
            mine = ["%d:%d" % (lf, t) for lf, t, d, *slots in leaves if d >= 2 and s in slots]
            want.append(" ".join(["%s list %d" % (tag, s)] + mine))
        assert [ln for ln in out if ln.startswith(tag + " list ")] == want
        assert all(d == len(slots) for _, _, d, *slots in leaves)
    some = [ln for ln in out if ln.startswith("some l")]
    assert "some leaf 8 2 3 0 3 3" in some and "some list 3 6:2 7:2 8:2 9:2" in some          # rest holds two elements of one leaf, listed once
    assert "some list 2 12:4 13:4" in some and "all list 5" in out and "leaf list 0" in out    # rest is empty under every feature; single leaves
    plans = [tuple(int(x) for x in m.groups()) for m in (re.match(
        r"plan longest (\d+) wr (\d+) slots (\d+): (\d) docs (\d+) per_pass (\d+) limit64 (\d+) limit128 (\d+) limit256 (\d+)", ln) for ln in out) if m]
    assert len(plans) == 15
    for longest, wr, slots, ok, docs, per, l64, l128, l256 in plans:
        assert wr == max(1, longest) and ok == 1 and docs in (64, 128, 256)
        assert (l64, l128, l256) == (IR.slot_limit(wr, 64), IR.slot_limit(wr, 128), IR.slot_limit(wr, 256))
        assert (per * (docs + 1) + wr * docs) * 8 <= 160 * 1024
        assert per == slots <= IR.slot_limit(wr, docs) or (docs == 64 and per == l64 < slots)
        assert docs == 256 or slots > IR.slot_limit(wr, docs * 2)                # the widest block that holds every slot
    assert IR.slot_limit(32, 64) == SR.slot_limit(33, 64) + 1 == 283             # one row of w[] less than k_model_shap's
    chunks = [[int(x) for x in re.findall(r"-?\d+", ln)] for ln in out if ln.startswith("chunk ")]
    assert len(chunks) == 8
    for n, stride, c, scratch, got, per_row in chunks:
        assert per_row == 4 * stride + 8 * (c + 2) ** 2 + 8 * (c + 2) and got == IR.chunk_rows(n, stride, c, scratch)
    assert [c[4] for c in chunks] == [257, 100, 99, 1, 1, 1743, 6972, 1]
    who = "rl_model_predict_interactions: "
    rcs = [ln for ln in out if ln.startswith("rc ")]
    assert rcs == ["rc 0 "] + ["rc -1 " + who + m for m in ("null model", "null X", "n_docs must be >= 0", "row_stride must be >= 1",
                                                             "the model has no trees")] + \
        ["rc 0 ", "rc -4 " + who + "more than 2^31 documents per call", "rc 0 ", "rc 0 "] + \
        ["rc -1 " + who + m for m in ("null output", "n_columns must be >= 0", "n_columns must be >= 1 with columns given",
                                      "columns[1] = -2 is negative", "columns[3] = 2 is listed twice", "scratch_bytes must be >= 0")] + \
        ["rc 0 ", "rc 0 ", "rc 0 ", "rc -4 " + who + "65536 conditioned slots, more than 65535", "rc 0 ",
         "rc -4 " + who + "the path to leaf 32 (node 65) of tree 0 holds 33 distinct features, more than 32"]
    assert [ln for ln in out if ln.startswith("longest ")] == ["longest 32", "longest 33"]


# ---- (f) symbols, the flag, the refusals that need no device ------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return N.lib()


def test_the_entry_points_are_declared_exported_and_named():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = C.CDLL(_lib()._name)
    for n in ("rl_model_predict_interactions", "rl_debug_interact_times", "rl_debug_interact_passes"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in N.ABI_SYMBOLS
    assert lib.rl_abi_version() == 5 and re.search(r"RL_MODEL_PATH_INTERACT = %d\b" % N.MODEL_PATH_INTERACT, hdr) and N.MODEL_PATH_INTERACT == 8


def test_the_refusals_that_need_no_device():
    lib = _lib()
    rows, out, a = np.zeros((4, 3), np.float32), np.zeros((4, 4, 4)), C.c_double(0)
    for call, msg in ((lambda: lib.rl_model_predict_interactions(None, rows.ctypes.data, 4, 3, None, 0, 0, out.ctypes.data),
                       "rl_model_predict_interactions: null model"),
                      (lambda: lib.rl_debug_interact_times(C.byref(a), None), "rl_debug_interact_times: null argument"),
                      (lambda: lib.rl_debug_interact_passes(None), "rl_debug_interact_passes: null argument")):
        assert call() == -1 and lib.rl_last_error().decode() == msg
    assert min(N.interact_times()) >= 0.0 and N.interact_passes() >= 0


def test_the_interactions_flag_and_the_refusals(tmp_path, capsys):
    assert CL.main([]) == 0
    assert "[-interactions tsv]" in capsys.readouterr().out
    for argv, msg in ((["-interactions", "p", "-background", "b", "-test", "t"], "exactly one -load model"),
                      (["-load", "m", "-interactions", "p", "-test", "t"], "needs a -background file"),
                      (["-load", "m", "-background", "b", "-INTERACTIONS", "p"], "needs a -test file"),
                      (["-load", "m", "-background", "b", "-test", "t", "-interactions"], "Missing value for -interactions")):
        with pytest.raises(N.RankLibError, match=msg):
            CL.main(argv)
    lin = tmp_path / "ca.txt"
    lin.write_text("## Coordinate Ascent\n## Restart = 5\n## MaxIteration = 25\n## StepBase = 0.05\n## StepScale = 2.0\n## Tolerance = 0.001\n"
                   "## Regularized = false\n## Slack = 0.001\n1:0.5 2:0.5\n")
    with pytest.raises(N.RankLibError, match="needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        CL.main(["-load", str(lin), "-background", "b", "-test", "t", "-interactions", str(tmp_path / "p.tsv")])


def test_the_pair_lines_of_the_command_line():
    """the sums are one serial chain per cell in file order whatever the chunking, divided once; sorted by the first number descending,
    then by the ids; the pairs with rest apart"""
    rng = np.random.default_rng(8)
    inter = rng.standard_normal((7, 5, 5)) * 10.0 ** rng.integers(-8, 8, (7, 5, 5))
    vals = CL.pair_values(inter)
    assert vals.shape == (7, 4, 4) and vals[3, 1, 2] == inter[3, 1, 2] + inter[3, 2, 1] and vals[3, 2, 2] == inter[3, 2, 2]
    want_a, want_s = np.zeros((4, 4)), np.zeros((4, 4))
    for d in range(7):
        want_a, want_s = want_a + np.abs(vals[d]), want_s + vals[d]
    for cuts in ([0, 7], [0, 1, 2, 3, 4, 5, 6, 7], [0, 3, 3, 7]):
        a, s = np.zeros((4, 4)), np.zeros((4, 4))
        for lo, hi in zip(cuts, cuts[1:]):
            a, s = CL.chain_sums(a, np.abs(vals[lo:hi])), CL.chain_sums(s, vals[lo:hi])
        assert bits(a).tolist() == bits(want_a).tolist() and bits(s).tolist() == bits(want_s).tolist()
    a = np.array([[4.0, 6.0, 0.0, 1.0], [6.0, 6.0, 2.0, 1.0], [0.0, 2.0, 0.0, 3.0], [1.0, 1.0, 3.0, 8.0]])
    kept, rest = CL.pair_lines([9, 2, 5], a, -a, 2)
    assert kept == ["2\t2\t3.0\t-3.0", "9\t2\t3.0\t-3.0", "9\t9\t2.0\t-2.0", "2\t5\t1.0\t-1.0", "5\t5\t0.0\t-0.0", "9\t5\t0.0\t-0.0"]
    assert rest == ["rest\trest\t4.0\t-4.0", "5\trest\t1.5\t-1.5", "9\trest\t0.5\t-0.5", "2\trest\t0.5\t-0.5"]


def test_a_forest_and_a_linear_model_are_refused():
    from ranklib_amd.learning import CoorAscent, RFRanker
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Random Forests model has no trees of one ensemble: "
                                             "a forest is several ensembles averaged"):
        RFRanker().interactions([], [])
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        CoorAscent().interactions([], [])
