"""Interventional TreeSHAP without a GPU: tests/interv_restatement.py's exact run against Shapley values enumerated from
the meaning, hand cases, its f64 run's accuracy, rl_interv_host.h through tools/interv_host_check.cpp, the symbols, the flag, a refusal."""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import contrib_restatement as CR
import interv_restatement as IV
import shap_restatement as SR
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL
from test_shap_cpu import _lib, _restore_statics, bits, named_case, small_models      # noqa: F401  (the fixture is autouse)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = ["count_37", "nodes_81", "nan_leaf", "chain_left", "chain_right", "distinct_30"]


def small_background(k):
    """1 to 4 rows with NaN and +-Infinity cells; every other one is narrower than the model's features (a column beyond bg_stride)"""
    return CR.grid_rows(np.random.default_rng(100 + k), 1 + k % 4, 7 if k % 2 else 5, special=0.25)


@functools.lru_cache(maxsize=None)
def runs(name):
    """(trees, weights, rows, f64 run, exact run, sum |W out|) under all the model's features; the named models meet 20 background rows"""
    trees, w, _, rows, cols = small_models()[name] if isinstance(name, int) else named_case(name)
    bg = small_background(name) if isinstance(name, int) else CR.grid_rows(np.random.default_rng(3), 20, rows.shape[1])
    mag = []
    return trees, w, rows, bg, cols, IV.interv(trees, w, rows, bg, cols, abs_leaf=mag), IV.interv(trees, w, rows, bg, cols, IV.frac), sum(mag)


# ---- (a) the algorithm is the meaning ------------------------------------------------------------------------------------------------------
def test_the_computed_form_in_exact_arithmetic_is_the_shapley_value_of_the_hybrid_rows():
    moved = 0
    for k in range(len(small_models())):
        trees, w, rows, bg, cols, _, got, _ = runs(k)
        want = IV.brute(trees, w, rows, bg, cols)
        assert got.shape == want.shape and (got == want).all(), (k, np.argwhere(got != want)[0])      # Fractions: no tolerance
        leaf = [sum(SR.frac(np.float64(np.float32(wt))) * SR.frac(np.float64(t["output"][CR.walk(t, r)[-1]])) for t, wt in zip(trees, w)) for r in rows]
        assert got.sum(axis=1).tolist() == leaf, k                                  # local accuracy, exactly
        moved += int((got[:, :-1] != 0).sum())
    assert moved > 500


# ---- (b) hand values: the AND tree ---------------------------------------------------------------------------------------------------------
def test_the_and_tree_by_hand():
    trees, w, _ = SR.and_tree()
    doc, left = np.array([[0, 1.0, 1.0]], np.float32), np.array([[0, -1.0, -1.0]], np.float32)
    assert bits(IV.interv(trees, w, doc, left, [1, 2])).tolist() == bits([[0.5, 0.5, 0.0, 0.0]]).tolist()
    assert IV.interv(trees, w, doc, left, [1, 2], IV.frac)[0].tolist() == [Fraction(1, 2), Fraction(1, 2), 0, 0]
    assert bits(IV.interv(trees, w, doc, doc, [1, 2])).tolist() == bits([[0.0, 0.0, 0.0, 1.0]]).tolist()      # the document itself: bias only


# ---- (c) the f64 form is accurate, and sums to the leaf sums -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small"] + NAMED)
def test_the_f64_run_is_close_to_its_exact_run_and_sums_to_the_leaf_sums(name):
    worst = off = 0.0
    for key in (range(len(small_models())) if name == "small" else [name]):
        trees, w, rows, bg, cols, got, exact, mag = runs(key)
        leaf = CR.leaf_sums(trees, w, rows)
        for g, e, lf in zip(got, exact, leaf):
            worst = max(worst, float(sum(abs(Fraction(float(a)) - b) for a, b in zip(g, e))) / mag / IV.U)
            s = np.float64(0.0)
            for v in g:
                s = s + v
            off = max(off, abs(float(s) - float(lf)) / mag / IV.U)
    print("%s: worst gap %.3f, worst |sum of slots - leaf sum| %.3f, in units of 2^-52 x sum |W out|" % (name, worst, off))
    assert worst * IV.U <= IV.BOUND and off * IV.U <= IV.BOUND


# ---- (d) the host side of the library ------------------------------------------------------------------------------------------------------
def test_the_host_side(tmp_path):
    """tools/interv_host_check.cpp: T as bit patterns, the path tables without covers, the path limit and every argument check by
    message, the LDS plan and the tree chunks of the mask buffer"""
    exe = str(tmp_path / "interv_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "interv_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    T = IV.table(IV.f64)
    tabs = [ln.split() for ln in out if ln.startswith("table ")]
    assert len(tabs) == 32 * 33 // 2 and all(int(h, 16) == int(T[int(p), int(q)].view(np.uint64)) for _, p, q, h in tabs)
    assert "unused 0" in out and "paths 5 7 9" in out and "strides 4 4 8 16384" in out
    who = "rl_model_predict_shap_background: "
    assert [ln for ln in out if ln.startswith("rc ")] == ["rc 0 "] + ["rc -1 " + who + m for m in (
        "null model", "null X", "n_docs must be >= 0", "row_stride must be >= 1", "the model has no trees")] + [
        "rc -4 " + who + "more than 2^31 documents per call", "rc 0 "] + ["rc -1 " + who + m for m in (
            "null BG", "n_background must be >= 1", "n_background must be >= 1", "bg_stride must be >= 1")] + [
        "rc 0 ", "rc -4 " + who + "more than 16384 background rows"] + ["rc -1 " + who + m for m in (
            "null output", "columns[1] = -2 is negative", "scratch_bytes must be >= 0")] + [
        "rc 0 ", "rc -4 " + who + "the path to leaf 32 (node 65) of tree 1 holds 33 distinct features, more than 32"]
    # 160 KiB less T's 8 712 bytes and s[wd][docs] f64, in accumulators of (docs + 1) f64: 3 slots fit blocks of 256 whatever wd; 138 fit
    # blocks of 128 beside wd <= 1 (150, 149) and not beside 13 or 32 (137, 118); blocks of 64 hold 298, 297, 285 and 266 of 402 slots
    assert [tuple(int(x) for x in re.findall(r"\d+", ln)[2:]) for ln in out if ln.startswith("plan ")] == [
        (1, 256, 3), (1, 128, 138), (1, 64, 298), (1, 256, 3), (1, 128, 138), (1, 64, 297),
        (1, 256, 3), (1, 64, 138), (1, 64, 285), (1, 256, 3), (1, 64, 138), (1, 64, 266)]
    # trees of 2, 3, 4, 4, 1 and 2 leaves against 5 background rows (rows of 8 masks) are 84, 116, 148, 148, 52 and 84 bytes, 632 in all
    each = "0 1 2 3 4 5 6"
    assert [ln.split(None, 1)[1] for ln in out if ln.startswith("chunks ")] == [
        "5 0 0 6", "5 632 0 6", "5 400 0 3 6", "5 300 0 2 4 6", "5 1 " + each, "300 2000 " + each]


# ---- (e) symbols, the flag, the refusals that need no device -------------------------------------------------------------------------------
def test_the_entry_points_the_flag_and_the_refusals(capsys):
    from ranklib_amd.learning import RFRanker
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = C.CDLL(_lib()._name)
    for n in ("rl_model_predict_shap_background", "rl_debug_interv_times", "rl_debug_interv_passes"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in N.ABI_SYMBOLS, n
    assert lib.rl_abi_version() == 5 and re.search(r"RL_MODEL_PATH_INTERV = %d\b" % N.MODEL_PATH_INTERV, hdr) and N.MODEL_PATH_INTERV == 9
    assert CL.main([]) == 0
    assert "[-interventional] [-nbg n] [-bgseed s]" in capsys.readouterr().out
    for argv, msg in ((["-load", "m", "-interventional", "-nbg", "7", "-bgseed", "3", "-test", "t"], "needs a -background file"),
                      (["-load", "m", "-background", "b", "-test", "t", "-interventional", "-exact"], "-interventional or -exact / -interactions, not both"),
                      (["-load", "m", "-background", "b", "-test", "t", "-interactions", "p", "-INTERVENTIONAL"], "not both")):
        with pytest.raises(N.RankLibError, match=msg):
            CL.main(argv)
    with pytest.raises(N.RankLibError, match="contributions needs a LambdaMART or MART model: a Random Forests model has no trees of one ensemble"):
        RFRanker().contributions([], [], interventional=True, nBackground=5, backgroundSeed=2)
