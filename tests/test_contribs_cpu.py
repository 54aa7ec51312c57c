"""Feature contributions without a GPU: the restatement (tests/contrib_restatement.py) against answers derived by hand and
against the properties the definitions imply, the host side of librlhip.so (rl_contrib_host.h) through tools/contrib_host_check.cpp, the
refusals of the entry points that need no device, and the command line's."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import contrib_restatement as CR
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(autouse=True)
def _restore_statics():
    """the command line writes the evaluator's statics, as every command line here does"""
    from ranklib_amd.evaluator import Evaluator
    saved = (Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile)
    yield
    Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile = saved


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------------------
def test_the_hand_derived_stump():
    trees, w, bg = CR.hand_stump()
    cov = CR.covers(trees, bg)
    assert cov[0].tolist() == [4, 3, 1]
    val = CR.node_values(trees, cov)
    assert bits(val[0]).tolist() == bits([0.0, -1.0, 3.0]).tolist()          # (3 * -1 + 1 * 3) / 4 is exactly +0.0
    rows = np.array([[0, -3.0], [0, 0.0], [0, 7.0], [0, np.nan]], np.float32)
    got = CR.contribs(trees, w, val, rows, [1])
    want = np.array([[-0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 0.0, 0.0]])      # feature 1, rest, bias; the NaN goes right
    assert bits(got).tolist() == bits(want).tolist()
    other = CR.contribs(trees, w, val, rows, [5])                            # feature 1 not asked for: it is the rest
    assert bits(other).tolist() == bits(want[:, [1, 0, 2]]).tolist()
    narrow = CR.contribs(trees, w, val, rows[:, :1], [1])                    # the column is beyond the row: it reads 0 and goes left
    assert bits(narrow).tolist() == bits([[-0.5, 0.0, 0.0]] * 4).tolist()


def test_a_node_the_background_never_reaches_takes_the_plain_average():
    trees = [TM.flatten(TM.S(1, 0.0, TM.L(1.0), TM.S(2, 0.0, TM.L(2.0), TM.L(5.0))))]
    bg = np.array([[0, -1.0, 9.0]] * 3, np.float32)                          # all left of the root
    cov = CR.covers(trees, bg)
    assert cov[0].tolist() == [3, 3, 0, 0, 0]
    val = CR.node_values(trees, cov)[0]
    assert val[2] == 3.5 and val[0] == 1.0                                   # (2 + 5) / 2; the root: (3 * 1 + 0 * 3.5) / 3
    none = CR.node_values(trees, [np.zeros(5, np.uint64)])[0]                # no background at all: plain averages everywhere
    assert none[2] == 3.5 and none[0] == (1.0 + 3.5) / 2


def test_a_subtree_with_one_empty_side_takes_the_other_childs_value():
    trees = [TM.flatten(TM.S(1, 0.0, TM.S(2, 0.0, TM.L(0.3), TM.L(-8.0)), TM.L(4.0)))]
    bg = np.array([[0, -1.0, -1.0], [0, -1.0, -2.0], [0, 1.0, 0.0]], np.float32)
    cov = CR.covers(trees, bg)
    assert cov[0].tolist() == [3, 2, 2, 0, 1]
    val = CR.node_values(trees, cov)[0]
    assert bits(val[1]) == bits(np.float64(np.float32(0.3)))                 # (2 * x + 0 * -8) / 2 == x


def test_the_vectorised_covers_are_the_scalar_ones():
    for name in ("count_37", "nan_leaf"):
        trees = TM.case(name)[0].trees
        for rows in (CR.grid_rows(np.random.default_rng(4), 130), CR.grid_rows(np.random.default_rng(4), 40, 6), np.zeros((0, 13), np.float32)):
            a, b = CR.covers(trees, rows), CR.covers_np(trees, rows)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(int(x[0]) == len(rows) for x in a)


# ---- 2. properties ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prop_case(name):
    if name == "chain_30":
        trees, w = CR.chain_model("left")
        rows = CR.grid_rows(np.random.default_rng(2), 80)
    else:
        c = TM.case(name)[0]
        trees, w, rows = c.trees, c.weights, c.rows[:80]
    bg = CR.grid_rows(np.random.default_rng(3), 150, rows.shape[1])
    val = CR.node_values(trees, CR.covers(trees, bg))
    return trees, w, rows, val, CR.paths(trees, rows)


@pytest.mark.parametrize("name", ["count_37", "nodes_81", "chain_30"])
def test_local_accuracy(name):
    """|sum of the slots - sum of W * out_leaf| <= n_adds * 2^-52 * sum |terms|: n_adds the additions behind the two sums, the terms every
    d, every bias term and every W * out_leaf -- the first-order bound of n rounded operations at 2^-53 each, doubled"""
    trees, w, rows, val, paths = prop_case(name)
    feats = CR.model_features(trees)
    dterms, lterms = [], []
    got = CR.contribs(trees, w, val, rows, feats, paths, dterms)
    leaf = CR.leaf_sums(trees, w, rows, paths, lterms)
    assert not got[:, len(feats)].any() and not np.signbit(got[:, len(feats)]).any()       # every feature asked for: rest is +0.0
    checked = 0
    for i in range(len(rows)):
        if not np.isfinite(leaf[i]):
            continue
        total = np.float64(0.0)
        for v in got[i]:
            total = total + v
        n_adds = len(dterms[i]) + len(got[i]) + len(lterms[i])
        bound = n_adds * U * (sum(abs(x) for x in dterms[i]) + sum(abs(x) for x in lterms[i]))
        assert abs(float(total) - float(leaf[i])) <= bound, (name, i, float(total), float(leaf[i]), bound)
        checked += 1
    assert checked == len(rows)


@pytest.mark.parametrize("name", ["count_37", "nodes_81"])
def test_the_rest_slot(name):
    trees, w, rows, val, paths = prop_case(name)
    feats = CR.model_features(trees)
    full = CR.contribs(trees, w, val, rows, feats, paths)
    some = feats[1::2]
    assert 0 < len(some) < len(feats)
    part = CR.contribs(trees, w, val, rows, some, paths)
    assert bits(part[:, :len(some)]).tolist() == bits(full[:, [feats.index(f) for f in some]]).tolist()
    assert bits(part[:, -1]).tolist() == bits(full[:, -1]).tolist()
    uses_other = np.array([any(int(t["feature"][j]) not in some for t, p in zip(trees, per) for j in p[:-1]) for per in paths])
    assert uses_other.any()
    for i, per in enumerate(paths):
        if not uses_other[i]:
            assert bits(part[i, len(some)]) == 0                             # +0.0, the bits
            continue
        # (a step between two nodes of equal value contributes exactly zero: the row must then have another one that does not)
        mag = sum(abs(float(np.float64(np.float32(wt)) * (v[n] - v[j]))) for t, wt, v, p in zip(trees, w, val, per)
                  for j, n in zip(p[:-1], p[1:]) if int(t["feature"][j]) not in some)
        assert mag > 0.0 and part[i, len(some)] != 0.0, (name, i)


# ---- 3. the host side of the library ------------------------------------------------------------------------------------------------------
def test_the_host_side_on_a_five_tree_model(tmp_path):
    """tools/contrib_host_check.cpp: rl_contrib_host.h's covers, node values and slots on hand-set leaf covers against the restatement, its
    argument checks by message, and the kernel's LDS plan"""
    exe = str(tmp_path / "contrib_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "contrib_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    trees, leaf, got = [], [], []
    for ln in out:
        p = ln.split()
        if p[0] == "tree":
            trees.append(dict(feature=[], threshold=[], left=[], right=[], output=[]))
            leaf.append([])
            got.append({})
        elif p[0] == "node":
            t = trees[-1]
            t["feature"].append(int(p[2])); t["left"].append(int(p[4])); t["right"].append(int(p[5]))
            t["threshold"].append(np.array([int(p[3], 16)], np.uint32).view(np.float32)[0])
            t["output"].append(np.array([int(p[6], 16)], np.uint32).view(np.float32)[0])
            leaf[-1].append(int(p[7]))
        elif p[0] in ("cover", "value", "slot"):
            got[-1][p[0]] = p[1:]
    assert len(trees) == 5
    for t, lc, g in zip(trees, leaf, got):
        t = {k: np.array(v, np.float32 if k in ("threshold", "output") else np.int32) for k, v in t.items()}
        cov = np.array(lc, np.uint64)
        for j in range(len(lc) - 1, -1, -1):
            if t["feature"][j] != -1:
                cov[j] = cov[t["left"][j]] + cov[t["right"][j]]
        assert [int(x) for x in g["cover"]] == cov.tolist() and int(cov[0]) == 40
        val = CR.node_values([t], [cov])[0]
        assert [int(x, 16) for x in g["value"]] == bits(val).tolist()
        want_slot = [-1 if f == -1 else {7: 0, 2: 1}.get(int(f), 2) for f in t["feature"]]
        assert [int(x) for x in g["slot"]] == want_slot
    rcs = [ln for ln in out if ln.startswith("rc ")]
    assert rcs == ["rc 0 ", "rc -1 who: null model", "rc -1 who: null X", "rc -1 who: n_docs must be >= 0", "rc -1 who: row_stride must be >= 1",
                   "rc -1 who: the model has no trees", "rc 0 ", "rc -4 who: more than 2^31 documents per call",
                   "rc 0 ", "rc 0 ", "rc -1 who: null output", "rc -1 who: n_columns must be >= 0",
                   "rc -1 who: n_columns must be >= 1 with columns given", "rc -1 who: columns[1] = -2 is negative",
                   "rc -1 who: columns[3] = 2 is listed twice", "rc -1 who: scratch_bytes must be >= 0", "rc 0 "]
    plans = {(int(m.group(1)), int(m.group(2))): tuple(int(x) for x in m.groups()[2:])
             for m in (re.match(r"plan maxn (\d+) slots (\d+): (\d) tile (\d+) docs (\d+) per_pass (\d+) limit64 (\d+)", ln) for ln in out) if m}
    for (maxn, slots), (ok, tile, docs, per, limit) in plans.items():
        assert (tile, limit) == (CR.tree_tile(maxn), CR.slot_limit(maxn, 64))
        assert ok == (1 if limit >= 1 else 0)
        if ok:
            assert tile * maxn * 32 + per * (docs + 1) * 8 <= 160 * 1024 and docs in (64, 128, 256)
            assert per == slots or (docs == 64 and per == limit < slots)
    assert plans[(3, 402)][2:4] == (64, 313) and plans[(61, 138)][2] == 128 and plans[(3, 3)][2] == 256 and plans[(5104, 3)][0] == 0


def _lib():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return N.lib()


def test_the_refusals_that_need_no_device():
    lib = _lib()
    rows, out, n = np.zeros((4, 3), np.float32), np.zeros((4, 4)), C.c_int64(5)
    for call, msg in ((lambda: lib.rl_model_cover(None, rows.ctypes.data, 4, 3, 0), "rl_model_cover: null model"),
                      (lambda: lib.rl_model_predict_contribs(None, rows.ctypes.data, 4, 3, None, 0, 0, out.ctypes.data), "rl_model_predict_contribs: null model"),
                      (lambda: lib.rl_model_get_cover(None, 0, None, None, 0, None), "rl_model_get_cover: null model"),
                      (lambda: lib.rl_model_predict_leaf_sums(None, rows.ctypes.data, 4, 3, out.ctypes.data), "rl_model_predict_leaf_sums: null model"),
                      (lambda: lib.rl_model_cover_rows(None, C.byref(n)), "rl_model_cover_rows: null argument"),
                      (lambda: lib.rl_debug_contrib_times(None, None), "rl_debug_contrib_times: null argument"),
                      (lambda: lib.rl_debug_contrib_passes(None), "rl_debug_contrib_passes: null argument")):
        assert call() == -1 and lib.rl_last_error().decode() == msg
    assert min(N.contrib_times()) >= 0.0 and N.contrib_passes() >= 0


def test_the_entry_points_are_declared_exported_and_named():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = C.CDLL(_lib()._name)
    for n in ("rl_model_cover", "rl_model_cover_rows", "rl_model_get_cover", "rl_model_predict_contribs", "rl_model_predict_leaf_sums",
              "rl_debug_contrib_times", "rl_debug_contrib_passes"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in N.ABI_SYMBOLS
    assert lib.rl_abi_version() == 5 and re.search(r"#define RLHIP_ABI_VERSION 5\b", hdr)
    assert re.search(r"RL_MODEL_PATH_COVER = %d, RL_MODEL_PATH_CONTRIBS = %d\b" % (N.MODEL_PATH_COVER, N.MODEL_PATH_CONTRIBS), hdr)
    assert (N.MODEL_PATH_COVER, N.MODEL_PATH_CONTRIBS) == (4, 5)


# ---- 4. the command line ------------------------------------------------------------------------------------------------------------------
def test_the_command_line_refusals(tmp_path, capsys):
    assert CL.main([]) == 0
    assert capsys.readouterr().out.startswith("Usage: -load model -background file [-background file ...] -test file [-feature file]")
    for argv, msg in ((["-background", "b", "-test", "t"], "exactly one -load model"),
                      (["-load", "m", "-test", "t"], "needs a -background file"),
                      (["-load", "m", "-background", "b"], "needs a -test file"),
                      (["-load", "m", "-background", "b", "-test", "t", "-bogus"], "Unknown command-line parameter: -bogus"),
                      (["-load", "m", "-background", "b", "-test", "t", "-feature"], "Missing value for -feature")):
        with pytest.raises(N.RankLibError, match=msg):
            CL.main(argv)
    lin = tmp_path / "ca.txt"
    lin.write_text("## Coordinate Ascent\n## Restart = 5\n## MaxIteration = 25\n## StepBase = 0.05\n## StepScale = 2.0\n## Tolerance = 0.001\n"
                   "## Regularized = false\n## Slack = 0.001\n1:0.5 2:0.5\n")
    with pytest.raises(N.RankLibError, match="needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"):
        CL.main(["-load", str(lin), "-background", "b", "-test", "t"])


def test_the_summary_arithmetic_and_order():
    ids = [3, 9, 4]
    m = np.array([[0.5, -1.0, 0.25, 0.0, 7.0], [-0.5, 1.0, 0.25, 0.0, 7.0], [0.25, 0.0, -0.5, 0.0, 7.0]])
    lines = CL.summary_lines(ids, m)
    assert lines == ["9\t0.6666666666666666\t0.0", "3\t0.4166666666666667\t0.08333333333333333", "4\t0.3333333333333333\t0.0"]
    tie = CL.summary_lines([8, 2], np.array([[1.0, -1.0, 0.0, 0.0]]))
    assert [ln.split("\t")[0] for ln in tie] == ["2", "8"]         # equal means: by id
