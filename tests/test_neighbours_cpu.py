"""Neighbours in leaf space without a device (rl_model_predict_neighbours): the names, every refusal that needs no model, those after the model
and the plan of a call through tools/near_host_check.cpp, the command line's argument errors and the rankers that have no leaves to share."""
import os
import re
import subprocess

import numpy as np
import pytest

from ranklib_amd import _native as N
from ranklib_amd import learning as RL
from ranklib_amd import neighbours as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rl_model_predict_neighbours", "rl_debug_neighbours_times")


def test_the_names_are_in_the_header_the_library_and_the_symbol_list():
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    lib = N.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in N.ABI_SYMBOLS
    assert re.search(r"RL_MODEL_PATH_NEIGHBOURS = %d\b" % N.MODEL_PATH_NEIGHBOURS, hdr) and N.MODEL_PATH_NEIGHBOURS == 13
    assert re.search(r"RL_NEAR_SKIP_SAME_INDEX = 1\b", hdr) and re.search(r"#define RL_NEAR_MAX_K %d\b" % N.NEAR_MAX_K, hdr)
    assert lib.rl_abi_version() == 5


@pytest.mark.parametrize("kw,rc,text", [
    (dict(), -1, "null model"), (dict(Xq=None), -1, "null Xq"), (dict(Xr=None), -1, "null Xr"), (dict(index=None), -1, "null out_index"),
    (dict(shared=None), -1, "null out_shared"), (dict(nq=0), -1, "nq must be >= 1"), (dict(nr=0), -1, "nr must be >= 1"),
    (dict(stride=0), -1, "row_stride must be >= 1"), (dict(k=0), -1, "k = 0 is outside [1, 64]"), (dict(k=65), -1, "k = 65 is outside [1, 64]"),
    (dict(flags=6), -1, "unknown flags 6"), (dict(scratch=-1), -1, "scratch_bytes must be >= 0"), (dict(first=-1), -1, "first_tree must be >= 0"),
    (dict(cnt=-1), -1, "n_trees must be >= 0")])
def test_the_refusals_that_need_no_device(kw, rc, text):
    """the model is looked at after the arguments that need none, so a null model reaches every one of them"""
    lib = N.lib()
    rows, out = np.zeros((4, 3), np.float32), np.zeros(8, np.int32)
    a = dict(dict(Xq=rows.ctypes.data, nq=4, Xr=rows.ctypes.data, nr=4, stride=3, first=0, cnt=0, k=2, flags=1, scratch=0, index=out.ctypes.data,
                  shared=out.ctypes.data), **kw)
    got = lib.rl_model_predict_neighbours(None, a["Xq"], a["nq"], a["Xr"], a["nr"], a["stride"], a["first"], a["cnt"], a["k"], a["flags"], a["scratch"],
                                          a["index"], a["shared"], None)
    assert (got, lib.rl_last_error().decode()) == (rc, "rl_model_predict_neighbours: " + text)


def test_the_times_and_the_wrapper_refuse_by_message():
    with pytest.raises(N.RankLibError, match="rl_debug_neighbours_times: null argument"):
        N.check(N.lib().rl_debug_neighbours_times(None, None))
    assert N.debug_neighbours_times() >= (0.0, 0.0)
    for q, r, text in ((np.zeros(3), np.zeros((2, 3)), r"neighbours take queries \[nq\]\[row_stride\] and reference \[nr\]\[row_stride\]"),
                       (np.zeros((2, 3)), np.zeros((2, 4)), "one width \\(got 3 and 4\\)")):
        with pytest.raises(N.RankLibError, match=text):        # (refused before the handle is looked at)
            N.Model.predict_neighbours(None, q, r, 1)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/near_host_check.cpp: rl_near_host.h's shape, checks and plan as a program of its own"""
    exe = str(tmp_path_factory.mktemp("near") / "near_host_check")
    subprocess.check_call(["g++", "-std=c++17", os.path.join(ROOT, "tools", "near_host_check.cpp"), "-o", exe])
    return lambda *a: subprocess.check_output([exe] + [str(v) for v in a], text=True).splitlines()


def test_the_mirrored_shape_and_the_refusals_that_need_a_model(host_check):
    assert host_check("shape") == ["shape %d %d %d %d %d 63 65535" % (N.NEAR_QUERY_TILE, N.NEAR_REF_TILE, N.NEAR_TREE_CHUNK, N.NEAR_BLOCKS, N.NEAR_MAX_K)]
    for args, want in (((70000, 2, 2, 0, 65535, 1, 0), "0 65535 "),                  # the longest window the packed 16-bit counters take
                       ((70000, 2, 2, 0, 65536, 1, 0), "-4 65536 a window of 65536 trees: 65535 at most"), ((70000, 2, 2, 4465, 0, 1, 1), "0 65535 "),
                       ((70000, 2, 2, 0, 0, 1, 0), "-4 70000 a window of 70000 trees: 65535 at most"),
                       ((0, 2, 2, 0, 0, 1, 0), "-1 0 the model has no trees"), ((-1, 2, 2, 0, 0, 1, 0), "-1 0 null model"),
                       ((5, 2, 2, 5, 0, 1, 0), "-1 0 first_tree = 5 is outside [0, 5)"), ((5, 2, 2, 2, 4, 1, 0), "-1 4 n_trees = 4 from tree 2 leaves the model's 5 trees"),
                       ((5, 1 << 31, 2, 0, 0, 1, 0), "-4 5 more than 2^31 rows per call"), ((5, 2, 1 << 31, 0, 0, 1, 0), "-4 5 more than 2^31 rows per call"),
                       ((5, (1 << 31) - 1, (1 << 31) - 1, 1, 0, 64, 1), "0 4 ")):
        assert host_check("check", *args) == [want], args


def test_the_plan_of_a_call(host_check):
    """plan <query chunk> <reference band> <rows of the partial lists>, then launch <queries> <references> <tiles per split> <splits>"""
    qt, rt = N.NEAR_QUERY_TILE, N.NEAR_REF_TILE
    assert host_check("plan", 1, 1, 188, 0) == ["plan 1 1 1", "launch 1 1 1 1"]
    assert host_check("plan", 1, 3 * rt, 188, 0) == ["plan 1 %d 3" % (3 * rt), "launch 1 %d 1 3" % (3 * rt)]
    # 65 reference tiles: 63 splits at most, so two tiles a split and a last split of one -- the shape tests/test_gpu_neighbours.py runs
    assert host_check("plan", qt + 1, 64 * rt + 1, 188, 0) == ["plan %d %d %d" % (qt + 1, 64 * rt + 1, 63 * (qt + 1)), "launch %d %d 2 33" % (qt + 1, 64 * rt + 1)]
    # many queries: ceil(1024 / 157) = 7 splits of 107 tiles under the default scratch, 11 bands
    assert host_check("plan", 10000, 1000000, 2548, 0) == ["plan 10000 95232 70000", "launch 10000 47680 54 7", "launch 10000 95232 107 7"]
    # one byte of scratch: one query tile a chunk, one reference tile a band
    assert host_check("plan", 2 * qt + 2, 2 * rt + 1, 188, 1) == ["plan %d %d %d" % (qt, rt, qt)] + ["launch %d %d 1 1" % (a, b) for a in (2, qt) for b in (1, rt)]


def test_a_line_of_the_command_line():
    assert NB.out_line(RL.DataPoint("2 qid:q7 1:0.5 # doc-3"), 1, RL.DataPoint("1 qid:q9 1:0.25"), 40, 67) == "q7\t# doc-3\t1\tq9\t\t1\t40\t67"


@pytest.mark.parametrize("argv,text", [
    (["-test", "f", "-reference", "r", "-out", "o"], "ranklib_amd.neighbours takes exactly one -load model (got 0)"),
    (["-load", "a", "-reference", "r", "-out", "o"], "ranklib_amd.neighbours takes exactly one -test file (got 0)"),
    (["-load", "a", "-test", "f", "-out", "o"], "ranklib_amd.neighbours takes -self or exactly one -reference file (got 0)"),
    (["-load", "a", "-test", "f", "-self", "-reference", "r", "-out", "o"], "ranklib_amd.neighbours takes -self or exactly one -reference file (got -self and 1)"),
    (["-load", "a", "-test", "f", "-self"], "ranklib_amd.neighbours needs -out tsv"),
    (["-load", "a", "-test", "f", "-self", "-out", "o", "-k", "0"], "-k must be in 1 .. 64 (got 0)"),
    (["-load", "a", "-test", "f", "-self", "-out", "o", "-k", "65"], "-k must be in 1 .. 64 (got 65)"),
    (["-load", "a", "-test", "f", "-self", "-out", "o", "-k", "x"], "-k takes a number of neighbours (got x)"),
    (["-load", "a", "-test", "f", "-self", "-out", "o", "-from", "-1"], "-from must be at least 0 (got -1)"),
    (["-load", "a", "-test", "f", "-self", "-out", "o", "-count", "0"], "-count must be at least 1 (got 0)"),
    (["-load", "a", "-test", "f", "-self", "-out"], "Missing value for -out"),
    (["-load", "a", "-test", "f", "-self", "-out", "o", "-gmax", "2"], "Unknown command-line parameter: -gmax")])
def test_the_command_line_refuses_by_message(argv, text):
    with pytest.raises(N.RankLibError) as e:
        NB.main(argv)
    assert str(e.value) == text
    assert NB.main([]) == 0                                    # the usage line


@pytest.mark.parametrize("cls,text", [
    (RL.RFRanker, RL.NEIGHBOURS_NOT_BAGS),
    (RL.CoorAscent, "rlhip: neighbours needs a LambdaMART or MART model: a Coordinate Ascent model has no trees"),
    (RL.LinearRegRank, "rlhip: neighbours needs a LambdaMART or MART model: a Linear Regression model has no trees"),
    (RL.RankNet, "rlhip: neighbours needs a LambdaMART or MART model: a RankNet model has no trees")])
def test_rankers_without_one_ensemble_of_trees_are_refused(cls, text):
    with pytest.raises(N.RankLibError) as e:
        cls().neighbours([], [])
    assert str(e.value) == text and "\n" not in text and "Random Forests" in RL.NEIGHBOURS_NOT_BAGS
