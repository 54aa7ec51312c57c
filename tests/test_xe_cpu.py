"""The XE-NDCG objective where it needs no device: the restatement against a long-double evaluation of the loss's gradient, its
guard and its short lists; the packing of ranklib_amd/csrc/rl_xe_host.h (through tools/xe_host_check.cpp) against a few lines of Python; the
command line's refusals; the two ABI names."""
import os
import subprocess

import numpy as np
import pytest

import xe_restatement as XR
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd.learning import LambdaMART, RFRanker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.mark.parametrize("n,seed", [(2, 1), (7, 2), (40, 3)])
def test_first_order_term_is_softmax_minus_target(n, seed):
    rng = np.random.default_rng(seed)
    s, lab = rng.normal(size=n), rng.integers(0, 5, n).astype(np.float32)
    gamma = XR.gammas(seed, 0, 100, n)
    assert all(0.0 <= g < 1.0 for g in gamma)
    e, phi = np.exp(s.astype(LD) - LD(s.max())), np.exp2(lab.astype(LD)) - np.array(gamma, LD)
    want = e / e.sum() - phi / phi.sum()
    assert np.all(np.abs(np.array(XR.list_terms(list(s), list(lab), gamma)["a"], LD) - want) <= 1e-13 * np.abs(want))


def test_a_dominating_score_stays_finite_and_one_document_gives_zeros():
    t = XR.list_terms([0.3, 800.5, -0.2, 0.1], [1.0, 0.0, 3.0, 2.0], XR.gammas(5, 2, 0, 4))
    assert np.all(np.isfinite(t["lam"])) and t["w"] == [0.0] * 4      # rho = (0, 1, 0, 0): the guard divides
    assert XR.lambdas([1.5], [2.0], [0, 1], 5, 0) == ([0.0], [0.0])


def _pack(lens, tile):
    """consecutive whole lists while they fit a tile; a list above the tile alone -> [(first list, lists)]"""
    out, docs = [], 0
    for q, n in enumerate(lens):
        if n > tile or not out or out[-1][2] or docs + n > tile:
            out.append([q, 0, n > tile])
            docs = 0
        out[-1][1] += 1
        docs += n
    return [(q0, nq) for q0, nq, _ in out]


@pytest.mark.parametrize("tile,lens", [(8, [4, 4, 3, 5, 8]), (8, [3, 9, 2, 2]), (8, [5, 3, 2]), (4, [1] * 6), (0, [300, 212, 1, 513, 512]), (100000, [512, 1])],
                         ids=["lists_fill_tiles", "tile_plus_1", "trailing_partial", "single_documents", "default_tile", "knob_above_default"])
def test_the_packing_of_the_host_header(tile, lens, tmp_path):
    exe = str(tmp_path / "xe_host_check")
    subprocess.check_call(["g++", "-std=c++17", os.path.join(ROOT, "tools", "xe_host_check.cpp"), "-o", exe])
    lines = subprocess.check_output([exe, str(tile)] + [str(n) for n in lens]).decode().splitlines()
    eff = int(lines[0].split()[1])
    assert eff == (tile if 0 < tile <= 512 else 512)
    assert [tuple(int(v) for v in ln.split()) for ln in lines[1:]] == _pack(lens, eff)
    assert tile != 8 or lens[0] != 4 or _pack(lens, 8) == [(0, 2), (2, 2), (4, 1)]


@pytest.mark.parametrize("args,match", [
    (["-train", "t.txt", "-ranker", "6", "-objective", "pairwise"], "-objective must be lambda or xendcg"),
    (["-train", "t.txt", "-ranker", "6", "-xeseed", "3"], "-xeseed s belongs to -objective xendcg"),
    (["-train", "t.txt", "-ranker", "6", "-objective", "lambda", "-xeseed", "3"], "-xeseed s belongs to -objective xendcg"),
    (["-train", "t.txt", "-ranker", "6", "-objective", "xendcg", "-xeseed", "-1"], "-xeseed must be an unsigned 64-bit number"),
    (["-load", "m.txt", "-test", "t.txt", "-objective", "xendcg"], "-objective is a way to train: it needs -train"),
    (["-train", "t.txt", "-ranker", "0", "-objective", "xendcg"], "ranking objective of -ranker 6.*not of -ranker 0"),
    (["-train", "t.txt", "-ranker", "4", "-objective", "xendcg"], "ranking objective of -ranker 6.*not of -ranker 4"),
    (["-train", "t.txt", "-ranker", "8", "-objective", "xendcg"], "bags of Random Forests.*trainers of their own"),
])
def test_the_command_line_refuses(args, match):
    with pytest.raises(N.RankLibError, match=match):
        evaluator.main(args)
    assert (LambdaMART.objective, LambdaMART.xeSeed) == ("lambda", 0)


def test_the_usage_text_the_statics_and_the_abi_names(capsys, monkeypatch):
    assert evaluator.main([]) == 0
    out = capsys.readouterr().out
    assert "[-objective lambda|xendcg [-xeseed s]]" in out and "-objective lambda|xendcg [-xeseed s] is an rlhip extension" in out
    monkeypatch.setattr(LambdaMART, "objective", "xendcg")
    with pytest.raises(N.RankLibError, match="bags of Random Forests"):
        RFRanker(features=[1]).init()
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    assert all("int %s(" % name in hdr and name in N.ABI_SYMBOLS for name in ("rl_set_objective", "rl_debug_xe_lambdas"))
    assert "RL_OBJECTIVE_LAMBDA = 0, RL_OBJECTIVE_XENDCG = 1" in hdr and N.OBJECTIVE == {"lambda": 0, "xendcg": 1}
