"""DART where it needs no device: the command line's usage errors, the restatement's weights by hand, the draw's determinism and
its host code (ranklib_amd/csrc/rl_dart_host.h through tools/dart_host_check.cpp) against the restatement."""
import os
import subprocess

import numpy as np
import pytest

import dart_restatement as DR
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd.learning import MART, LambdaMART, RFRanker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.mark.parametrize("args,match", [
    (["-train", "t.txt", "-ranker", "6", "-maxdrop", "3"], "-maxdrop n belongs to -dart rate"),
    (["-train", "t.txt", "-ranker", "6", "-dartseed", "3"], "-dartseed s belongs to -dart rate"),
    (["-train", "t.txt", "-ranker", "6", "-dart", "0"], r"-dart must be in \(0, 1\] \(got 0.0\)"),
    (["-train", "t.txt", "-ranker", "0", "-dart", "1.5"], r"-dart must be in \(0, 1\] \(got 1.5\)"),
    (["-train", "t.txt", "-ranker", "6", "-dart", "nan"], r"-dart must be in \(0, 1\] \(got nan\)"),
    (["-train", "t.txt", "-ranker", "6", "-dart", "0.1", "-maxdrop", "-1"], "-maxdrop must be >= 0"),
    (["-train", "t.txt", "-ranker", "6", "-dart", "0.1", "-dartseed", "-1"], "-dartseed must be an unsigned 64-bit number"),
    (["-load", "m.txt", "-test", "t.txt", "-dart", "0.1"], "-dart is a way to train: it needs -train"),
    (["-train", "t.txt", "-ranker", "4", "-dart", "0.1"], "-dart is built for the tree trainers.*not for -ranker 4"),
    (["-train", "t.txt", "-ranker", "8", "-dart", "0.1"], "bags of Random Forests.*trainers of their own"),
    (["-train", "t.txt", "-ranker", "6", "-dart", "0.1", "-resume", "m.txt"], "-dart together with -resume"),
    (["-train", "t.txt", "-ranker", "0", "-dart", "0.1", "-refit", "m.txt"], "-dart together with -refit"),
    (["-train", "t.txt", "-ranker", "6", "-dart"], "Missing value for -dart"),
])
def test_the_command_line_refuses(args, match):
    with pytest.raises(N.RankLibError, match=match):
        evaluator.main(args)
    assert (LambdaMART.dartRate, LambdaMART.dartMaxDrop, LambdaMART.dartSeed) == (0.0, 50, 0) and MART.dartRate == 0.0


def test_the_usage_text_and_the_class_statics(capsys, monkeypatch):
    assert evaluator.main([]) == 0
    out = capsys.readouterr().out
    assert "[-dart rate [-maxdrop n] [-dartseed s]] [-fastleaf]" in out and "-dart rate [-maxdrop n] [-dartseed s] is an rlhip extension" in out
    monkeypatch.setattr(LambdaMART, "dartRate", 0.1)
    with pytest.raises(N.RankLibError, match="bags of Random Forests"):
        RFRanker(features=[1]).init()


def test_two_rounds_by_hand():
    """k = 1, lr = 0.1: the new tree gets 0.1 / 1.1, the dropped one keeps 1 / 1.1 of its weight; s' takes all of it out, base puts the rest back"""
    lr = F32(0.1)
    assert DR.new_weights(0, 0.1, []) == (lr, [])
    w_m, (w0,) = DR.new_weights(1, 0.1, [lr])
    assert w_m == F32(float(lr) / (1.0 + float(lr))) and w0 == F32(float(lr) * float(F32(1.0 / (1.0 + float(lr)))))
    assert abs(float(w_m) - 0.1 / 1.1) < 1e-8 and abs(float(w0) - 0.1 / 1.1) < 1e-8
    out = np.array([2.0, -4.0], F32)
    s = float(lr) * out.astype(np.float64)
    sp, base = DR.thin(s, [out], [0], [lr], [w0])
    assert np.array_equal(sp, np.zeros(2)) and np.array_equal(base, float(w0) * out.astype(np.float64))


def test_the_draw_is_a_function_of_seed_and_round_and_the_host_code_draws_it(tmp_path):
    a = [DR.draw(7, m, 0.5, 0) for m in range(20)]
    assert a == [DR.draw(7, m, 0.5, 0) for m in range(20)] and a != [DR.draw(8, m, 0.5, 0) for m in range(20)]
    assert a[0] == [] and all(d == sorted(set(d)) and all(0 <= i < m for i in d) for m, d in enumerate(a))
    for m in range(1, 20):
        capped = DR.draw(7, m, 0.5, 2)
        assert len(capped) == min(2, len(a[m])) and set(capped) <= set(a[m])
    exe = str(tmp_path / "dart_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "dart_host_check.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().strip() == "ok"
    for rate, cap in ((0.5, 0), (0.5, 2), (0.12, 0)):
        w = []
        for m, line in enumerate(subprocess.check_output([exe, "7", str(rate), str(cap), "0.1", "20"]).decode().splitlines()):
            f = line.split()
            D = DR.draw(7, m, rate, cap)
            w_m, w_new = DR.new_weights(len(D), 0.1, [w[i] for i in D])
            for i, x in zip(D, w_new):
                w[i] = x
            w.append(w_m)
            assert [int(v) for v in f[f.index("dropped") + 1:f.index("weights")]] == D, (rate, cap, m)
            assert [int(v, 16) for v in f[f.index("weights") + 1:]] == [int(np.float32(x).view(np.uint32)) for x in w], (rate, cap, m)
