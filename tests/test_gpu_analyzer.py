"""The Analyzer's randomisation test on the GPU (rl_perm_test / k_perm_test, ranklib_amd/csrc/rl_perm.inc) against the
restatement (tests/analyzer_restatement.py).  No tolerance anywhere: every pDiff, every trueDiff and every count is compared bit for bit.
(One exception in kind, not in size: where the sums are NaN the payload bits are nobody's contract, the test asks for NaN and count 0.)"""
import logging
import os

import numpy as np
import pytest

import analyzer_restatement as R
from ranklib_amd import _native as N
from ranklib_amd import analyzer as A
from ranklib_amd import stats as S
from ranklib_amd.learning import java_double_str, java_round

pytestmark = pytest.mark.gpu

SEED = 20240229


def _values(n, k, seed):
    """base [n], targets [k][n]: random doubles of mixed magnitude (the sum order shows in the bits), a -0.0 among them"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    t = rng.standard_normal((k, n)) * 10.0 ** rng.integers(-6, 7, (k, n))
    b[rng.integers(0, n)] = -0.0
    t[:, rng.integers(0, n)] = -0.0
    return b, t


def _check(b, t, seed, begin, count):
    got_c, got_td, got_pd = N.perm_test(b, t, seed, begin, count, want_pdiff=True)
    assert got_pd.shape == (len(t), count)
    for k in range(len(t)):
        c, td, pd = R.perm_numpy(b, t[k], seed, begin, count)
        assert np.array_equal(got_pd[k].view(np.uint64), pd.view(np.uint64)), (k, int(np.argmax(got_pd[k] != pd)))
        assert np.float64(got_td[k]).view(np.uint64) == np.float64(td).view(np.uint64)
        assert int(got_c[k]) == c
    c2, td2, none = N.perm_test(b, t, seed, begin, count)          # without out_pdiff: the same counts
    assert none is None and np.array_equal(c2, got_c) and np.array_equal(td2, got_td)
    return got_c, got_pd


@pytest.mark.parametrize("n", [1, 9, 10, 11, 19, 20, 21, 63, 64, 65, 1000])
def test_every_length_around_the_chunk_of_ten(n):
    b, t = _values(n, 2, n)
    _check(b, t, SEED, 0, 257)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 10000])
def test_permutation_counts_around_the_wavefront_and_the_block(count):
    b, t = _values(21, 1, 7)
    _check(b, t, SEED, 0, count)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_target_counts(k):
    b, t = _values(33, k, 40 + k)
    c, pd = _check(b, t, -SEED, 5, 300)
    for i in range(k):                                   # a target's result does not depend on which others are in the launch
        ci, _, pdi = N.perm_test(b, t[i:i + 1], -SEED, 5, 300, want_pdiff=True)
        assert int(ci[0]) == int(c[i]) and np.array_equal(pdi[0], pd[i])


@pytest.mark.parametrize("begin", [0, 1, 12345, 3 * 10 ** 9])
def test_perm_begin_and_a_split_run(begin):
    b, t = _values(21, 2, 99)                            # D = 3: permutation 3e9 starts 1.8e10 LCG steps in, past 2^32
    c, pd = _check(b, t, 2 ** 63 - 1, begin, 300)
    c1, _, p1 = N.perm_test(b, t, 2 ** 63 - 1, begin, 130, want_pdiff=True)
    c2, _, p2 = N.perm_test(b, t, 2 ** 63 - 1, begin + 130, 170, want_pdiff=True)
    assert np.array_equal(c1 + c2, c) and np.array_equal(np.concatenate([p1, p2], axis=1), pd)


@pytest.mark.parametrize("seed", [0, 1, -1, 2 ** 63 - 1, -2 ** 63])
def test_seeds(seed):
    b, t = _values(25, 1, 3)
    _check(b, t, seed, 2, 130)


def test_the_literal_loop_agrees_too():
    b, t = _values(37, 1, 11)
    c, td, pd = N.perm_test(b, t, 5, 7, 150, want_pdiff=True)
    lc, ltd, lpd = R.perm_literal(b, t[0], 5, 7, 150)
    assert int(c[0]) == lc and td[0] == ltd and np.array_equal(pd[0].view(np.uint64), lpd.view(np.uint64))


def test_signed_zeros():
    b = np.array([-0.0, 0.0, -0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 0.0, -0.0, -0.0])
    t = np.array([[0.0, -0.0, -0.0, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 0.0, -0.0]])
    c, pd = _check(b, t, SEED, 0, 200)
    assert int(c[0]) == 200 and not pd.any()             # 0 >= 0: every permutation counts


def test_a_nan_entry_never_counts():
    b, t = _values(23, 2, 1)
    b[4] = np.nan
    c, td, pd = N.perm_test(b, t, SEED, 0, 300, want_pdiff=True)
    assert np.isnan(td).all() and np.isnan(pd).all() and not c.any()
    b2, t2 = _values(23, 2, 1)
    t2[1, 22] = np.nan                                   # the second target only
    c, td, pd = N.perm_test(b2, t2, SEED, 0, 300, want_pdiff=True)
    want = R.perm_numpy(b2, t2[0], SEED, 0, 300)
    assert int(c[0]) == want[0] and np.array_equal(pd[0], want[2]) and int(c[1]) == 0 and np.isnan(pd[1]).all() and np.isnan(td[1])


def test_target_equal_to_base_gives_exactly_one():
    b, _ = _values(48, 1, 8)
    c, pd = _check(b, b[None, :].copy(), SEED, 0, 1000)
    assert int(c[0]) == 1000 and not pd.any()
    assert int(c[0]) / 1000 == 1.0


def test_an_exact_tie_counts():
    # n = 1: either bit gives pDiff = |b - t| = trueDiff, a tie in every permutation
    c, pd = _check(np.array([0.1]), np.array([[0.7]]), SEED, 0, 500)
    assert int(c[0]) == 500 and (pd == abs(0.1 - 0.7)).all()
    # and among ordinary values: the permutations that swap nothing or everything tie with trueDiff, and are counted
    b, t = _values(3, 1, 6)
    c, td, pd = N.perm_test(b, t, SEED, 0, 400, want_pdiff=True)
    bits = R.perm_bits(3, SEED, 0, 400)
    same = ~bits.any(axis=1)
    assert same.any() and (pd[0][same] == td[0]).all()
    assert int(c[0]) == int(np.sum(pd[0] >= td[0])) >= int(same.sum())


def test_the_estimate_lies_within_the_binomial_error_of_the_exact_p():
    """does not lean on the restatement: for n = 10 the exact p over all 1024 sign patterns, in numpy; the GPU estimate at 100 000
    permutations must lie within 5 standard errors sqrt(p (1 - p) / np) of it"""
    rng = np.random.default_rng(12)
    b = rng.random(10)
    t = b + rng.standard_normal(10) * 0.2 + 0.03
    masks = ((np.arange(1024)[:, None] >> np.arange(10)[None, :]) & 1).astype(bool)
    pb, pt = np.where(masks, t, b), np.where(masks, b, t)
    diffs = np.abs(pb.mean(axis=1) - pt.mean(axis=1))
    true = abs(b.mean() - t.mean())
    assert np.min(np.abs(diffs - true)[(masks.any(axis=1)) & (~masks.all(axis=1))]) > 1e-9      # no near-tie a rounding could flip
    p = float(np.mean(diffs >= true - 1e-12))
    assert 0.2 < p < 0.8
    np_ = 100000
    c, _, _ = N.perm_test(b, t[None, :], 4242, 0, np_)
    assert abs(int(c[0]) / np_ - p) <= 5 * np.sqrt(p * (1 - p) / np_), (int(c[0]) / np_, p)


def test_refusals_name_the_argument():
    b, t = _values(5, 1, 0)
    for kw, word in ((dict(perm_count=0), "perm_count"), (dict(perm_begin=-1), "perm_begin"), (dict(perm_begin=2 ** 62), "overflow")):
        with pytest.raises(N.RankLibError) as e:
            N.perm_test(b, t, 0, **kw)
        assert word in str(e.value)


# ---- end to end: two hand-built models -> -test ... -idv -> the analyzer's main ---------------------------------------------------------
def _letor(path, n_queries=60):
    rng = np.random.default_rng(77)
    with open(path, "w") as f:
        for q in range(1, n_queries + 1):
            nd = int(rng.integers(4, 12))
            for d in range(nd):
                x = rng.random(3)
                label = int(min(4, max(0, round(2 * x[0] + 2 * x[1] * x[1] + rng.standard_normal() * 0.7))))
                f.write("%d qid:%d 1:%.6f 2:%.6f 3:%.6f # d%d\n" % (label, q, x[0], x[1], x[2], d))


def _read_plain(path):
    out = {}
    for line in open(path):
        _, key, val = line.split()
        out[key] = float(val)
    return out


def test_end_to_end_idv_files_through_the_analyzer(tmp_path, caplog):
    from ranklib_amd import evaluator
    data = tmp_path / "test.txt"
    _letor(str(data))
    runs = tmp_path / "runs"
    runs.mkdir()
    models = {"base.txt": "1:0.2 2:0.1 3:0.7", "sys_a.txt": "1:0.6 2:0.4 3:0.0", "sys_b.txt": "1:0.1 2:0.8 3:0.1"}
    for name, weights in models.items():
        m = tmp_path / (name + ".model")
        m.write_text("## Coordinate Ascent\n" + weights + "\n")
        assert evaluator.main(["-load", str(m), "-test", str(data), "-metric2t", "NDCG@10", "-idv", str(runs / name)]) == 0
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        assert A.main(["-all", str(runs), "-base", "base.txt", "-np", "1000", "-npseed", "7"]) == 0
    got = [r.getMessage() for r in caplog.records]

    base = _read_plain(runs / "base.txt")
    assert len(base) == 61 and "all" in base
    order = R.hashmap_order_closed_form(list(base.keys()))
    thr = [-1, -0.75, -0.5, -0.25, 0, 0.25, 0.5, 0.75, 1, 1000]
    want = ["Reading %s... 61 ranked lists" % (str(runs) + os.sep + n) for n in ("base.txt", "sys_a.txt", "sys_b.txt")]
    want += ["Overall comparison", "System\tPerformance\tImprovement\tWin\tLoss\tp-value",
             "base.txt [baseline]\t" + java_double_str(java_round(base["all"], 4))]
    rows = []
    for name in ("sys_a.txt", "sys_b.txt"):
        tg = _read_plain(runs / name)
        win = sum(1 for k in base if k != "all" and tg[k] > base[k])
        loss = sum(1 for k in base if k != "all" and tg[k] < base[k])
        hist = [0] * 10
        for k in base:
            ch = tg[k] - base[k]
            if k != "all" and ch != 0:
                hist[[i for i in range(4, 10) if ch <= thr[i]][0] if ch > 0 else [i for i in range(5) if ch < thr[i]][0]] += 1
        count = R.perm_numpy([base[k] for k in order], [tg[k] for k in order], 7, 0, 1000)[0]
        delta = tg["all"] - base["all"]
        plus = "+" if delta > 0 else ""
        want.append("%s\t%s\t%s%s (%s%s%%)\t%d\t%d\t%s" % (name, java_double_str(java_round(tg["all"], 4)), plus, java_double_str(java_round(delta, 4)),
                                                          plus, java_double_str(java_round(delta * 100 / base["all"], 2)), win, loss,
                                                          java_double_str(count / 1000)))
        rows.append(name + "".join("\t%d" % h for h in hist))
        assert win + loss > 10                           # the systems really differ
    want += ["Detailed break down",
             "\t[ < -100%)\t[-100%, -75%)\t[-75%, -50%)\t[-50%, -25%)\t[-25%, 0%)\t(0%, +25%]\t(+25%, +50%]\t(+50%, +75%]\t(+75%, +100%]\t( > +100%]"]
    assert got == want + rows
    assert (S.RandomPermutationTest.nPermutation, S.RandomPermutationTest.seed) == (10000, None)
