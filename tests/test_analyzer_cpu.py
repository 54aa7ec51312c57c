"""CPU-side checks of the Analyzer (ranklib_amd/analyzer.py, ranklib_amd/stats.py): HashMap order, the reader, compare and
its log text, SimpleMath.round, the LCG jump and the two forms of the restatement (tests/analyzer_restatement.py).  Where a p-value is
needed without a GPU, _native.perm_test is replaced by the restatement; the kernel itself is tests/test_gpu_analyzer.py's."""
import gzip
import logging

import numpy as np
import pytest

import analyzer_restatement as R
from ranklib_amd import _native as N
from ranklib_amd import analyzer as A
from ranklib_amd import stats as S
from ranklib_amd.learning import java_double_str, java_round


def _ids(k):
    """k entries: "1" .. str(k - 1), then "all" (what -idv writes)"""
    return [str(i) for i in range(1, k)] + ["all"]


# ---- HashMap order ------------------------------------------------------------------------------------------------------------------
def test_order_of_twelve_entries_by_hand():
    # no resize (size 12 is not > 12).  "1".."9" hash to 49..57 -> slots 1..9; "10" = 1567 -> 15; "11" = 1568 -> 0;
    # "all" = 96673 ^ 1 = 96672 -> 0, behind "11" which was put first
    assert S.java_hashmap_order(_ids(12)) == ["11", "all", "1", "2", "3", "4", "5", "6", "7", "8", "9", "10"]


def test_order_of_thirteen_entries_by_hand():
    # the 13th put doubles the table to 32: "1".."9" -> 17..25, "10" -> 31, "11" -> 0, "12" = 1569 -> 1, "all" -> 0
    assert S.java_hashmap_order(_ids(13)) == ["11", "all", "12", "1", "2", "3", "4", "5", "6", "7", "8", "9", "10"]


@pytest.mark.parametrize("k", [12, 13, 24, 25, 48, 49, 96, 97])
@pytest.mark.parametrize("style", ["plain", "q"])
def test_order_on_both_sides_of_every_resize(k, style):
    keys = _ids(k) if style == "plain" else ["q%05d" % i for i in range(k - 1)] + ["all"]
    got = S.java_hashmap_order(keys)
    assert sorted(got) == sorted(keys)
    assert got == R.hashmap_order_closed_form(keys)
    assert got != keys                                   # not file order, even for tiny files


def test_a_repeated_id_keeps_its_place(tmp_path):
    assert S.java_hashmap_order(["2", "1", "2", "3", "1"]) == S.java_hashmap_order(["2", "1", "3"])
    f = tmp_path / "dup.txt"
    f.write_text("NDCG@10   7   0.25\nNDCG@10   3   0.5\nNDCG@10   7   0.75\nNDCG@10   all   0.625\n")
    m = A.Analyzer().read(str(f))
    assert list(m.items()) == [("7", 0.75), ("3", 0.5), ("all", 0.625)]


def _colliding(n):
    """n distinct strings with one hashCode: "Aa" and "BB" hash alike, and so does every string built from such pairs"""
    out = []
    for i in range(n):
        out.append("".join("BB" if (i >> b) & 1 else "Aa" for b in range(4)))
    assert len({S.java_string_hash(s) for s in out}) == 1 and len(set(out)) == n
    return out


def test_the_ninth_node_of_a_bin_is_refused(tmp_path):
    assert len(S.java_hashmap_order(_colliding(8))) == 8
    f = tmp_path / "collide.txt"
    f.write_text("".join("P@1 %s 0.5\n" % s for s in _colliding(9)))
    with pytest.raises(N.RankLibError) as e:
        A.Analyzer().read(str(f))
    assert str(f) in str(e.value) and "bin" in str(e.value) and "ninth" in str(e.value)


def test_the_means_depend_on_the_order():
    """the order is really under test: with mixed magnitudes the hash-order sum and the file-order sum differ in bits"""
    rng = np.random.default_rng(5)
    keys = _ids(24)
    vals = {k: float(rng.standard_normal() * 10.0 ** int(rng.integers(-6, 7))) for k in keys}
    b, _ = S.RandomPermutationTest.arrays(vals, vals)
    assert b == [vals[k] for k in S.java_hashmap_order(keys)]
    assert S.BasicStats.mean(b) != S.BasicStats.mean([vals[k] for k in keys])
    assert S.BasicStats.mean(b) == R.mean(b)
    with pytest.raises(N.RankLibError):
        S.BasicStats.mean([])


# ---- the reader -----------------------------------------------------------------------------------------------------------------------
def test_reader_spaces_tabs_blank_lines_and_gz(tmp_path):
    text = "\n  NDCG@10     1   0.5  \nNDCG@10\ta\tb\t0.25\n\n \t \nNDCG@10 3 1.0E-5\r\nNDCG@10   all   0.375\n"
    f = tmp_path / "p.txt"
    f.write_text(text, newline="")
    want = {"1": 0.5, "a": None, "3": 1e-5, "all": 0.375}
    with pytest.raises(N.RankLibError) as e:            # a tab inside the name splits it: field 2 is "b"
        A.Analyzer().read(str(f))
    assert "line 3" in str(e.value) and "'b'" in str(e.value)
    f.write_text(text.replace("a\tb\t0.25", "a\t0.25\tb"), newline="")
    want["a"] = 0.25
    assert A.Analyzer().read(str(f)) == want
    g = tmp_path / "p.txt.gz"
    with gzip.open(str(g), "wt", encoding="utf-8") as z:
        z.write(text.replace("a\tb\t0.25", "a\t0.25\tb"))
    assert A.Analyzer().read(str(g)) == want


def test_reader_refuses_short_lines_and_bad_numbers(tmp_path):
    f = tmp_path / "short.txt"
    f.write_text("NDCG@10 1 0.5\nNDCG@10 2\n")
    with pytest.raises(N.RankLibError) as e:
        A.Analyzer().read(str(f))
    assert str(f) in str(e.value) and "line 2" in str(e.value)
    for bad in ("1_0", "nan", "inf", "-inf", "infinity", "0x1.8p1", "1e", "--1", "1.0dd", "", "١"):
        f.write_text("NDCG@10 1 0.5\n\nNDCG@10 2 %s x\n" % bad)
        with pytest.raises(N.RankLibError) as e:
            A.Analyzer().read(str(f))
        assert str(f) in str(e.value) and "line 3" in str(e.value), bad
    with pytest.raises(N.RankLibError):
        A.Analyzer().read(str(tmp_path / "missing.txt"))


def test_the_doubles_java_reads():
    p = A.parse_java_double
    assert p("0.5") == 0.5 and p("+.5") == 0.5 and p("5.") == 5.0 and p("-1.5e-3") == -0.0015 and p("1E3") == 1000.0
    assert p("1.0d") == 1.0 and p("2D") == 2.0 and p("3f") == 3.0 and p("4.5E1F") == 45.0 and p(" 7 ") == 7.0
    assert np.isnan(p("NaN")) and np.isnan(p("-NaN")) and p("Infinity") == np.inf and p("-Infinity") == -np.inf and p("+Infinity") == np.inf
    assert str(p("-0.0")) == "-0.0"
    for v in (0.1, 1e-5, 123456789.25, 5e-324, 1.7976931348623157e308, -2.5e-7):
        assert p(java_double_str(v)) == v
    with pytest.raises(ValueError) as e:
        p("0x1p3")
    assert "hexadecimal" in str(e.value)


# ---- compare ---------------------------------------------------------------------------------------------------------------------------
def _beside(v, up):
    return float(np.nextafter(v, np.inf if up else -np.inf))


def test_locate_segment_at_every_boundary():
    seg = A.Analyzer().locateSegment
    tiny = 5e-324
    # (0, .25] -> 5, (.25, .5] -> 6, (.5, .75] -> 7, (.75, 1] -> 8, (1, 1000] -> 9, above: -1
    for v, at, above in ((0.25, 5, 6), (0.5, 6, 7), (0.75, 7, 8), (1.0, 8, 9), (1000.0, 9, -1)):
        assert (seg(_beside(v, False)), seg(v), seg(_beside(v, True))) == (at, at, above)
    assert seg(tiny) == 5
    # value < -1 -> 0, [-1, -.75) -> 1, [-.75, -.5) -> 2, [-.5, -.25) -> 3, [-.25, 0) -> 4
    for v, below, at in ((-1.0, 0, 1), (-0.75, 1, 2), (-0.5, 2, 3), (-0.25, 3, 4)):
        assert (seg(_beside(v, False)), seg(v), seg(_beside(v, True))) == (below, at, at)
    assert seg(-tiny) == 4 and seg(-1e9) == 0
    assert seg(0.0) == -1 and seg(-0.0) == -1 and seg(float("nan")) == -1


def test_compare_counts_and_histogram():
    a = A.Analyzer()
    changes = [0.25, 0.2500000000000001, 0.5, 0.75, 1.0, 1.5, -0.25, -0.2500000000000001, -0.5, -0.75, -1.0, -1.5, 0.0]
    base = {str(i): 0.0 for i in range(len(changes))}          # change = pt - 0.0: exact
    base["all"] = 0.0
    tgt = {str(i): c for i, c in enumerate(changes)}
    tgt["all"] = 9.0                                    # "all" counts neither as a win nor in the histogram
    r = a.compare(base, tgt)
    assert (r.status, r.win, r.loss) == (0, 6, 6)
    assert r.countByImprovementRange == [1, 1, 1, 2, 1, 1, 2, 1, 1, 1]
    rs = a.compare(base, [tgt, base])
    assert [x.status for x in rs] == [0, 0] and rs[1].win == rs[1].loss == 0 and sum(rs[1].countByImprovementRange) == 0


def test_a_change_outside_every_range_is_an_error():
    a = A.Analyzer()
    with pytest.raises(N.RankLibError) as e:
        a.compare({"1": 0.0, "all": 0.0}, {"1": 1000.5, "all": 0.0})
    assert "'1'" in str(e.value)
    with pytest.raises(N.RankLibError):
        a.compare({"1": 0.0, "all": 0.0}, {"1": float("nan"), "all": 0.0})


def test_status_codes():
    a = A.Analyzer()
    base = {"1": 0.5, "2": 0.5, "all": 0.5}
    assert a.compare(base, {"1": 0.5, "all": 0.5}).status == -1
    assert a.compare(base, {"1": 0.5, "3": 0.5, "all": 0.5}).status == -2


def _fake_perm_test(monkeypatch, calls=None):
    def fake(base, targets, seed, perm_begin=0, perm_count=10000, want_pdiff=False, device=0):
        if calls is not None:
            calls.append((np.array(base), np.array(targets), seed, perm_begin, perm_count))
        out = [R.perm_numpy(base, t, seed, perm_begin, perm_count) for t in np.asarray(targets)]
        return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out]), None
    monkeypatch.setattr(S._native, "perm_test", fake)


def _write(path, rows):
    path.write_text("".join("NDCG@10   %s   %s\n" % (k, java_double_str(v)) for k, v in rows))


HEADER = ("\t[ < -100%)\t[-100%, -75%)\t[-75%, -50%)\t[-50%, -25%)\t[-25%, 0%)\t(0%, +25%]\t(+25%, +50%]\t(+50%, +75%]\t(+75%, +100%]"
          "\t( > +100%]")


def test_the_log_of_a_two_target_run(tmp_path, monkeypatch, caplog):
    calls = []
    _fake_perm_test(monkeypatch, calls)
    d = tmp_path / "runs"
    d.mkdir()
    base = [("1", 0.4), ("2", 0.6), ("3", 0.5), ("all", 0.5)]
    ta = [("1", 0.5), ("2", 0.3), ("3", 0.5), ("all", 0.45)]            # +0.1 -> (0%, +25%], -0.3 -> [-50%, -25%)
    tb = [("1", 0.9), ("2", 0.6), ("3", 2.0), ("all", 0.75)]            # +0.5 -> (+25%, +50%], +1.5 -> ( > +100%]
    _write(d / "base.txt", base)
    _write(d / "b_sys.txt", tb)
    _write(d / "a_sys.txt", ta)
    monkeypatch.setattr(S.RandomPermutationTest, "nPermutation", 200)
    monkeypatch.setattr(S.RandomPermutationTest, "seed", 11)
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        A.Analyzer().compare(str(d), "base.txt")
    order = ["all", "1", "2", "3"]                                      # slots 0, 1, 2, 3 of 16
    assert S.java_hashmap_order([k for k, _ in base]) == order
    pa = R.perm_literal([dict(base)[k] for k in order], [dict(ta)[k] for k in order], 11, 0, 200)[0] / 200
    pb = R.perm_literal([dict(base)[k] for k in order], [dict(tb)[k] for k in order], 11, 0, 200)[0] / 200
    p = str(d) + "/"
    assert [r.getMessage() for r in caplog.records] == [
        "Reading %sbase.txt... 4 ranked lists" % p,
        "Reading %sa_sys.txt... 4 ranked lists" % p,
        "Reading %sb_sys.txt... 4 ranked lists" % p,
        "Overall comparison",
        "System\tPerformance\tImprovement\tWin\tLoss\tp-value",
        "base.txt [baseline]\t0.5",
        "a_sys.txt\t0.45\t-0.05 (-10.0%)\t1\t1\t" + java_double_str(pa),
        "b_sys.txt\t0.75\t+0.25 (+50.0%)\t2\t0\t" + java_double_str(pb),
        "Detailed break down",
        HEADER,
        "a_sys.txt\t0\t0\t0\t1\t0\t1\t0\t0\t0\t0",
        "b_sys.txt\t0\t0\t0\t0\t0\t0\t1\t0\t0\t1",
    ]
    assert len(calls) == 1 and calls[0][1].shape == (2, 4) and calls[0][2:] == (11, 0, 200)          # one launch for both targets
    assert list(calls[0][0]) == [0.5, 0.4, 0.6, 0.5]                    # the "all" entry is part of the arrays, in HashMap order


def test_targets_that_are_not_comparable(tmp_path, monkeypatch, caplog):
    _fake_perm_test(monkeypatch)
    d = tmp_path / "runs"
    d.mkdir()
    _write(d / "base.txt", [("1", 0.4), ("2", 0.6), ("all", 0.5)])
    _write(d / "other_ids.txt", [("1", 0.4), ("9", 0.6), ("all", 0.5)])
    monkeypatch.setattr(S.RandomPermutationTest, "nPermutation", 50)
    monkeypatch.setattr(S.RandomPermutationTest, "seed", 1)
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        A.Analyzer().compare([str(d / "other_ids.txt")], str(d / "base.txt"))
    msgs = [r.getMessage() for r in caplog.records]
    warn = "WARNING: [%s] skipped: NOT comparable to the baseline due to different ranked list IDs." % str(d / "other_ids.txt")
    assert warn in msgs and [r.levelno for r in caplog.records if r.getMessage() == warn] == [logging.WARNING]
    assert msgs[-1].startswith("other_ids.txt\t")                       # status -2 still has a (partial) histogram row, as in the Java
    caplog.clear()
    _write(d / "fewer.txt", [("1", 0.4), ("all", 0.5)])
    with caplog.at_level(logging.INFO, logger="ranklib_amd"), pytest.raises(N.RankLibError) as e:
        A.Analyzer().compare([str(d / "fewer.txt")], str(d / "base.txt"))       # status -1: the Java's break-down dereferences null
    assert "fewer.txt" in str(e.value)
    assert ("WARNING: [%s] skipped: NOT comparable to the baseline due to different ranked list IDs." % str(d / "fewer.txt")) in \
        [r.getMessage() for r in caplog.records]


def test_a_missing_all_entry_is_an_error(tmp_path, monkeypatch):
    _fake_perm_test(monkeypatch)
    _write(tmp_path / "base.txt", [("1", 0.4), ("2", 0.6)])
    _write(tmp_path / "t.txt", [("1", 0.4), ("2", 0.7)])
    with pytest.raises(N.RankLibError) as e:
        A.Analyzer().compare([str(tmp_path / "t.txt")], str(tmp_path / "base.txt"))
    assert "'all'" in str(e.value) and "base.txt" in str(e.value)


def test_simple_math_round_at_a_half():
    assert java_round(0.125, 2) == 0.13 and java_round(-0.125, 2) == -0.12           # floor(x + .5): halves go up
    assert java_round(2.5, 0) == 3.0 and java_round(-2.5, 0) == -2.0 and java_round(0.00005, 4) in (0.0, 0.0001)
    assert java_double_str(A._round(0.03125, 4)) == "0.0313" and java_double_str(A._round(-0.03125, 4)) == "-0.0312"
    assert np.isnan(A._round(float("nan"), 4)) and A._round(float("inf"), 2) == np.inf and A._round(-1e308, 4) == -np.inf


# ---- the random stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, -1, 2 ** 63 - 1])
def test_lcg_jump_against_stepping(seed):
    for k in (0, 1, 2, 47, 1 << 20):
        r = R.JavaRandom(seed)
        for _ in range(k if k < 1000 else 0):
            r.next(32)
        if k >= 1000:                                   # stepped with numpy-free integer arithmetic, 2^20 steps
            s = r.state
            for _ in range(k):
                s = (s * R.A + R.C) & R.MASK
            r.state = s
        a, c = R.lcg_jump(k)
        assert (a * R.JavaRandom(seed).state + c) & R.MASK == r.state


@pytest.mark.parametrize("seed", [0, 1, -1, 2 ** 63 - 1])
def test_lcg_jumps_compose_above_2_to_the_32(seed):
    s0 = R.JavaRandom(seed).state
    for ka, kb in (((1 << 32) + 12345, (1 << 33) + 7), (3 * 10 ** 9 * 2002, 1), ((1 << 47) - 1, (1 << 47) + 5), ((1 << 62), (1 << 20))):
        a1, c1 = R.lcg_jump(ka)
        a2, c2 = R.lcg_jump(kb)
        a3, c3 = R.lcg_jump(ka + kb)
        assert (a2 * ((a1 * s0 + c1) & R.MASK) + c2) & R.MASK == (a3 * s0 + c3) & R.MASK
    assert R.lcg_jump(1 << 48) == (1, 0)                # the period
    assert R.random_at(seed, 5).state == R.random_at(seed, 5 + (1 << 47)).state


def test_java_random_known_values():
    """java.util.Random(42).nextInt() is -1170105035 and Random(0).nextDouble() 0.730967787376657 (widely published first draws)"""
    assert R.JavaRandom(42).next(32) == -1170105035
    assert R.JavaRandom(0).nextDouble() == 0.730967787376657


def test_the_ten_bits_are_a_shift_of_the_state():
    rng = np.random.default_rng(9)
    for s in [0, R.MASK, 1 << 47, (1 << 38) - 1] + [int(v) for v in rng.integers(0, 1 << 48, 20000)]:
        r = R.JavaRandom(0)
        r.state = s
        x = int((1 << 10) * r.nextDouble())
        first = (s * R.A + R.C) & R.MASK
        assert x == first >> 38 and 0 <= x < 1024


@pytest.mark.parametrize("n,begin,count", [(1, 0, 40), (9, 3, 33), (10, 0, 40), (11, 1, 40), (20, 0, 17), (21, 12345, 9), (37, 3 * 10 ** 9, 12)])
def test_literal_and_vectorised_restatement_agree(n, begin, count):
    rng = np.random.default_rng(n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-5, 6, n)
    t = rng.standard_normal(n) * 10.0 ** rng.integers(-5, 6, n)
    c1, d1, p1 = R.perm_literal(b, t, 17, begin, count)
    c2, d2, p2 = R.perm_numpy(b, t, 17, begin, count)
    assert (c1, d1) == (c2, d2) and np.array_equal(p1.view(np.uint64), p2.view(np.uint64))
    bits = R.perm_bits(n, 17, begin, count)
    r = R.random_at(17, begin * (n // 10 + 1))
    for i in range(count):
        assert "".join("1" if v else "0" for v in bits[i]) == R.random_bit_vector(r, n)[:n]
    # a split run is the whole run
    h = count // 2
    assert np.array_equal(np.concatenate([R.perm_numpy(b, t, 17, begin, h)[2], R.perm_numpy(b, t, 17, begin + h, count - h)[2]]), p2)


def test_test_all_is_test_per_target(monkeypatch):
    _fake_perm_test(monkeypatch)
    monkeypatch.setattr(S.RandomPermutationTest, "nPermutation", 64)
    monkeypatch.setattr(S.RandomPermutationTest, "seed", -3)
    rng = np.random.default_rng(2)
    keys = _ids(30)
    base = {k: float(rng.random()) for k in keys}
    tg = [{k: float(rng.random()) for k in keys} for _ in range(3)]
    t = S.RandomPermutationTest()
    assert t.test_all(tg, base) == [t.test(x, base) for x in tg]
    assert t.test(base, base) == 1.0
    monkeypatch.setattr(S.RandomPermutationTest, "nPermutation", 0)
    assert np.isnan(t.test(tg[0], base))


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_usage_text(caplog):
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        assert A.main(["-np"]) == 0
    assert [r.getMessage() for r in caplog.records] == [
        "Usage: java -cp bin/RankLib.jar ciir.umass.edu.eval.Analyzer <Params>",
        "Params:",
        "\t-all <directory>\tDirectory of performance files (one per system)",
        "\t-base <file>\t\tPerformance file for the baseline (MUST be in the same directory)",
        "\t[ -np ] \t\tNumber of permutation (Fisher randomization test) [default=10000]",
        "\t[ -npseed ] \t\tSeed of the permutations' java.util.Random (rlhip extension) [default=drawn and logged]",
    ]


def test_main_sets_and_restores_the_statics(tmp_path, monkeypatch, caplog):
    seen = []

    def fake(base, targets, seed, perm_begin=0, perm_count=10000, want_pdiff=False, device=0):
        seen.append((seed, perm_count, S.RandomPermutationTest.nPermutation, S.RandomPermutationTest.seed))
        return np.zeros(len(targets), np.int64), np.zeros(len(targets)), None
    monkeypatch.setattr(S._native, "perm_test", fake)
    _write(tmp_path / "base.txt", [("1", 0.4), ("all", 0.4)])
    _write(tmp_path / "sys.txt", [("1", 0.5), ("all", 0.5)])
    before = (S.RandomPermutationTest.nPermutation, S.RandomPermutationTest.seed)
    assert before == (10000, None)
    assert A.main(["-all", str(tmp_path), "-base", "base.txt", "-np", "123", "-npseed", "-9"]) == 0
    assert seen == [(-9, 123, 123, -9)]
    assert (S.RandomPermutationTest.nPermutation, S.RandomPermutationTest.seed) == before
    with pytest.raises(N.RankLibError):
        A.main(["-all", str(tmp_path / "nowhere"), "-base", "base.txt", "-np", "77", "-npseed", "5"])
    assert (S.RandomPermutationTest.nPermutation, S.RandomPermutationTest.seed) == before
    with pytest.raises(N.RankLibError):
        A.main(["-all", str(tmp_path), "-base", "base.txt", "-np", "1_0"])
    # without -npseed the seed is drawn and logged, so the run can be repeated
    seen.clear()
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        A.main(["-all", str(tmp_path), "-base", "base.txt", "-np", "5"])
    logged = [r.getMessage() for r in caplog.records if r.getMessage().startswith("npseed = ")]
    assert len(logged) == 1 and int(logged[0][len("npseed = "):]) == seen[0][0] and -2 ** 63 <= seen[0][0] < 2 ** 63


def test_no_cpu_fallback_and_the_refusals(gpu_available):
    if not gpu_available:
        with pytest.raises(N.RankLibError) as e:
            S.RandomPermutationTest().test({"1": 0.5, "all": 0.5}, {"1": 0.25, "all": 0.25})
        assert "no CPU fallback" in str(e.value)
    # the argument checks come before the device is looked at
    for kw, word in ((dict(perm_count=0), "perm_count"), (dict(perm_begin=-1), "perm_begin"), (dict(perm_begin=2 ** 62, perm_count=5), "overflow")):
        with pytest.raises(N.RankLibError) as e:
            N.perm_test(np.zeros(3), np.zeros((1, 3)), 0, **kw)
        assert word in str(e.value)
    with pytest.raises(N.RankLibError) as e:
        N.perm_test(np.zeros(0), np.zeros((1, 0)), 0)
    assert "n must be" in str(e.value)
    with pytest.raises(N.RankLibError) as e:
        N.perm_test(np.zeros(3), np.zeros((0, 3)), 0)
    assert "n_targets" in str(e.value)
