"""The command lines DESIGN.md 22 adds, where no device is needed: DataPoint.toString and FeatureManager.save (both writers), the
FeatureManager command line (shuffle, folds, splits), FeatureStats, the Combiner, and how evaluator.main reads repeated -load / -test and
dispatches.  Every expected text is written out here from the Java source (no JVM exists in this environment); nothing is compared with
what the code under test itself produced."""
import logging
import os

import numpy as np
import pytest

import ca_restatement as CR
import tree_models as T
from ranklib_amd import _native as N
from ranklib_amd import combiner, evaluator, features
from ranklib_amd.evaluator import Evaluator
from ranklib_amd.feature_stats import FeatureStats, java_format_2f
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, JavaRandom, RankerFactory, RankerType, RankList, RFRanker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "featstats")


# ---- DataPoint.toString (learning/DataPoint.java:188-199) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("line, want", [
    # a gap in the ids, Float.toString in E-notation and as 1.0, a fractional label cast to int
    ("2.7 qid:q1 1:0.5 3:0.00001 4:1 # doc a", "2 qid:q1 1:0.5 3:1.0E-5 4:1.0 # doc a"),
    ("0 qid:7 1:3", "0 qid:7 1:3.0 "),                                   # no description: the space before it stays
    ("1 qid:x # d", "1 qid:x  # d"),                                     # no features: the space after the id and the one before the description
    ("1 qid:x", "1 qid:x  "),
    ("3 qid:9 1:0.25 2:NaN #z", "3 qid:9 1:0.25  #z"),                   # a literal NaN last: its separator goes with it, the one before stays
    ("4 qid:9 1:NaN 2:0.125 #z", "4 qid:9 2:0.125 #z"),
    ("0 qid:a:b 2:-1.5e10 3:12345678 #", "0 qid:b 2:-1.5E10 3:1.2345678E7 #"),
])
def test_datapoint_tostring(line, want):
    assert DataPoint(line).toString() == want


def random_points(seed, n=200):
    """rows with NaN cells inside, no features at all, empty descriptions, fractional labels; the last cell is a number, so that parsing
    the line gives the row's length back"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(0, 9))
        bits = rng.integers(0, 1 << 32, k + 1, dtype=np.uint64).astype(np.uint32)
        fv = bits.view(np.float32).copy()
        fv[~np.isfinite(fv)] = np.float32(0.1)
        small = rng.random(k + 1) < 0.4
        fv[small] = (rng.integers(-2000, 2000, int(small.sum())) / 8.0).astype(np.float32)      # everyday values beside the arbitrary bit patterns
        if k:
            gone = rng.random(k + 1) < 0.25
            gone[k] = False
            fv[gone] = np.nan
            if i % 17 == 0:
                fv[k] = np.inf
        fv[0] = np.nan
        label = float(np.float32([0, 1, 2, 3.5, 2.7, 4][int(rng.integers(0, 6))]))
        out.append(DataPoint.from_parsed(label, "q%d" % (i // 7), "" if i % 5 == 0 else "#docid = d%d x" % i, fv))
    return out


def test_parse_of_tostring_gives_the_point_back():
    for dp in random_points(5):
        back = DataPoint(dp.toString())
        assert back.label == float(int(dp.label)) and back.id == dp.id and back.description == dp.description
        assert back.fVals.dtype == np.float32 and np.array_equal(back.fVals.view(np.uint32), np.asarray(dp.fVals, np.float32).view(np.uint32)), dp.toString()


# ---- the two writers ------------------------------------------------------------------------------------------------------------------------------
def _lists(points):
    out, cur = [], []
    for dp in points:
        if cur and cur[-1].id != dp.id:
            out.append(RankList(cur)); cur = []
        cur.append(dp)
    out.append(RankList(cur))
    return out


def _native_writer_or_skip():
    try:
        if not hasattr(N.lib(), "rl_letor_format"):
            pytest.skip("this librlhip.so has no rl_letor_format")
    except N.RankLibError:
        pytest.skip("librlhip.so does not load")


def test_python_writer_is_tostring_and_a_newline(tmp_path, monkeypatch):
    pts = random_points(6, 40)
    monkeypatch.setattr(FeatureManager, "native", False)
    FeatureManager.save(_lists(pts), str(tmp_path / "py.txt"))
    assert open(tmp_path / "py.txt", "rb").read() == "".join(dp.toString() + "\n" for dp in pts).encode()


@pytest.mark.parametrize("shape", ["ragged", "uniform", "chunks"])
def test_native_writer_equals_the_python_writer(shape, tmp_path, monkeypatch):
    _native_writer_or_skip()
    pts = random_points(7, 300)
    if shape == "uniform":                                   # rows of one length take the stacked path
        pts = [dp for dp in pts if len(dp.fVals) == 6]
        assert len(pts) > 10
    if shape == "chunks":
        monkeypatch.setattr(FeatureManager, "SAVE_CHUNK", 64)
        pts[70].id = "qé"                               # one chunk is not ASCII: it alone goes through the Python writer
    calls = []
    real = N.letor_format
    monkeypatch.setattr(N, "letor_format", lambda *a, **kw: (calls.append(len(a[1])), real(*a, **kw))[1])
    FeatureManager.save(_lists(pts), str(tmp_path / "native.txt"))
    assert calls == ([len(pts)] if shape != "chunks" else [64, 64, 64, 300 - 4 * 64])
    monkeypatch.setattr(FeatureManager, "native", False)
    FeatureManager.save(_lists(pts), str(tmp_path / "py.txt"))
    assert len(calls) == (1 if shape != "chunks" else 4)
    got, want = open(tmp_path / "native.txt", "rb").read(), open(tmp_path / "py.txt", "rb").read()
    assert got == want and got.count(b"\n") == len(pts)


def test_native_writer_refuses_rows_and_strings_out_of_bounds():
    _native_writer_or_skip()
    X = np.zeros((2, 3), np.float32)
    ok = dict(row_len=[3, 3], labels=[0, 1], strings=b"q1q2", qid_off=[0, 2], qid_len=[2, 2], desc_off=[0, 0], desc_len=[0, 0])
    assert bytes(N.letor_format(X, **ok)) == b"0 qid:q1 1:0.0 2:0.0 \n1 qid:q2 1:0.0 2:0.0 \n"
    for bad in (dict(row_len=[3, 4]), dict(row_len=[-1, 3]), dict(qid_off=[0, 3]), dict(desc_off=[0, 5]), dict(desc_len=[0, -1]), dict(qid_len=[2, 9])):
        with pytest.raises(N.RankLibError, match="letor_format"):
            N.letor_format(X, **dict(ok, **bad))


# ---- the FeatureManager command line (features/FeatureManager.java:37-169) ----------------------------------------------------------------------------
LENS = [2, 1, 3, 2, 1, 2, 3, 1, 2, 2]


def list_text(q):
    """list q as save writes it, so that an output file is a concatenation of these"""
    return "".join("%d qid:q%d 1:%s 2:0.25 4:%d.0 #d%d_%d\n" % ((q + j) % 3, q, ("0.5", "1.0E-5", "3.0")[j], q, q, j) for j in range(LENS[q]))


def text_of(order):
    return "".join(list_text(q) for q in order)


@pytest.fixture
def ten(tmp_path):
    src = tmp_path / "in" / "ten.txt"
    src.parent.mkdir()
    src.write_text("# ten lists\n" + text_of(range(10)))
    out = tmp_path / "out"
    out.mkdir()
    return str(src), str(out)


def files_of(out):
    return {n: open(os.path.join(out, n)).read() for n in sorted(os.listdir(out))}


def java_shuffle(n, seed):
    rnd, lst = JavaRandom(seed), list(range(n))
    for i in range(n, 1, -1):
        j = rnd.nextInt(i)
        lst[i - 1], lst[j] = lst[j], lst[i - 1]
    return lst


@pytest.mark.parametrize("native", [True, False])
def test_shuffle_with_a_seed(ten, native, monkeypatch, tmp_path):
    src, out = ten
    monkeypatch.setattr(FeatureManager, "native", native)
    perm = java_shuffle(10, 1)
    assert perm == [6, 9, 7, 8, 4, 2, 0, 3, 1, 5]            # pinned: a change to JavaRandom shows here
    assert CR.shuffle(list(range(10)), CR.JavaRandom(1)) == perm          # ... and the tests' own java.util.Random agrees
    assert features.main(["-input", src, "-output", out, "-shuffle", "-seed", "1"]) == 0
    assert files_of(out) == {"ten.txt.shuffled": text_of(perm)}          # whole lists moved: the documents inside each keep their order
    again = tmp_path / "again"
    again.mkdir()
    features.main(["-INPUT", src, "-Output", str(again) + os.sep, "-Shuffle", "-SEED", "1"])
    assert files_of(str(again)) == files_of(out)


def test_shuffle_without_a_seed_logs_the_one_it_drew(ten, caplog):
    src, out = ten
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        features.main(["-input", src, "-output", out, "-shuffle"])
    seeds = [int(r.getMessage().split(" = ")[1]) for r in caplog.records if r.getMessage().startswith("seed = ")]
    assert len(seeds) == 1
    assert files_of(out) == {"ten.txt.shuffled": text_of(java_shuffle(10, seeds[0]))}


def test_k_folds(ten, caplog):
    src, out = ten
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        features.main(["-input", src, "-output", out, "-k", "3"])
    tests = [[0, 1, 2], [3, 4, 5], [6, 7, 8, 9]]
    want = {}
    for f, t in enumerate(tests):
        want["f%d.test.ten.txt" % (f + 1)] = text_of(t)
        want["f%d.train.ten.txt" % (f + 1)] = text_of([q for q in range(10) if q not in t])
    assert files_of(out) == want
    log = [r.getMessage() for r in caplog.records]
    at = log.index("Test[2]=")                               # printQueriesForSplit :413-428
    assert log[at:at + 5] == ["Test[2]=", ' "q6"', ' "q7"', ' "q8"', ' "q9"'] and "Train[0]=" in log and "Validate[0]=" not in log
    assert "Saving fold 3/3... " in log


@pytest.mark.parametrize("tvs", ["0.8", "0.5"])
def test_k_folds_with_a_validation_split(ten, tvs):
    src, out = ten
    features.main(["-input", src, "-output", out, "-k", "3", "-tvs", tvs])
    keep = 1.0 - float(np.float32(tvs))                      # the Java holds -tvs in a float and computes 1.0 - tvs in double
    want = {}
    for f, t in enumerate([[0, 1, 2], [3, 4, 5], [6, 7, 8, 9]]):
        train = [q for q in range(10) if q not in t]
        n_val = int(len(train) * keep)
        assert n_val == ({"0.8": 1, "0.5": 3}[tvs])
        vali = [train.pop() for _ in range(n_val)]           # from the end of train, back to front
        want["f%d.test.ten.txt" % (f + 1)] = text_of(t)
        want["f%d.train.ten.txt" % (f + 1)] = text_of(train)
        want["f%d.validation.ten.txt" % (f + 1)] = text_of(vali)
    assert files_of(out) == want


def test_train_test_split(ten):
    src, out = ten
    features.main(["-input", src, "-output", out, "-tts", "0.75"])
    assert files_of(out) == {"train.ten.txt": text_of(range(7)), "test.ten.txt": text_of(range(7, 10))}


def test_shuffle_then_folds_use_the_shuffled_name_and_order(ten):
    src, out = ten
    features.main(["-input", src, "-output", out, "-shuffle", "-seed", "1", "-k", "2"])
    perm = java_shuffle(10, 1)
    assert files_of(out) == {"ten.txt.shuffled": text_of(perm),
                             "f1.test.ten.txt.shuffled": text_of(perm[:5]), "f1.train.ten.txt.shuffled": text_of(perm[5:]),
                             "f2.test.ten.txt.shuffled": text_of(perm[5:]), "f2.train.ten.txt.shuffled": text_of(perm[:5])}


def test_several_inputs_are_read_in_order_and_named_after_the_first(ten, tmp_path):
    src, out = ten
    more = tmp_path / "in" / "more.txt"
    more.write_text("1 qid:zz 1:2.0 #m\n")
    features.main(["-input", src, "-input", str(more), "-output", out, "-tts", "0.5", "-unknown"])
    assert files_of(out) == {"train.ten.txt": text_of(range(5)), "test.ten.txt": text_of(range(5, 10)) + "1 qid:zz 1:2.0 #m\n"}


def test_k_with_tts_and_an_empty_input_write_nothing(ten, tmp_path, caplog):
    src, out = ten
    empty = tmp_path / "in" / "empty.txt"
    empty.write_text("# nothing\n\n")
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        assert features.main(["-input", src, "-output", out, "-k", "3", "-tts", "0.5"]) == 0
        assert features.main(["-input", str(empty), "-output", out, "-k", "3"]) == 0
        assert features.main(["-input", str(empty), "-output", out, "-shuffle"]) == 0
    assert files_of(out) == {}
    log = [r.getMessage() for r in caplog.records]
    assert log.count("Error: Only one of k or tts should be specified.") == 1 and log.count("Error: The input file is empty.") == 2


def test_without_output_the_files_go_to_the_working_directory(ten, tmp_path, monkeypatch):
    src, _ = ten
    here = tmp_path / "cwd"
    here.mkdir()
    monkeypatch.chdir(here)
    features.main(["-input", src, "-tts", "0.75", "-x"])
    assert sorted(os.listdir(here)) == ["test.ten.txt", "train.ten.txt"]


# ---- FeatureStats (features/FeatureStats.java:121-192) ---------------------------------------------------------------------------------------------------
def stats_log(path, caplog):
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        assert features.main(["-feature_stats", path]) == 0
    return [r.getMessage() for r in caplog.records]


def summary(n, lo, hi, med, avg, var, std):
    return ["Total Features Used: %d" % n, "Min frequency    : " + lo.rjust(10), "Max frequency    : " + hi.rjust(10), "Median frequency : " + med.rjust(10),
            "Avg frequency    : " + avg.rjust(10), "Variance         : " + var.rjust(10), "STD              : " + std.rjust(10)]


def test_feature_stats_lambdamart_two_trees(caplog):
    # tree 1 splits on 1 2 3 4, tree 2 on 5 6 7 8 1: eight frequencies, seven 1 and one 2.  Mean 9 / 8 = 1.125 and variance
    # (7 * 0.125^2 + 0.875^2) / 7 = 0.125 are exact in binary and ties of %10.2f: HALF_UP prints 1.13 and 0.13 (Python's % gives 1.12, 0.12)
    path = os.path.join(GOLDEN, "lambdamart_two_trees.txt")
    assert stats_log(path, caplog) == ["Model File: " + path, "Algorithm : LambdaMART", "Feature frequencies : ",
                                       "\tFeature[1] :       2"] + ["\tFeature[%d] :       1" % f for f in range(2, 9)] + \
        summary(8, "1.00", "2.00", "1.00", "1.13", "0.13", "0.35")
    assert "%10.2f" % 1.125 == "      1.12"


def test_feature_stats_random_forests_two_bags(caplog):
    # feature 3 in both bags, feature 7 in the second: an even count, the median is interpolated between 1 and 2
    path = os.path.join(GOLDEN, "random_forests_two_bags.txt")
    assert stats_log(path, caplog) == ["Model File: " + path, "Algorithm : Random Forests", "Feature frequencies : ", "\tFeature[3] :       2",
                                       "\tFeature[7] :       1"] + summary(2, "1.00", "2.00", "1.50", "1.50", "0.50", "0.71")


def test_feature_stats_adarank_counts_a_repeated_feature(caplog):
    # 2 2 2 5 9: frequencies 3 1 1; mean 5 / 3, variance (16/9 + 4/9 + 4/9) / 2 = 4 / 3
    path = os.path.join(GOLDEN, "adarank_repeated_feature.txt")
    assert stats_log(path, caplog) == ["Model File: " + path, "Algorithm : AdaRank", "Feature frequencies : ", "\tFeature[2] :       3",
                                       "\tFeature[5] :       1", "\tFeature[9] :       1"] + summary(3, "1.00", "3.00", "1.00", "1.67", "1.33", "1.15")


def test_feature_stats_rankboost_one_feature(caplog):
    path = os.path.join(GOLDEN, "rankboost_one_feature.txt")
    assert stats_log(path, caplog) == ["Model File: " + path, "Algorithm : RankBoost", "Feature frequencies : ", "\tFeature[4] :       2"] + \
        summary(1, "2.00", "2.00", "2.00", "2.00", "0.00", "0.00")


def test_feature_stats_a_mean_ending_in_375(tmp_path, caplog):
    # feature 1 four times and 2 .. 8 once: mean 11 / 8 = 1.375, variance (2.625^2 + 7 * 0.375^2) / 7 = 1.125, both exact ties
    path = tmp_path / "ada.txt"
    path.write_text("## AdaRank\n## Iteration = 500\n1:0.5 2:0.5 1:0.25 3:1.0 4:1.0 1:0.125 5:1.0 6:1.0 7:1.0 1:0.0625 8:1.0\n")
    assert stats_log(str(path), caplog)[-7:] == summary(8, "1.00", "4.00", "1.00", "1.38", "1.13", "1.06")


def test_feature_stats_refusals(tmp_path, caplog):
    ca = tmp_path / "ca.txt"
    ca.write_text("## Coordinate Ascent\n## Restart = 5\n1:0.5 2:0.25\n")
    assert stats_log(str(ca), caplog) == ["Coordinate Ascent uses all features.  Can't do selected model statistics for this algorithm."]
    four = tmp_path / "four.txt"
    four.write_text("## Random Forests v2\n1:0.5\n")
    with pytest.raises(N.RankLibError, match=r"^No model name defined\.  Quitting\.$"):
        FeatureStats(str(four)).writeFeatureStats()
    bad = tmp_path / "bad.txt"
    bad.write_text("## AdaRank\n1:0.5  2:0.25\n")            # two spaces: the Java's split leaves an empty token, Integer.valueOf refuses it
    with pytest.raises(N.RankLibError, match="NumberFormatException"):
        FeatureStats(str(bad)).writeFeatureStats()


def test_format_2f_rounds_half_up_on_exact_ties():
    assert [java_format_2f(v).strip() for v in (0.125, 0.375, 2.625, -0.125, 0.0, 1234567.875, 0.12)] == \
        ["0.13", "0.38", "2.63", "-0.13", "0.00", "1234567.88", "0.12"]
    assert len(java_format_2f(1.0)) == 10 and len(java_format_2f(123456789.0)) == 12


# ---- the Combiner (learning/Combiner.java:28-45) -----------------------------------------------------------------------------------------------------------
RF_HEADER = ("## Random Forests\n## No. of bags = 1\n## Sub-sampling = 1.0\n## Feature-sampling = 0.3\n## No. of trees = 1\n## No. of leaves = 10\n"
             "## No. of threshold candidates = 256\n## Learning rate = 0.1\n\n")


def ensemble_block(trees):
    text = T.model_text(trees, np.ones(len(trees), np.float32))
    return text[text.index("<ensemble>"):]


def one_bag_files(d):
    a = ensemble_block([T.flatten(T.S(2, 0.25, T.L(-1.0), T.L(2.0)))])
    b = ensemble_block([T.flatten(T.S(1, 1.0, T.L(0.0), T.S(3, 0.5, T.L(0.375), T.L(1.0)))), T.flatten(T.L(0.25))])
    os.makedirs(d)
    with open(os.path.join(d, "bag_b.txt"), "w") as f:      # written first: the order in the output is the names', not the directory's
        f.write(RF_HEADER + b)
    with open(os.path.join(d, "bag_a.txt"), "w") as f:
        f.write(RF_HEADER + a)
    with open(os.path.join(d, "x.progress"), "w") as f:
        f.write("not a model\n")
    return a, b


def test_combiner_merges_the_bags_in_name_order(tmp_path):
    d = str(tmp_path / "bags")
    a, b = one_bag_files(d)
    out = str(tmp_path / "forest.txt")
    assert combiner.main([d, out]) == 0
    text = open(out).read()
    assert text == "## Random Forests\n" + a + b
    # what RankerFactory and RFRanker.loadFromString read from it, short of building the bags on a device (tests/test_gpu_cmdline.py loads it)
    assert RankerFactory().names[text.split("\n", 1)[0].replace("## ", "").strip().upper()] == "RANDOM_FOREST"
    assert [blk + "\n" for blk in RFRanker.ensembleBlocks(text)] == [a, b]


def test_combiner_names_a_file_that_is_no_random_forests_model(tmp_path):
    d = str(tmp_path / "bags")
    one_bag_files(d)
    with open(os.path.join(d, "bag_c.txt"), "w") as f:
        f.write(T.model_text([T.flatten(T.L(1.0))], [1.0]))  # "## LambdaMART"
    with pytest.raises(N.RankLibError, match="bag_c.txt is not a Random Forests model"):
        combiner.main([d, str(tmp_path / "forest.txt")])
    assert not os.path.exists(tmp_path / "forest.txt")


# ---- evaluator.main: repeated -load / -test and the dispatch (eval/Evaluator.java:492-545) -----------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []
    for name in ("test", "score", "rank", "testWithScoreFile"):
        monkeypatch.setattr(Evaluator, name, lambda self, *a, _n=name: seen.append((_n,) + a))
    return seen


@pytest.mark.parametrize("argv, want", [
    (["-load", "m", "-test", "t", "-idv", "p"], ("test", "m", "t", "p")),                              # one model: as before
    (["-load", "m", "-test", "t"], ("test", "m", "t", "")),
    (["-load", "m", "-rank", "r", "-score", "s"], ("score", "m", "r", "s")),
    (["-load", "m", "-rank", "r", "-indri", "i"], ("rank", "m", "r", "i")),
    (["-load", "m", "-rank", "r", "-indri", "i", "-score", "s"], ("rank", "m", "r", "i")),           # one model, both: -indri goes on winning
    (["-load", "m", "-test", "t1", "-test", "t2"], ("test", "m", "t2", "")),                          # testFile is the last one
    (["-load", "a", "-load", "b", "-LOAD", "c", "-test", "t", "-idv", "p"], ("test", ["a", "b", "c"], "t", "p")),
    (["-load", "a", "-load", "b", "-test", "t1", "-test", "t2"], ("test", ["a", "b"], ["t1", "t2"], "")),
    (["-load", "a", "-load", "b", "-rank", "r", "-score", "s"], ("score", ["a", "b"], "r", "s")),
    (["-load", "a", "-load", "b", "-rank", "r", "-indri", "i"], ("rank", ["a", "b"], "r", "i")),
    (["-load", "a", "-load", "b", "-rank", "r", "-indri", "i", "-score", "s"], ("score", ["a", "b"], "r", "s")),   # several: the Java's order (:499-505)
    (["-test", "t", "-idv", "p", "-metric2T", "MAP"], ("test", None, "t", "p")),                      # no model
    (["-test", "t", "-score", "s"], ("testWithScoreFile", "t", "s")),
    (["-rank", "r", "-indri", "i"], ("rank", "r", "i")),
])
def test_main_dispatch(argv, want, calls):
    assert evaluator.main(argv) == 0
    assert calls == [want]


@pytest.mark.parametrize("argv", [["-rank", "r"], ["-load", "m", "-rank", "r"], ["-load", "a", "-load", "b", "-rank", "r"]])
def test_rank_alone_is_the_removed_function(argv, calls):
    with pytest.raises(N.RankLibError) as e:
        evaluator.main(argv)
    assert str(e.value) == ("This function has been removed.\nConsider using -score in addition to your current parameters, "
                            "and do the ranking yourself based on these scores.")
    assert calls == []


def test_nothing_to_do_still_returns(calls):
    assert evaluator.main(["-metric2t", "MAP"]) == 0 and calls == []


def test_score_file_errors_name_the_line_or_the_counts(ten, tmp_path):
    src, _ = ten
    e = Evaluator(RankerType.LAMBDAMART, "NDCG@10", "NDCG@10")
    n_docs = sum(LENS)
    own = tmp_path / "own.txt"                               # the flow's own -score output is no input to it, as in the Java
    own.write_text("".join("1\t%d\t0.5\n" % j for j in range(n_docs)))
    with pytest.raises(N.RankLibError, match=r"own\.txt, line 1: .*is not a Java double"):
        e.testWithScoreFile(src, str(own))
    short = tmp_path / "short.txt"
    short.write_text("\n".join("0.5" for _ in range(n_docs - 1)) + "\n\n")
    with pytest.raises(N.RankLibError, match=r"holds %d scores, .* holds %d documents" % (n_docs - 1, n_docs)):
        e.testWithScoreFile(src, str(short))
    with pytest.raises(N.RankLibError, match="2 models were given and only 1 test files"):
        e.test(["a", "b"], [src], "")
