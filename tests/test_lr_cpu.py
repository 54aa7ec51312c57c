"""Linear Regression (-ranker 9) without a GPU: the restatement of LinearRegRank.learn / solve / eval against cases computed by hand, its
two forms of the accumulation, the model text, RankerFactory, the command line, and the refusal without a device."""
import numpy as np
import pytest

import lr_restatement as LR
from conftest import has_gpu
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd._native import RankLibError
from ranklib_amd.learning import LambdaMART, LinearRegRank, RankerFactory, RankerType


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = (LinearRegRank.lambda_, LinearRegRank.device)
    LinearRegRank.lambda_ = 1E-10      # the Java's default, whatever an earlier test's command line left
    yield
    LinearRegRank.lambda_, LinearRegRank.device = saved


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def test_two_documents_by_hand_and_feature_F_is_dropped():
    # F = 2: the regressors are feature 1 and the constant.  (x1 = 0 -> 1), (x1 = 2 -> 3): y = 1 + 1 * x1
    X = np.array([[0.0, 5.0], [2.0, 7.0]], np.float32)
    lab = np.array([1.0, 3.0], np.float32)
    xtx, xty = LR.accumulate_literal(X, lab, 2)
    assert xtx.tolist() == [[4.0, 2.0], [2.0, 2.0]] and xty.tolist() == [6.0, 4.0]
    # multiplier 0.5: a[1][1] = 2 - 2 * 0.5 = 1, b[1] = 4 - 6 * 0.5 = 1; x[1] = 1, x[0] = (6 - 2 * 1) / 4 = 1
    assert LR.solve(xtx, xty) == [1.0, 1.0]
    r = LR.learn((X, lab, [0, 2], ["a"]), None, "NDCG", 10, lam=0.0)
    assert r["weight"] == [1.0, 1.0]
    # eval starts from weight[1], the constant's, and with the default list 1 .. F uses it AGAIN on feature 2: 1 + x1 + x2
    assert r["train_scores"].tolist() == [6.0, 10.0]
    # nVar = F, not F + 1: feature F never reaches the fit
    X2 = X.copy()
    X2[:, 1] = [-100.0, 3.5]
    r2 = LR.learn((X2, lab, [0, 2], ["a"]), None, "NDCG", 10, lam=0.0)
    assert _bits(r2["xtx"]) == _bits(r["xtx"]) and _bits(r2["xty"]) == _bits(r["xty"]) and r2["weight"] == r["weight"]
    assert r2["train_scores"].tolist() == [1.0 + 0.0 - 100.0, 1.0 + 2.0 + 3.5]


def test_three_documents_by_hand_and_a_feature_list():
    # F = 3: (0, 0) -> 1, (1, 0) -> 2, (0, 2) -> 5: y = 1 + x1 + 2 x2
    X = np.array([[0, 0, 9], [1, 0, 8], [0, 2, 7]], np.float32)
    lab = np.array([1, 2, 5], np.float32)
    xtx, xty = LR.accumulate_literal(X, lab, 3)
    assert xtx.tolist() == [[1.0, 0.0, 1.0], [0.0, 4.0, 2.0], [1.0, 2.0, 3.0]] and xty.tolist() == [2.0, 10.0, 8.0]
    assert LR.solve(xtx, xty) == [1.0, 2.0, 1.0]
    # -feature 2: weight[0], fitted for feature 1, multiplies feature 2
    r = LR.learn((X, lab, [0, 1, 3], ["a", "b"]), None, "NDCG", 10, lam=0.0, features=[2])
    assert r["train_scores"].tolist() == [1.0, 1.0, 1.0 + 1.0 * 2.0]
    with pytest.raises(IndexError):
        LR.eval_scores(X, [1, 2, 3, 1], [1.0, 2.0, 1.0])
    # the ridge term reaches every diagonal cell, the constant's too, and only if lambda != 0.0
    a = xtx.copy()
    for i in range(3):
        a[i, i] += 0.5
    assert LR.learn((X, lab, [0, 3], ["a"]), None, "NDCG", 10, lam=0.5)["weight"] == LR.solve(a, xty)
    assert LR.learn((X, lab, [0, 3], ["a"]), None, "NDCG", 10, lam=0.5)["weight"] != [1.0, 2.0, 1.0]


def test_constant_only():
    # F = 1: no regressor but the constant, weight[0] = sum(label) / (N + lambda); eval = w0 + w0 * x1
    X = np.array([[3.0], [5.0], [-1.0]], np.float32)
    lab = np.array([1, 2, 3], np.float32)
    r = LR.learn((X, lab, [0, 3], ["a"]), None, "NDCG", 10, lam=0.0)
    assert r["xtx"].tolist() == [[3.0]] and r["xty"].tolist() == [6.0] and r["weight"] == [2.0]
    assert r["train_scores"].tolist() == [8.0, 12.0, 0.0]
    assert LR.learn((X, lab, [0, 3], ["a"]), None, "NDCG", 10)["weight"] == [6.0 / (3.0 + 1E-10)]


def test_the_xty_product_is_a_float_product():
    x, lab = np.float32(0.1), np.float32(3.0)
    as_float, as_double = float(np.float32(x * lab)), float(x) * float(lab)
    assert as_float != as_double                            # 0.30000001192092896 against 0.3000000044703484
    xtx, xty = LR.accumulate_literal(np.array([[x, 0]], np.float32), np.array([lab]), 2)
    assert xty[0] == as_float and xtx[0, 0] == float(x) * float(x) and xtx[0, 0] != float(np.float32(x * x))
    # a product that is subnormal in f32 stays: 1e-20f * 1e-20f = 1e-40, not 0
    tiny = np.float32(1e-20)
    _, xty = LR.accumulate(np.array([[tiny, 0]], np.float32), np.array([tiny]), 2)
    assert 0.0 < xty[0] < float(np.finfo(np.float32).tiny) and xty[0] == float(np.float32(tiny * tiny))


def test_both_forms_of_the_accumulation_and_symmetry():
    rng = np.random.default_rng(5)
    for F in (1, 2, 4, 7):
        X = rng.standard_normal((60, F)).astype(np.float32)
        X[rng.random(X.shape) < 0.2] = 0.0
        X[3, :] = np.float32(1e-20)
        lab = rng.integers(0, 5, 60).astype(np.float32)
        a, b = LR.accumulate_literal(X, lab, F), LR.accumulate(X, lab, F)
        assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])
        assert _bits(a[0]) == _bits(a[0].T.copy())         # (both forms assert it themselves)
    # the sums are order dependent: the restatement's order is the documents' order
    X = (rng.standard_normal((200, 3)) * 1e3).astype(np.float32)
    lab = rng.integers(0, 5, 200).astype(np.float32)
    assert _bits(LR.accumulate(X, lab, 3)[0]) != _bits(LR.accumulate(X[::-1], lab[::-1], 3)[0])


def test_solve_by_hand_without_pivoting():
    # j = 0: rows 1, 2 with multipliers 2, 4 -> [1, 1 | 2], [3, 5 | 8]; j = 1: multiplier 3 -> [2 | 2]; x = (1, 1, 1)
    assert LR.solve([[2, 1, 1], [4, 3, 3], [8, 7, 9]], [4, 10, 24]) == [1.0, 1.0, 1.0]
    assert LR.solve([[4.0]], [2.0]) == [0.5]
    # no pivoting: a zero on the diagonal is not swapped away
    with pytest.raises(LR.NotReproduced) as e:
        LR.solve([[0.0, 1.0], [1.0, 0.0]], [1.0, 1.0])
    assert e.value.column == 0
    with pytest.raises(LR.NotReproduced) as e:              # a column of zeros with lambda = 0
        LR.learn((np.array([[1, 0, 2], [2, 0, 1], [3, 0, 0]], np.float32), np.array([0, 1, 2], np.float32), [0, 3], ["a"]), lam=0.0)
    assert e.value.column == 1
    LR.learn((np.array([[1, 0, 2], [2, 0, 1], [3, 0, 0]], np.float32), np.array([0, 1, 2], np.float32), [0, 3], ["a"]))      # the default ridge


def test_model_text_and_loading():
    lr = LinearRegRank()
    lr.features, lr.weight = [1, 2, 3], [0.5, -1.0E-5, 12345678.5]
    text = lr.model()
    # trained with the default list: features.length == weight.length, so the Java's `i == weight.length - 1` holds on the last pair and
    # only that one has no trailing space; the "0:" entry carries weight[0], not the constant's weight[2]
    assert text == "## Linear Regression\n## Lambda = 1.0E-10\n0:0.5 1:0.5 2:-1.0E-5 3:1.23456785E7"
    assert text == LR.model_text(lr.weight, lr.features, 1E-10)
    r = RankerFactory().loadRankerFromString(text)
    assert isinstance(r, LinearRegRank) and r.name() == "Linear Regression"
    # loading: keys > 0 fill features / weight in order, the key 0 value goes last: weight[last] = the saved weight[0]
    assert r.getFeatures() == [1, 2, 3] and r.weight == [0.5, -1.0E-5, 12345678.5, 0.5]
    assert (r.getFeatures(), r.weight) == LR.load(text)
    # a loaded model has one weight more than features: every pair ends in a space, the last one too
    assert r.model() == "## Linear Regression\n## Lambda = 1.0E-10\n0:0.5 1:0.5 2:-1.0E-5 3:1.23456785E7 "
    assert r.model() == LR.model_text(r.weight, r.features, 1E-10)
    # so does a model trained with a feature list shorter than nVar
    lr.features = [3, 1]
    assert lr.toString() == "0:0.5 3:0.5 1:-1.0E-5 " and lr.toString() == LR.to_string(lr.weight, lr.features)
    LinearRegRank.lambda_ = 0.5
    assert r.model().startswith("## Linear Regression\n## Lambda = 0.5\n")
    c = RankerFactory().loadRankerFromString(text + "  # trained on d.txt\n")
    assert c.weight == r.weight
    with pytest.raises(RankLibError):
        RankerFactory().loadRankerFromString("## Linear Regression\n## Lambda = 0.5\n\n")
    assert RankerFactory().createRanker(RankerType.LINEAR_REGRESSION).name() == "Linear Regression"
    assert isinstance(RankerFactory().createRanker("LINEAR_REGRESSION"), LinearRegRank)
    assert isinstance(LinearRegRank().createNew(), LinearRegRank)


def test_cli_picks_the_class_and_sets_lambda(monkeypatch):
    picked = []
    real = evaluator.Evaluator.__init__

    def spy(self, rtype, *a, **k):
        picked.append(rtype)
        real(self, rtype, *a, **k)
    monkeypatch.setattr(evaluator.Evaluator, "__init__", spy)
    with pytest.raises(RankLibError):                      # the reader refuses the missing file after the flags are parsed
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "9", "-L2", "0.5", "-device", "0"])
    assert picked == [RankerType.LINEAR_REGRESSION] and LinearRegRank.lambda_ == 0.5 and LinearRegRank.device == 0
    with pytest.raises(RankLibError):
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "6", "-l2", "0.25"])       # still accepted with another ranker
    assert picked[-1] is RankerType.LAMBDAMART and LinearRegRank.lambda_ == 0.25
    assert LambdaMART.device == 0


def test_the_neural_rankers_are_still_refused(tmp_path):
    data = tmp_path / "d.txt"
    data.write_text("1 qid:1 1:1 2:0\n0 qid:1 1:0 2:1\n")
    for n in ("1", "5", "7"):
        with pytest.raises(RankLibError) as e:
            evaluator.main(["-train", str(data), "-ranker", n])
        assert "-ranker 9 (Linear Regression)" in str(e.value) and "neural-net" in str(e.value)
    with pytest.raises(RankLibError) as e:
        RankerFactory().createRanker(RankerType.LISTNET)
    assert "LISTNET" in str(e.value) and "neural-net" in str(e.value)


def test_metric_and_sizes_are_checked_first():
    with pytest.raises(RankLibError):
        N.LinearRegTrainer(metric="BEST")
    lr = LinearRegRank()
    lr.features, lr.weight = [1, 2, 3], [0.5, 0.25]
    with pytest.raises(RankLibError) as e:                  # features.length > weight.length: the Java's ArrayIndexOutOfBoundsException
        lr.evalList(learning.RankList([learning.DataPoint("1 qid:1 1:1.0 2:1.0 3:1.0")]))
    assert "ArrayIndexOutOfBoundsException" in str(e.value)


@pytest.mark.skipif(has_gpu(), reason="the refusal without a device")
def test_no_device_fails_with_no_cpu_fallback(tmp_path):
    with pytest.raises(RankLibError) as e:
        N.LinearRegTrainer()
    assert "no CPU fallback" in str(e.value)
    data = tmp_path / "d.txt"
    data.write_text("1 qid:1 1:1 2:0\n0 qid:1 1:0 2:1\n")
    with pytest.raises(RankLibError) as e:
        evaluator.main(["-train", str(data), "-ranker", "9"])
    assert "no CPU fallback" in str(e.value) and "builds -ranker 6" not in str(e.value)
    with pytest.raises(RankLibError) as e:
        RankerFactory().loadRankerFromString("## Linear Regression\n0:0.5 1:0.5 2:1.0").eval(learning.DataPoint("1 qid:1 1:1.0 2:2.0"))
    assert "no CPU fallback" in str(e.value)
