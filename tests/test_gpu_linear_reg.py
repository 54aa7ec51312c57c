"""Linear Regression (-ranker 9) on the MI355X: xTx and xTy as accumulated (rl_lr_debug_gram), the weights, both metric values, evalList and
the model text bit-identical to the literal restatement of LinearRegRank.learn / solve / eval (tests/lr_restatement.py); ragged cell tiles
and document slabs for every register block; unknown cells and short rows through the Python class; the refusals; and the command-line
flow on the LETOR fixtures.  Every comparison is float64.tobytes() equality.

-qrel judgments are covered by test_external_judgments_match_the_restatement (per set), test_cli_qrel_reaches_the_trainer and
test_external_judgment_refusals; labels of 31 and above (gains that wrap as Java ints) by test_wrapped_labels; fractional labels, which
xTy takes as they are, by test_fractional_labels."""
import os

import numpy as np
import pytest

import linear_ext as E
import lr_restatement as LR
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, LinearRegRank, RankList, RankerFactory, flatten, java_double_str, java_round
from ranklib_amd.metric import ERRScorer, MetricScorerFactory

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "letor")


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = (LinearRegRank.lambda_, LinearRegRank.device, ERRScorer.MAX, DataPoint.missingZero, evaluator.Evaluator.normalize)
    LinearRegRank.lambda_ = 1E-10      # the Java's default, whatever an earlier test's command line left
    yield
    LinearRegRank.lambda_, LinearRegRank.device, ERRScorer.MAX, DataPoint.missingZero, evaluator.Evaluator.normalize = saved


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def _data(rng, lengths, F, zero_col=None, tiny=True):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(qoff[-1])
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[rng.random(X.shape) < 0.15] = 0.0
    lab = rng.integers(0, 5, n).astype(np.float32)
    if tiny and n >= 8:                                       # cells and labels around 1e-20: the f32 product x * label is subnormal
        rows = rng.choice(n, max(1, n // 50), replace=False)
        X[rows, :] = (np.float32(1e-20) * rng.uniform(0.5, 2.0, (len(rows), F))).astype(np.float32)
        lab[rows[::2]] = np.float32(1.5e-20)
    if zero_col is not None:
        X[:, zero_col] = 0.0
    return X, lab, qoff, ["q%d" % i for i in range(len(lengths))]


def _trainer(train, valid=None, metric="NDCG", k=10, err_max=16.0, lam=1E-10, features=None, ext=None):
    """ext: the per-list external judgments of linear_ext.feed (ideal_tr / ideal_va / rdc_tr / rdc_va)"""
    t = E.feed(N.LinearRegTrainer(lambda_=lam, metric=metric, metric_k=k, err_max=err_max), train, valid, **(ext or {}))
    X = train[0]
    if features is not None:
        t.set_features(0, [f - 1 if 1 <= f <= X.shape[1] else -1 for f in features])
    return t


def _assert_same_run(t, r, valid):
    xtx, xty = t.gram()
    assert _bits(xtx) == _bits(r["xtx"]) and _bits(xty) == _bits(r["xty"])
    assert _bits(t.weights()) == _bits(r["weight"])
    ts, vs = t.scores()
    assert _bits(ts) == _bits(r["train"])
    if valid:
        assert _bits(vs) == _bits(r["valid"])


def _run(train, valid, metric, k, gmax, lam, features=None):
    r = LR.learn(train, valid, metric, k, lam=lam, features=features, err_max=gmax)
    t = _trainer(train, valid, metric, k, gmax, lam, features)
    t.learn()
    _assert_same_run(t, r, valid is not None)
    return t, r


_METRICS = [("NDCG", 10, 16.0), ("DCG", 3, 16.0), ("MAP", 0, 16.0), ("ERR", 10, 8.0), ("P", 5, 16.0), ("RR", 10, 16.0)]
_LAMBDAS = [1E-10, 0.0, 0.5]


@pytest.mark.parametrize("valid", [True, False], ids=["valid", "novalid"])
@pytest.mark.parametrize("mi", range(6), ids=[m[0] for m in _METRICS])
def test_all_metrics_with_and_without_validation(mi, valid):
    metric, k, gmax = _METRICS[mi]
    rng = np.random.default_rng(100 + mi)
    tr = _data(rng, rng.integers(1, 25, 40), 5)
    va = _data(rng, rng.integers(1, 25, 30), 5) if valid else None
    t, r = _run(tr, va, metric, k, gmax, _LAMBDAS[(mi + valid) % 3])
    assert max(abs(w) for w in r["weight"]) < 1e3


# (F, list lengths, metric index, validation, lambda, register block or None for the library's choice)
_SHAPES = [
    (1, [1], 0, False, 1E-10, None),                                           # one document, the constant only
    (1, [3, 1, 7], 2, True, 0.0, 4),
    (2, [1, 2, 16, 17], 1, True, 0.0, None),
    (5, [1, 2, 16, 17, 9, 384, 385, 5003, 12], 2, True, 1E-10, 2),            # every class of the ranking kernel
    (33, "50k", 3, False, 0.5, None),                                          # ~50 000 documents: hundreds of slabs, a ragged tail
    (33, "50k", 0, False, 1E-10, 4),
    (137, "3k", 4, True, 1E-10, None),                                         # 137 = 17 * 8 + 1: ragged tiles for every register block
    (137, "3k", 4, False, 0.0, 2),
    (137, "3k", 5, False, 0.5, 4),
    (150, "3k", 5, True, 0.0, 1),
    (150, "3k", 1, False, 1E-10, 4),
]


@pytest.mark.parametrize("case", _SHAPES, ids=["F%d-%s-%s-rb%s" % (c[0], c[1] if isinstance(c[1], str) else "n%d" % sum(c[1]), _METRICS[c[2]][0], c[5])
                                               for c in _SHAPES])
def test_shapes_and_register_blocks(case, monkeypatch):
    F, lengths, mi, valid, lam, rb = case
    metric, k, gmax = _METRICS[mi]
    rng = np.random.default_rng(7 * F + mi)
    if lengths == "50k":
        lengths = np.concatenate([rng.integers(1, 400, 240), [5000, 1, 3777]])
    elif lengths == "3k":
        lengths = rng.integers(1, 60, 100)
    if rb is not None:
        monkeypatch.setenv("RLHIP_LR_RB", str(rb))
    tr = _data(rng, lengths, F, tiny=sum(lengths) > F + 8)
    va = _data(rng, rng.integers(1, 30, 20), F) if valid else None
    if sum(lengths) < F:                                      # fewer documents than unknowns: only the ridge term makes it solvable
        assert lam != 0.0
    t, r = _run(tr, va, metric, k, gmax, lam)
    if rb is not None:
        assert t.times()["register_block"] == rb
    assert np.all(np.isfinite(r["weight"]))


def test_subnormal_float_product_reaches_xty():
    X = np.array([[1e-20, 2.0, 0.0], [3e-20, -1.0, 0.0], [0.5, 0.25, 0.0], [1.0, 4.0, 0.0]], np.float32)
    lab = np.array([1.5e-20, 2e-20, 1.0, 2.0], np.float32)
    want = float(np.float32(X[0, 0] * lab[0])) + float(np.float32(X[1, 0] * lab[1]))
    assert 0.0 < float(np.float32(X[0, 0] * lab[0])) < float(np.finfo(np.float32).tiny)
    tr = (X[:2], lab[:2], np.array([0, 2], np.int32), ["a"])
    t = _trainer(tr, lam=0.5)
    t.learn()
    assert _bits(t.gram()[1][0]) == _bits(want) and want > 0.0
    _run((X, lab, np.array([0, 1, 4], np.int32), ["a", "b"]), None, "NDCG", 10, 16.0, 1E-10)


def test_a_column_of_zeros_and_a_feature_subset():
    rng = np.random.default_rng(3)
    tr = _data(rng, rng.integers(1, 30, 40), 6, zero_col=2)
    _run(tr, None, "NDCG", 10, 16.0, 1E-10)                   # the ridge term is the column's whole pivot
    _run(tr, None, "MAP", 0, 16.0, 0.5, features=[5, 2, 6])   # weight[i] (fitted for feature i + 1) multiplies features[i]
    _run(tr, None, "MAP", 0, 16.0, 0.5, features=[4, 9])      # an id no row has reads 0 (as under -missingZero)
    with pytest.raises(LR.NotReproduced) as want:
        LR.learn(tr, None, "NDCG", 10, lam=0.0)
    assert want.value.column == 2
    t = _trainer(tr, lam=0.0)
    with pytest.raises(N.RankLibError) as e:
        t.learn()
    assert "Linear Regression" in str(e.value) and "the column of feature 3" in str(e.value)
    assert _bits(t.gram()[0]) == _bits(LR.accumulate(tr[0], tr[1], 6)[0])      # the sums are there, the solve is what is refused


def test_refusals():
    rng = np.random.default_rng(2)
    X, lab, qoff, qid = _data(rng, [4, 5, 6], 3, tiny=False)
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[4, 1] = bad
        with pytest.raises(N.RankLibError):
            N.LinearRegTrainer().set_train(Xb, lab, qoff)
    with pytest.raises(N.RankLibError):
        N.LinearRegTrainer(metric="BEST")
    t = _trainer((X, lab, qoff, qid), features=[1, 2, 3, 1])  # features.length > weight.length
    with pytest.raises(N.RankLibError) as e:
        t.learn()
    assert "ArrayIndexOutOfBoundsException" in str(e.value)
    with pytest.raises(N.RankLibError) as e:
        N.lr_predict([1, 2, 3], [0.5, 0.25], np.zeros((2, 4), np.float32))
    assert "ArrayIndexOutOfBoundsException" in str(e.value)
    dup = X.copy()
    dup[:, 1] = dup[:, 0]                                     # a dependent column and no ridge term
    dup = (np.round(dup * 4) / 4).astype(np.float32)
    dup[:, 1] = dup[:, 0]
    try:
        LR.learn((dup, lab, qoff, qid), None, "NDCG", 10, lam=0.0)
        refused = False
    except LR.NotReproduced:
        refused = True
    t = _trainer((dup, lab, qoff, qid), lam=0.0)
    if refused:
        with pytest.raises(N.RankLibError):
            t.learn()
    else:
        t.learn()
    t = _trainer((X, lab, qoff, qid))
    t.learn()
    with pytest.raises(N.RankLibError):                       # once per handle
        t.learn()


def _lists(X, lab, qoff, unknown=None, short=None):
    """RankLists of DataPoints from text lines; unknown[i]: feature ids left out of row i (NaN, read as 0); short[i]: row i stops early"""
    out = []
    for q in range(len(qoff) - 1):
        dps = []
        for i in range(qoff[q], qoff[q + 1]):
            last = X.shape[1] if not short or i not in short else short[i]
            feats = " ".join("%d:%s" % (j + 1, repr(float(X[i, j]))) for j in range(last) if not unknown or (j + 1) not in unknown.get(i, ()))
            dps.append(DataPoint("%s qid:%d %s # d%d" % (repr(float(lab[i])), q, feats, i)))
        out.append(RankList(dps))
    return out


def test_python_class_unknown_cells_and_missing_zero():
    rng = np.random.default_rng(17)
    X, lab, qoff, qid = _data(rng, rng.integers(2, 12, 25), 6, tiny=False)
    unknown = {i: {int(f) for f in rng.choice(np.arange(1, 6), 2, replace=False)} for i in range(0, X.shape[0], 5)}
    Xz = X.copy()
    for i, fs in unknown.items():
        Xz[i, [f - 1 for f in fs]] = 0.0
    lists = _lists(X, lab, qoff, unknown)
    scorer = MetricScorerFactory().createScorer("NDCG@10")
    lr = LinearRegRank(lists, list(range(1, 7)), scorer)
    lr.init()
    lr.learn()
    r = LR.learn((Xz, lab, qoff, [str(q) for q in range(len(qoff) - 1)]), None, "NDCG", 10)
    assert _bits(lr.gram[0]) == _bits(r["xtx"]) and _bits(lr.gram[1]) == _bits(r["xty"])
    assert _bits(lr.weight) == _bits(r["weight"]) and lr.getScoreOnTrainingData() == java_round(r["train"], 4)
    got = np.concatenate([lr.evalList(rl) for rl in lists])
    assert _bits(got) == _bits(r["train_scores"])
    assert _bits(lr.eval(lists[0].get(0))) == _bits(r["train_scores"][0])
    assert lr.model() == LR.model_text(r["weight"], list(range(1, 7)), 1E-10)
    # a row that ends before feature 6: the Java's message without -missingZero, 0 with it
    short = {3: 4}
    lists = _lists(X, lab, qoff, unknown, short)
    lr = LinearRegRank(lists, list(range(1, 7)), scorer)
    with pytest.raises(N.RankLibError) as e:
        lr.init()
    assert "requesting unspecified feature" in str(e.value)
    DataPoint.missingZero = True
    Xz[3, 4:] = 0.0
    lr = LinearRegRank(lists, list(range(1, 7)), MetricScorerFactory().createScorer("NDCG@10"))
    lr.init()
    lr.learn()
    r = LR.learn((Xz, lab, qoff, [str(q) for q in range(len(qoff) - 1)]), None, "NDCG", 10)
    assert _bits(lr.weight) == _bits(r["weight"])
    assert _bits(np.concatenate([lr.evalList(rl) for rl in lists])) == _bits(r["train_scores"])


def test_python_class_with_a_feature_list(tmp_path):
    """-feature 5 2 6 through the command line: the fit still reads features 1 .. F - 1, eval pairs weight[i] with features[i], and the
    model text (a list shorter than nVar: every pair ends in a space) and the -score file are the restatement's, byte for byte; -kcv 3 -tvs 0.8 and -norm run"""
    rng = np.random.default_rng(31)
    X, lab, qoff, _ = _data(rng, rng.integers(2, 20, 30), 6, tiny=False)
    data, feats, model, scores = (str(tmp_path / n) for n in ("d.txt", "f.txt", "m.txt", "s.txt"))
    with open(data, "w") as f:
        for q in range(len(qoff) - 1):
            for i in range(qoff[q], qoff[q + 1]):
                f.write("%d qid:%d %s # d%d\n" % (int(lab[i]), q, " ".join("%d:%s" % (j + 1, repr(float(X[i, j]))) for j in range(6)), i))
    with open(feats, "w") as f:
        f.write("5\n2\n6\n")
    evaluator.main(["-train", data, "-ranker", "9", "-feature", feats, "-metric2t", "NDCG@5", "-L2", "0.0", "-save", model])
    r = LR.learn((X, lab, qoff, [str(q) for q in range(len(qoff) - 1)]), None, "NDCG", 5, lam=0.0, features=[5, 2, 6])
    text = open(model).read()
    assert text == LR.model_text(r["weight"], [5, 2, 6], 0.0) and text.endswith(" ")
    evaluator.main(["-load", model, "-rank", data, "-score", scores])
    lf, lw = LR.load(text)
    assert lf == [5, 2, 6] and len(lw) == 4
    rows = [line.rstrip("\n").split("\t") for line in open(scores)]
    assert [x[2] for x in rows] == [java_double_str(float(v)) for v in LR.eval_scores(X, lf, lw)]
    # the splits and -norm come through RankerTrainer
    evaluator.main(["-train", data, "-ranker", "9", "-kcv", "3", "-tvs", "0.8", "-metric2t", "MAP"])
    evaluator.main(["-train", data, "-ranker", "9", "-tvs", "0.8", "-norm", "zscore", "-metric2t", "NDCG@10", "-L2", "0.5"])


def _read(path, F=None):
    lists = FeatureManager.readInput(path)
    F = F or max(rl.getFeatureCount() for rl in lists)
    X, lab, qoff, _ = flatten(lists, list(range(1, F + 1)))
    return lists, (X, lab, qoff, [rl.getID() for rl in lists])


@pytest.mark.parametrize("lam", [1E-10, 0.0])
@pytest.mark.parametrize("name,F", [("small_mslr_k3", 5), ("lmart_map", 6), ("valid_estop", 4)])
def test_fixtures_train_with_finite_weights(name, F, lam):
    _, tr = _read(os.path.join(GOLDEN, name + ".train.txt"))
    assert tr[0].shape[1] == F
    t, r = _run(tr, None, "NDCG", 10, 16.0, lam)
    assert np.all(np.isfinite(r["weight"])) and 0.1 < max(abs(w) for w in r["weight"]) < 2.0


def test_command_line_flow(tmp_path):
    train = os.path.join(GOLDEN, "small_mslr_k3.train.txt")
    model, scores1, scores2 = (str(tmp_path / n) for n in ("m.txt", "s1.txt", "s2.txt"))
    evaluator.main(["-train", train, "-ranker", "9", "-metric2t", "NDCG@10", "-test", train, "-save", model])
    lists, tr = _read(train)
    r = LR.learn(tr, None, "NDCG", 10)
    feats = list(range(1, 6))
    assert open(model).read() == LR.model_text(r["weight"], feats, 1E-10)
    # the trained object scores with weight[F - 1] as the bias, the loaded one with weight[0]: every score moves by ONE constant
    e = evaluator.Evaluator(learning.RankerType.LINEAR_REGRESSION, "NDCG@10", "NDCG@10")
    trained = e.evaluate(train)
    assert _bits(trained.weight) == _bits(r["weight"])
    assert _bits(np.concatenate([trained.evalList(rl) for rl in lists])) == _bits(r["train_scores"])
    loaded = RankerFactory().loadRankerFromFile(model)
    lf, lw = LR.load(open(model).read())
    assert loaded.getFeatures() == lf == feats and _bits(loaded.weight) == _bits(lw) and lw[-1] == r["weight"][0] and len(lw) == 6
    want_loaded = LR.eval_scores(tr[0], lf, lw)
    assert _bits(np.concatenate([loaded.evalList(rl) for rl in lists])) == _bits(want_loaded)
    assert r["weight"][0] != r["weight"][4] and not np.array_equal(want_loaded, r["train_scores"])
    for a, b in zip(tr[2][:-1], tr[2][1:]):                   # ... and every list keeps its ranking
        assert np.array_equal(learning.stable_desc_order(want_loaded[a:b]), learning.stable_desc_order(r["train_scores"][a:b]))
    # -load -test and -load -rank -score; both models give the identical test metric here (the restatement says so first)
    sc = MetricScorerFactory().createScorer("NDCG@10")
    m_trained = sc.score(trained.rank(lists))
    m_loaded = e.test(model, train)
    from ca_restatement import LiteralScorer
    lit = LiteralScorer("NDCG", 10)
    w1 = lit.score([float(v) for v in r["train_scores"]], tr[1], tr[2], tr[3])
    w2 = lit.score([float(v) for v in want_loaded], tr[1], tr[2], tr[3])
    assert _bits(w1) == _bits(w2)
    assert _bits(m_trained) == _bits(w1) and _bits(m_loaded) == _bits(w2)
    evaluator.main(["-load", model, "-rank", train, "-score", scores1])
    rows = [line.rstrip("\n").split("\t") for line in open(scores1)]
    assert [x[2] for x in rows] == [java_double_str(float(v)) for v in want_loaded]
    # with a validation set and -L2
    vt, vv = os.path.join(GOLDEN, "valid_estop.train.txt"), os.path.join(GOLDEN, "valid_estop.valid.txt")
    evaluator.main(["-train", vt, "-validate", vv, "-ranker", "9", "-L2", "0.5", "-metric2t", "ERR@10", "-save", model])
    _, a = _read(vt)
    _, b = _read(vv, 4)
    r = LR.learn(a, b, "ERR", 10, lam=0.5)
    assert open(model).read() == LR.model_text(r["weight"], [1, 2, 3, 4], 0.5)
    e = evaluator.Evaluator(learning.RankerType.LINEAR_REGRESSION, "ERR@10", "ERR@10")
    ranker = e.evaluate(vt, vv)
    assert ranker.getScoreOnTrainingData() == java_round(r["train"], 4) and _bits(ranker.getScoreOnValidationData()) == _bits(r["valid"])
    evaluator.main(["-load", model, "-rank", vv, "-score", scores2])
    assert len(open(scores2).readlines()) == b[0].shape[0]


# ---- -qrel judgments, labels of 31 and above, fractional labels ---------------------------------------------------------------------
def _sets(seed, labels=(0, 1, 2)):
    """linear_ext.shared_sets (repeated qids, a validation set that shares some) with normal feature values: a well-conditioned fit"""
    rng = np.random.default_rng(seed)
    tr, va = E.shared_sets(rng, labels=labels)
    return ((rng.standard_normal(tr[0].shape).astype(np.float32),) + tr[1:], (rng.standard_normal(va[0].shape).astype(np.float32),) + va[1:], rng)


@pytest.mark.parametrize("where", ["train", "valid", "both"])
@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("MAP", 0)])
def test_external_judgments_match_the_restatement(metric, k, where):
    """external ideal DCGs (NaN for the qids without one; below, at and above the lists' own) and relevant-document counts (0, own, larger)
    given to the training set, the validation set or both: the weights stay, the two metric values are the restatement's"""
    tr, va, rng = _sets(91)
    m = E.ideal_map([tr, va], 10, rng) if metric == "NDCG" else E.count_map([tr, va], rng)
    assert any(q in m for q in set(tr[3]) & set(va[3])) and any(q not in m for q in set(tr[3])) and any(q not in m for q in set(va[3]))
    arrays, ext = E.judgments(metric, m, tr, va, where)
    r, plain = LR.learn(tr, va, metric, k, **ext), LR.learn(tr, va, metric, k)
    assert (r["valid"] != plain["valid"]) == (where != "train" or metric == "NDCG")      # counts stay with their set; an ideal DCG is cached for both
    assert (r["train"] != plain["train"]) == (where != "valid" or metric == "NDCG")
    t = _trainer(tr, va, metric, k, ext=arrays)
    t.learn()
    _assert_same_run(t, r, True)


@pytest.mark.parametrize("metric,k", [("NDCG", 10), ("DCG", 5), ("ERR", 10)])
def test_wrapped_labels(metric, k):
    """labels of 31, 32 and 33: gains 2147483647, 0 and 1 (metric/DCGScorer.java:28-31,137-139; ERRScorer.java:71-73); the regression
    fits the labels themselves"""
    tr, va, _ = _sets(93, E.WRAPPED)
    assert {31.0, 32.0, 33.0} <= set(tr[1].tolist())
    _, r = _run(tr, va, metric, k, 16.0, 1E-10)
    assert abs(r["train"]) > (1e6 if metric != "NDCG" else 0.0)


@pytest.mark.parametrize("metric,k", [("MAP", 0), ("P", 3), ("RR", 10), ("NDCG", 10)])
def test_fractional_labels(metric, k):
    """labels of 0.5, 1.5 and 2.99 enter xTy as they are (LinearRegRank.java:70-72), count as relevant for MAP / P / RR and as (int) label
    for NDCG"""
    tr, va, _ = _sets(94, E.FRACTIONAL)
    assert {0.5, 1.5} <= set(tr[1].tolist())
    t, r = _run(tr, va, metric, k, 16.0, 1E-10)
    assert not np.array_equal(r["xty"], LR.accumulate(tr[0], np.floor(tr[1]), tr[0].shape[1])[1])
    assert _bits(t.gram()[1]) == _bits(r["xty"])


def test_external_judgment_refusals():
    """rl_lr_set_external_judgments forwards to rl_ca_set_external_judgments; a later set_train discards the judgments"""
    rng = np.random.default_rng(95)
    tr = _data(rng, [4, 5, 6, 3], 3, tiny=False)
    t, t2 = E.forwarded_refusals(lambda: N.LinearRegTrainer(metric="MAP", metric_k=0), tr, N.RankLibError)
    judged, plain = LR.learn(tr, None, "MAP", 0, rel_doc_count=E.REFUSAL_MAP), LR.learn(tr, None, "MAP", 0)
    assert judged["train"] != plain["train"]
    _assert_same_run(t, judged, False)
    _assert_same_run(t2, plain, False)


@pytest.mark.parametrize("m2t", ["NDCG@10", "MAP"])
def test_cli_qrel_reaches_the_trainer(tmp_path, m2t):
    """-qrel <file> with -ranker 9.  The weights are a least-squares fit and know no metric, so the saved model is the restatement's with
    and without the judgments; what the judgments change is the score of the training data the ranker reports, and that is the
    restatement's fed the maps the host scorer loaded from the same file."""
    rng = np.random.default_rng(96)
    X, lab, qoff, _ = _data(rng, rng.integers(2, 25, 30), 4, tiny=False)
    data, qrel, m_q, m_raw = (str(tmp_path / n) for n in ("d.txt", "qrel.txt", "q.txt", "raw.txt"))
    E.write_letor(data, X, lab, qoff)
    E.write_qrel(qrel, rng, np.diff(qoff))
    sc = MetricScorerFactory().createScorer(m2t)
    sc.loadExternalRelevanceJudgment(qrel)
    ext = dict(ideal=dict(sc.idealGains)) if m2t != "MAP" else dict(rel_doc_count=dict(sc.relDocCount))
    metric, k = ("MAP", 0) if m2t == "MAP" else ("NDCG", 10)
    train = (X, lab, qoff, [str(q) for q in range(len(qoff) - 1)])
    r, plain = LR.learn(train, None, metric, k, **ext), LR.learn(train, None, metric, k)
    assert java_round(r["train"], 4) != java_round(plain["train"], 4)
    args = ["-train", data, "-ranker", "9", "-metric2t", m2t]
    try:
        evaluator.main(args + ["-qrel", qrel, "-save", m_q])
        assert evaluator.Evaluator.qrelFile == qrel           # the Evaluator built now loads the file, as main() just did
        judged = evaluator.Evaluator(learning.RankerType.LINEAR_REGRESSION, m2t, m2t).evaluate(data)
    finally:
        evaluator.Evaluator.qrelFile = ""                     # whatever fails above, no later test inherits the file
    evaluator.main(args + ["-save", m_raw])
    assert evaluator.Evaluator.qrelFile == ""
    raw = evaluator.Evaluator(learning.RankerType.LINEAR_REGRESSION, m2t, m2t).evaluate(data)
    assert open(m_q).read() == open(m_raw).read() == LR.model_text(r["weight"], [1, 2, 3, 4], 1E-10)
    assert judged.getScoreOnTrainingData() == java_round(r["train"], 4) and raw.getScoreOnTrainingData() == java_round(plain["train"], 4)
