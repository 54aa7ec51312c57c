"""The host bookkeeping every scoring and training call goes through, where no device and no library is needed: the list
chunker, the cut of a chunk's results, the row builder with its two check rules, what a scorer holds resolved per list id, the trainer
feed, and the argument cursor of the command lines.  Every expected boundary, key and message is written out here by hand."""
import numpy as np
import pytest

import list_cases as LC
from ranklib_amd import contribs, evaluator, features, importance, partial, stages
from ranklib_amd import metric as M
from ranklib_amd._native import RankLibError
from ranklib_amd.evaluator import ArgCursor, Evaluator, common_flag
from ranklib_amd.learning import (AdaRank, CoorAscent, DataPoint, LambdaMART, LinearRegRank, RankBoost, Ranker, RankList, RankNet,
                                  dense_rows, feed_trainer, list_chunks, result_steps)

UNSPECIFIED = "Error in DenseDataPoint::getFeatureValue(): requesting unspecified feature, fid=%d"


def point(n_features, qid="q", label=0.0, values=None):
    fv = np.full(n_features + 1, 0.5, np.float32) if values is None else np.asarray([np.nan] + list(values), np.float32)
    fv[0] = np.nan
    return DataPoint.from_parsed(label, qid, "", fv)


def lists_of(*shapes):
    """one list per (documents, features)"""
    return [RankList([point(f, "q%d" % i) for _ in range(n)]) for i, (n, f) in enumerate(shapes)]


# ---- list_chunks -------------------------------------------------------------------------------------------------------------------------
ROW = 6 * 4                                                 # a document of five features: six f32 columns

CHUNK_CASES = {
    "no lists": ([], 10 * ROW, []),
    "one list": ([(3, 5)], 10 * ROW, [(0, 1)]),
    "an empty list first": ([(0, 0), (4, 5), (7, 5)], 10 * ROW, [(0, 2), (2, 3)]),
    "an empty list in the middle": ([(6, 5), (0, 0), (4, 5), (1, 5)], 10 * ROW, [(0, 3), (3, 4)]),
    "an empty list last": ([(6, 5), (5, 5), (0, 0)], 10 * ROW, [(0, 1), (1, 3)]),
    "only empty lists": ([(0, 0), (0, 0)], 10 * ROW, [(0, 2)]),
    "a list larger than the limit stands alone": ([(2, 5), (30, 5), (2, 5), (3, 5)], 10 * ROW, [(0, 1), (1, 2), (2, 4)]),
    "a larger list first": ([(30, 5), (2, 5)], 10 * ROW, [(0, 1), (1, 2)]),
    "a sum equal to the limit stays": ([(4, 5), (6, 5), (1, 5)], 10 * ROW, [(0, 2), (2, 3)]),
    "the same sum plus one row is cut": ([(4, 5), (7, 5), (1, 5)], 10 * ROW, [(0, 1), (1, 3)]),
    "one byte under the equal sum is cut": ([(4, 5), (6, 5), (1, 5)], 10 * ROW - 1, [(0, 1), (1, 3)]),
    # 4 + 4 narrow rows are 8 * 3 * 4 = 96 bytes; the wide list makes them 8 * 11 * 4 = 352, over 300 through the width alone
    "a wide list pushes a narrow chunk over": ([(4, 2), (4, 10), (1, 2)], 300, [(0, 1), (1, 3)]),
    # the width of a chunk only grows: after the wide list a narrow one counts as wide (5 + 2 rows of 11 columns = 308 > 300)
    "the width stays": ([(5, 10), (2, 2), (2, 2)], 300, [(0, 1), (1, 3)]),
    "the wide list joins where it fits": ([(2, 2), (4, 10)], 300, [(0, 2)]),
    "no limit": ([(2, 5), (30, 5), (0, 0), (500, 40)], None, [(0, 4)]),
    "no limit, no lists": ([], None, []),
    # every list stands alone, the empty one too: behind a document its 0 rows still leave 1 * 6 * 4 > 0
    "a limit of nothing": ([(1, 5), (1, 5), (0, 0), (1, 5)], 0, [(0, 1), (1, 2), (2, 3), (3, 4)]),
}


@pytest.mark.parametrize("name", sorted(CHUNK_CASES))
def test_list_chunks(name):
    shapes, limit, want = CHUNK_CASES[name]
    samples = lists_of(*shapes)
    got = list(list_chunks(samples, limit))
    assert got == want
    covered = [q for a, b in got for q in range(a, b)]
    assert covered == list(range(len(samples))) and all(b > a for a, b in got)      # the pairs tile the file, no gap, no empty chunk


def test_list_chunks_of_the_shared_small_file():
    assert list(list_chunks(LC.lists(), LC.SMALL_LIMIT)) == LC.CHUNKS
    assert [sum(LC.SIZES[a:b]) for a, b in LC.CHUNKS] == LC.CHUNK_ROWS
    assert list(list_chunks(LC.lists(), Ranker.EVAL_ROW_BYTES)) == [(0, len(LC.SIZES))]


# ---- result_steps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit, want", [
    (5 * 5 * 8 - 1, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]),      # one matrix is over the limit: a piece holds one row all the same
    (5 * 5 * 8, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]),          # equal: one row
    (2 * 5 * 5 * 8 - 1, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]),
    (3 * 5 * 5 * 8, [(0, 3), (3, 6), (6, 7)]),                                      # below: three rows, the last piece short
    (100 * 5 * 5 * 8, [(0, 7)]),
])
def test_result_steps(limit, want, monkeypatch):
    monkeypatch.setattr(Ranker, "EVAL_ROW_BYTES", limit)
    assert list(result_steps(7, 8 * 5 * 5)) == want
    assert list(result_steps(0, 8 * 5 * 5)) == []


# ---- dense_rows --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def missing_zero():
    saved = DataPoint.missingZero
    yield lambda v: setattr(DataPoint, "missingZero", v)
    DataPoint.missingZero = saved


def test_dense_rows_width_nan_and_short_rows(missing_zero):
    missing_zero(False)
    dps = [point(3, values=[1.5, np.nan, -2.0]), point(1, values=[4.0]), point(5, values=[np.nan, 0.25, np.inf, -0.0, 7.0])]
    want = np.array([[0, 1.5, 0, -2.0, 0, 0], [0, 4.0, 0, 0, 0, 0], [0, 0, 0.25, np.inf, -0.0, 7.0]], np.float32)
    for rows in (dense_rows(dps, 1), dense_rows(dps, checked=[1]), dense_rows(dps, 0)):
        assert rows.dtype == np.float32 and rows.shape == (3, 6) and np.array_equal(rows.view(np.uint32), want.view(np.uint32))
    missing_zero(True)                                      # the width follows the largest id asked for where no document is that long
    assert dense_rows(dps, 8).shape == (3, 9) and dense_rows(dps, checked=[2, 8, 3]).shape == (3, 9)
    assert dense_rows([], 4).shape == (0, 5) and dense_rows([], checked=[]).shape == (0, 1)


def test_dense_rows_tree_rule(missing_zero):
    missing_zero(False)
    dps = [point(3), point(1), point(5)]
    assert dense_rows(dps, 0).shape == (3, 6)               # a model without features: id 0 is never refused
    assert dense_rows([point(0)], 0).shape == (1, 1)
    assert dense_rows(dps, 1).shape == (3, 6)
    with pytest.raises(RankLibError) as e:                  # the model's largest id, whichever document is too short
        dense_rows(dps, 3)
    assert str(e.value) == UNSPECIFIED % 3
    with pytest.raises(RankLibError) as e:
        dense_rows(dps, 7)
    assert str(e.value) == UNSPECIFIED % 7


def test_dense_rows_linear_rule(missing_zero):
    missing_zero(False)
    dps = [point(3), point(2), point(5)]
    assert dense_rows(dps, checked=[2, 1, 2]).shape == (3, 6)
    for fids, bad in (([1, 3, 2], 3),                       # document 1 has two features
                      ([2, 5, 4, 1], 5),                    # document 0 fails on 5 before document 1 fails on 4
                      ([4, 3], 4), ([1, 0, 9], 0), ([2, -1], -1), ([0], 0)):
        with pytest.raises(RankLibError) as e:
            dense_rows(dps, checked=fids)
        assert str(e.value) == UNSPECIFIED % bad, fids


def test_dense_rows_with_missing_zero_checks_nothing(missing_zero):
    missing_zero(True)
    dps = [point(3), point(1)]
    assert not dense_rows(dps, 9)[:, 4:].any() and dense_rows(dps, 9).shape == (2, 10)
    assert dense_rows(dps, checked=[9, 0, 2]).shape == (2, 10)


# ---- what a scorer holds -----------------------------------------------------------------------------------------------------------------
def test_metric_name():
    assert [M.metric_name(s) for s in (M.NDCGScorer(3), M.DCGScorer(), M.APScorer(), M.ERRScorer(5), M.PrecisionScorer(1),
                                       M.ReciprocalRankScorer(), M.BestAtKScorer(2))] == ["NDCG", "DCG", "MAP", "ERR", "P", "RR", "BEST"]


def test_id_keys_count_up_in_first_seen_order():
    k = M.id_keys(["b", "a", "b", "c", "a", "b"])
    assert k.dtype == np.int32 and k.tolist() == [0, 1, 0, 2, 1, 0]
    assert M.id_keys([]).shape == (0,) and M.id_keys(iter(["x"])).tolist() == [0]


def test_held_judgments_ndcg():
    s = M.NDCGScorer(10)
    s.idealGains.update({"a": 2.5, "c": 0.0})
    qkey, ideal, rdc = M.held_judgments(s, "NDCG", ["b", "a", "b", "c", "d"])
    assert qkey.dtype == np.int32 and qkey.tolist() == [0, 1, 0, 2, 3] and rdc is None
    assert ideal.dtype == np.float64 and np.array_equal(np.isnan(ideal), [True, False, True, False, True]) and ideal[1] == 2.5 and ideal[3] == 0.0
    qkey, ideal, rdc = M.held_judgments(M.NDCGScorer(10), "NDCG", ["a", "a"])       # nothing held: the array is sent all the same
    assert qkey.tolist() == [0, 0] and np.isnan(ideal).all() and ideal.shape == (2,) and rdc is None


def test_held_judgments_map():
    s = M.APScorer()
    assert s.relDocCount is None and M.held_judgments(s, "MAP", ["a", "b"]) == (None, None, None)
    s.relDocCount = {}                                      # a -qrel file without a relevant line: every id counts 0
    qkey, ideal, rdc = M.held_judgments(s, "MAP", ["a", "b"])
    assert qkey is None and ideal is None and rdc.dtype == np.int32 and rdc.tolist() == [0, 0]
    s.relDocCount = {"b": 3}
    assert M.held_judgments(s, "MAP", ["a", "b", "b"])[2].tolist() == [0, 3, 3]


@pytest.mark.parametrize("scorer", [M.DCGScorer(10), M.ERRScorer(10), M.PrecisionScorer(10), M.ReciprocalRankScorer()])
def test_held_judgments_of_the_other_metrics(scorer):
    name = M.metric_name(scorer)
    assert name in ("DCG", "ERR", "P", "RR") and M.held_judgments(scorer, name, ["a", "b"]) == (None, None, None)
    M.keep_ideals(scorer, name, ["a", "b"], [1.0, 2.0])
    assert not hasattr(scorer, "idealGains")


def test_keep_ideals():
    s = M.NDCGScorer(10)
    s.idealGains["a"] = 2.5
    M.keep_ideals(s, "NDCG", ["b", "a", "b", "c"], np.array([7.0, 9.0, 8.0, 0.0]))
    assert s.idealGains == {"a": 2.5, "b": 7.0, "c": 0.0}    # the entry stays, and so does the first list of a new id
    assert all(type(v) is float for v in s.idealGains.values())
    ap = M.APScorer()
    ap.relDocCount = {"a": 1}
    M.keep_ideals(ap, "MAP", ["a", "b"], [np.nan, np.nan])
    assert ap.relDocCount == {"a": 1} and not hasattr(ap, "idealGains")


# ---- the trainer feed --------------------------------------------------------------------------------------------------------------------
class Recorder:
    """stands in for a _native trainer: keeps what it is given"""

    def __init__(self):
        self.calls = []

    def set_train(self, X, labels, qoff, **kw):
        self.calls.append(("train", X.shape, qoff.tolist(), kw))

    def set_validation(self, X, labels, qoff, qkey=None):
        self.calls.append(("validation", X.shape, qoff.tolist(), qkey))

    def set_external_judgments(self, validation, ideal, rdc):
        self.calls.append(("judgments", validation, ideal, rdc))


def ranker_of(train_ids, valid_ids, scorer):
    r = Ranker([RankList([point(2, i), point(2, i)]) for i in train_ids], [1, 2], scorer)
    if valid_ids is not None:
        r.setValidationSet([RankList([point(2, i)]) for i in valid_ids])
    return r


def test_feed_trainer_keys():
    r, t = ranker_of(["a", "b", "a", "c"], ["b", "d", "a", "d", "e"], M.NDCGScorer(10)), Recorder()
    feed_trainer(r, t, "NDCG", feature_ids=[1, 2])
    assert [c[0] for c in t.calls] == ["train", "validation"]         # idealGains is empty: no judgments are sent
    kind, shape, qoff, kw = t.calls[0]
    assert shape == (8, 2) and qoff == [0, 2, 4, 6, 8] and sorted(kw) == ["feature_ids", "qkey"] and kw["feature_ids"] == [1, 2]
    assert kw["qkey"].dtype == np.int32 and kw["qkey"].tolist() == [0, 1, 0, 2]
    # an id of the training set keeps its key; the others continue after the three training keys, by their place in the validation set
    assert t.calls[1][1:3] == ((5, 2), [0, 1, 2, 3, 4, 5]) and t.calls[1][3].dtype == np.int32 and t.calls[1][3].tolist() == [1, 4, 0, 4, 7]


def test_feed_trainer_without_validation_and_without_further_arguments():
    r, t = ranker_of(["a", "a"], None, M.DCGScorer(10)), Recorder()
    feed_trainer(r, t, "DCG")
    assert len(t.calls) == 1 and sorted(t.calls[0][3]) == ["qkey"] and t.calls[0][3]["qkey"].tolist() == [0, 0]


def test_feed_trainer_judgments():
    s = M.NDCGScorer(10)
    s.idealGains["a"] = 2.5
    r, t = ranker_of(["a", "b", "a"], ["c", "a"], s), Recorder()
    feed_trainer(r, t, "NDCG")
    assert [c[:2] for c in t.calls] == [("train", (6, 2)), ("validation", (2, 2)), ("judgments", False), ("judgments", True)]
    for call, want in zip(t.calls[2:], ([2.5, np.nan, 2.5], [np.nan, 2.5])):
        assert call[2].dtype == np.float64 and np.array_equal(call[2], want, equal_nan=True) and call[3] is None
    ap = M.APScorer()
    r, t = ranker_of(["a", "b"], ["b"], ap), Recorder()
    feed_trainer(r, t, "MAP")
    assert [c[0] for c in t.calls] == ["train", "validation"]         # relDocCount None: the lists count their own
    ap.relDocCount = {"b": 4}
    t = Recorder()
    feed_trainer(r, t, "MAP")
    assert [(c[1], c[2], c[3].tolist()) for c in t.calls[2:]] == [(False, None, [0, 4]), (True, None, [4])]
    r, t = ranker_of(["a"], None, s), Recorder()             # the scorer holds NDCG entries, the run trains on DCG: nothing is sent
    feed_trainer(r, t, "DCG")
    assert [c[0] for c in t.calls] == ["train"]


def test_feed_trainer_with_the_rankers_own_columns():
    r, t = ranker_of(["a", "b"], ["b"], M.DCGScorer(10)), Recorder()
    seen = []

    def flat(lists):
        seen.append(lists)
        return np.zeros((len(lists), 7), np.float32), np.zeros(len(lists), np.float32), np.arange(len(lists) + 1, dtype=np.int32), np.arange(len(lists), dtype=np.int32)
    feed_trainer(r, t, "DCG", flat)
    assert seen[0] is r.samples and seen[1] is r.validationSamples and [c[1] for c in t.calls] == [(2, 7), (1, 7)]


# ---- the command lines' cursor -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def statics():
    """what common_flag writes"""
    classes = (LambdaMART, CoorAscent, AdaRank, RankBoost, LinearRegRank, RankNet)
    saved = (DataPoint.missingZero, Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.nml, Evaluator.qrelFile, M.ERRScorer.MAX, [c.device for c in classes])
    yield
    DataPoint.missingZero, Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.nml, Evaluator.qrelFile, M.ERRScorer.MAX = saved[:6]
    for c, d in zip(classes, saved[6]):
        c.device = d


def test_cursor_walks_flags_and_values():
    cur = ArgCursor(["-Load", "Model.TXT", "-WITHIN", "-seed", "7"])
    got = []
    for a in cur:
        got.append((a, cur.nxt() if a in ("-load", "-seed") else None))
    assert got == [("-load", "Model.TXT"), ("-within", None), ("-seed", "7")]      # flags in lower case, values as they are


def test_cursor_refusals():
    cur = ArgCursor(["-within", "-Seed"])
    flags = iter(cur)
    assert next(flags) == "-within" and next(flags) == "-seed"
    with pytest.raises(RankLibError) as e:
        cur.nxt()
    assert str(e.value) == "Missing value for -Seed"
    cur = ArgCursor(["-x", "-Bogus"])
    flags = iter(cur)
    next(flags), next(flags)
    with pytest.raises(RankLibError) as e:
        cur.unknown()
    assert str(e.value) == "Unknown command-line parameter: -Bogus"


def test_common_flag(statics):
    def run(args, **kw):
        cur = ArgCursor(args)
        return [common_flag(a, cur.nxt, **kw) for a in cur]
    DataPoint.missingZero, Evaluator.mustHaveRelDoc, Evaluator.normalize, Evaluator.qrelFile = False, False, False, ""
    assert run(["-MissingZero", "-HR", "-QREL", "j.txt", "-gMax", "3", "-NORM", "zscore", "-Device", "2", "-load"]) == [True] * 6 + [False]
    assert DataPoint.missingZero and Evaluator.mustHaveRelDoc and Evaluator.qrelFile == "j.txt" and M.ERRScorer.MAX == 8.0
    assert Evaluator.normalize and type(Evaluator.nml).__name__ == "ZScoreNormalizor"
    assert [c.device for c in (LambdaMART, CoorAscent, AdaRank, RankBoost, LinearRegRank, RankNet)] == [2] * 6
    DataPoint.missingZero = Evaluator.normalize = False
    assert run(["-missingzero", "-norm", "sum", "-device", "5"], reader_only=True) == [True] * 3
    assert DataPoint.missingZero and Evaluator.normalize
    assert [c.device for c in (LambdaMART, CoorAscent, AdaRank, RankBoost, LinearRegRank, RankNet)] == [5, 2, 2, 2, 2, 2]
    assert run(["-gmax", "-qrel", "-hr"], reader_only=True) == [False] * 3 and M.ERRScorer.MAX == 8.0
    with pytest.raises(RankLibError, match="Missing value for -device"):
        run(["-device"])


@pytest.mark.parametrize("tool, flag", [(stages, "-within"), (stages, "-feature"), (importance, "-step"), (importance, "-grid"), (partial, "-repeat"),
                                        (partial, "-metric2t"), (contribs, "-gmax"), (contribs, "-qrel"), (contribs, "-hr"), (contribs, "-metric2t"),
                                        (evaluator, "-step"), (evaluator, "-background")])
def test_a_flag_the_tool_does_not_take(tool, flag, statics):
    with pytest.raises(RankLibError) as e:
        tool.main(["-load", "m.txt", flag.upper(), "1"])
    assert str(e.value) == "Unknown command-line parameter: " + flag.upper()


@pytest.mark.parametrize("tool, flags", [
    (stages, ["-test", "-metric2T", "-step", "-curve", "-save", "-pick", "-gmax", "-qrel", "-norm", "-device"]),
    (importance, ["-test", "-metric2T", "-repeat", "-seed", "-feature", "-out", "-gmax", "-qrel", "-norm", "-device"]),
    (partial, ["-test", "-grid", "-feature", "-out", "-ice", "-gmax", "-qrel", "-norm", "-device"]),
    (contribs, ["-background", "-test", "-feature", "-out", "-summary", "-interactions", "-norm", "-device"]),
    (evaluator, ["-train", "-ranker", "-qrel", "-norm", "-device", "-tree"]),
    (features, ["-input", "-k", "-tvs", "-tts", "-output", "-seed"]),
])
def test_every_value_flag_of_a_tool_asks_for_its_value(tool, flags, statics):
    for flag in flags:
        with pytest.raises(RankLibError) as e:
            tool.main(["-load", "m.txt", "-load", "n.txt", flag] if tool is not features else ["-shuffle", "-shuffle", flag])
        assert str(e.value) == "Missing value for " + flag, flag
