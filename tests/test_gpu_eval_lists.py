"""rl_eval_lists on the GPU against the flat restatement (tests/eval_lists_restatement.py, which test_eval_lists_cpu.py holds equal to the
scorer classes): every length class edge of k_eval_lists, the score and label patterns, every metric and k, the external tables, chunking;
and the evaluator's test-time flows end to end, batch against list by list, byte for byte.  No tolerance anywhere."""
import functools
import logging
import os

import numpy as np
import pytest

import eval_lists_restatement as ER
import tree_models as T
from ranklib_amd import _native as N
from ranklib_amd import metric as M
from ranklib_amd.evaluator import Evaluator
from ranklib_amd.learning import DataPoint, Ranker, RankerFactory, RankerType

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETOR = os.path.join(ROOT, "tests", "golden", "letor")
TINY, WAVE, BLOCK = 16, 256, 6144     # kEvTiny, kEvWave, kEvBlock of rl_eval.inc: 6145 documents are past the LDS class, on global scratch
GROUPS = {"short": [1, 2, 3], "tiny": [TINY - 1, TINY, TINY + 1], "wave": [WAVE - 1, WAVE, WAVE + 1], "block": [BLOCK - 1, BLOCK, BLOCK + 1]}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def group_file(group):
    """one file per group and its ranking by the restatement, made once"""
    sc, lab, qoff, what = ER.make_file(GROUPS[group], seed=len(group))
    _, pos, _ = ER.eval_lists(sc, lab, qoff, "DCG", 1, want_pos=True)
    for a in (sc, lab, qoff, pos):
        a.setflags(write=False)
    return sc, lab, qoff, what, pos


def same(got, want, what, tag):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert not bad.size, (tag, [what[q] for q in bad[:3]], got[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("metric", ER.METRICS)
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_length_class_pattern_metric_and_k(group, metric):
    sc, lab, qoff, what, pos = group_file(group)
    for k in ER.ks_of(GROUPS[group]):
        got, gpos, gideal = N.eval_lists(sc, lab, qoff, metric, k, want_pos=True)
        want, _, ideal = ER.eval_lists(sc, lab, qoff, metric, k, pos=pos)
        assert np.array_equal(gpos, pos), (metric, k)
        same(got, want, what, (metric, k))
        assert np.array_equal(bits(gideal), bits(ideal))
    for q, (n, sp, _) in enumerate(what):
        if sp == "equal":
            assert np.array_equal(gpos[qoff[q]:qoff[q + 1]], np.arange(n))
    if metric == "RR":                                      # plain RR: k = 0 scores 0, as written
        assert not N.eval_lists(sc, lab, qoff, "RR", M.ReciprocalRankScorer().k)[0].any()
    if metric == "BEST":
        zero = [q for q, w in enumerate(what) if w[2] == "zero"]
        assert zero and not N.eval_lists(sc, lab, qoff, "BEST", 3)[0][zero].any()


def test_many_tiny_lists_fill_the_last_block_partly():
    rng = np.random.default_rng(21)
    lens = rng.integers(1, TINY + 1, 16 * 3 + 5)           # 16 lists per block: the last block holds 5
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    sc = rng.integers(-3, 4, qoff[-1]) * 0.5
    lab = rng.integers(0, 5, qoff[-1]).astype(np.float32)
    for metric, k in (("NDCG", 10), ("MAP", 0), ("ERR", 3), ("P", 5), ("RR", 2), ("BEST", 3), ("DCG", 0)):
        got, gpos, _ = N.eval_lists(sc, lab, qoff, metric, k, want_pos=True)
        want, pos, _ = ER.eval_lists(sc, lab, qoff, metric, k, want_pos=True)
        assert np.array_equal(gpos, pos) and np.array_equal(bits(got), bits(want)), metric


def test_external_tables_and_the_first_list_of_a_key():
    rng = np.random.default_rng(22)
    lens = [9, 30, 4, 300, 12, 30]
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    sc = rng.standard_normal(qoff[-1]).round(1)
    lab = rng.integers(0, 5, qoff[-1]).astype(np.float32)
    lab[qoff[5]:qoff[6]] = 0
    lab[qoff[5]], sc[qoff[5]] = 4, 9.0                      # lists 1 and 5 share a key and differ in their labels; list 5's DCG is not 0
    qkey = np.array([0, 1, 2, 3, 0, 1], np.int32)
    ideal = np.array([np.nan, np.nan, 3.25, np.nan, np.nan, np.nan])
    for k in (0, 3, 10, 31):
        got, _, used = N.eval_lists(sc, lab, qoff, "NDCG", k, qkey=qkey, ideal_dcg=ideal)
        want, _, wused = ER.eval_lists(sc, lab, qoff, "NDCG", k, qkey=qkey, ideal_dcg=ideal)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(used), bits(wused))
        assert used[5] == used[1] and used[4] == used[0] and used[2] == 3.25      # the second list took the first's ideal, and out_ideal says so
        own, _, uown = N.eval_lists(sc, lab, qoff, "NDCG", k)
        assert uown[5] != used[5] and own[5] != got[5]
    rdc = np.array([3, 0, 1, 40, 0, 2], np.int32)
    got, _, _ = N.eval_lists(sc, lab, qoff, "MAP", 0, rel_doc_count=rdc)
    want, _, _ = ER.eval_lists(sc, lab, qoff, "MAP", 0, rel_doc_count=rdc)
    assert np.array_equal(bits(got), bits(want)) and got[1] == 0.0 and got[4] == 0.0
    got, _, _ = N.eval_lists(sc, lab, qoff, "ERR", 10, err_max=4.0)
    want, _, _ = ER.eval_lists(sc, lab, qoff, "ERR", 10, err_max=4.0)
    assert np.array_equal(bits(got), bits(want))


def test_a_file_cut_at_a_list_boundary_equals_one_call():
    sc, lab, qoff, what, pos = group_file("wave")
    cut = len(what) // 2 + 1
    d = int(qoff[cut])
    for metric, k in (("NDCG", 10), ("MAP", 0), ("BEST", 3)):
        whole, wpos, _ = N.eval_lists(sc, lab, qoff, metric, k, want_pos=True)
        a, apos, _ = N.eval_lists(sc[:d], lab[:d], qoff[:cut + 1], metric, k, want_pos=True)
        b, bpos, _ = N.eval_lists(sc[d:], lab[d:], qoff[cut:] - d, metric, k, want_pos=True)
        assert np.array_equal(bits(np.concatenate([a, b])), bits(whole)) and np.array_equal(np.concatenate([apos, bpos]), wpos)


def test_a_nan_score_is_refused_with_the_list_named():
    with pytest.raises(N.RankLibError, match="NaN score in list 1"):
        N.eval_lists([1.0, 2.0, np.nan], [0, 1, 0], [0, 2, 3], "NDCG", 10)


# ---- the evaluator's flows, batch against list by list ------------------------------------------------------------------------------------
def tree_text(trees, weights=None):
    return T.model_text(trees, np.ones(len(trees), np.float32) if weights is None else np.array(weights, np.float32))


def _trees_a():
    return [T.flatten(T.S(1, 5.0, T.S(3, 4.0, T.L(0.5), T.L(-0.25)), T.S(2, 0.5, T.L(0.125), T.L(1.0)))),
            T.flatten(T.S(5, 10.0, T.L(0.25), T.L(-0.5))), T.flatten(T.S(4, 0.0, T.L(0.0), T.L(0.75)))]


def _trees_b():
    return [T.flatten(T.S(2, 0.25, T.L(-1.0), T.S(3, 10.0, T.L(0.5), T.L(2.0)))), T.flatten(T.S(1, 1.0, T.L(0.0), T.L(0.375)))]


def _ensemble_block(text):
    return text[text.index("<ensemble>"):]


MODELS = {
    "trees": lambda: tree_text(_trees_a(), [0.1, 1.0, 0.5]),
    "random_forests": lambda: ("## Random Forests\n## No. of bags = 2\n## Sub-sampling = 1.0\n## Feature-sampling = 0.3\n## No. of trees = 3\n"
                               "## No. of leaves = 10\n## No. of threshold candidates = 256\n## Learning rate = 0.1\n\n"
                               + _ensemble_block(tree_text(_trees_a(), [1.0, 0.5, 0.25])) + _ensemble_block(tree_text(_trees_b()))),
    "coordinate_ascent": lambda: "## Coordinate Ascent\n## Restart = 5\n1:0.5 2:-0.25 3:0.125 5:0.0625",
    "rankboost": lambda: "## RankBoost\n## Iteration = 4\n2:0.25:0.75 1:5.0:-1.5 3:10.0:0.125 5:3.0:1.0E-5",
    "net": lambda: ("## RankNet\n## Epochs = 100\n## No. of features = 3\n## No. of hidden layers = 1\n## Layer 1: 2 neurons\n1 2 3\n1\n2\n"
                    "0 0 0.05 -0.01\n0 1 -1.0 0.5\n0 2 0.01 0.02\n0 3 0.1 0.2 -0.001\n1 0 1.5\n1 1 -0.75\n"),
}
FIXTURE = {"trees": "lmart_err", "random_forests": "small_ns", "coordinate_ascent": "mart_ndcg", "rankboost": "small_mslr_k3", "net": "lmart_map"}
TEST_METRICS = ("NDCG@10", "MAP", "ERR@10", "P@5", "RR@3", "Best@3")


def run_flows(model, data, tmp, tag, caplog, metrics=TEST_METRICS):
    """what test (every metric, with -idv), score and rank leave behind: {name: file bytes, log lines or the error's text}"""
    out = {}

    def flow(name, fn, path):
        caplog.clear()
        try:
            fn()
            out[name] = open(path, "rb").read()
        except Exception as ex:       # noqa: BLE001 -- an error is part of what the two paths must share
            out[name] = "%s: %s" % (type(ex).__name__, ex)
        out[name + ".log"] = [r.getMessage() for r in caplog.records if r.name == "ranklib_amd"]
    with caplog.at_level(logging.INFO, logger="ranklib_amd"):
        for m in metrics:
            e = Evaluator(RankerType.LAMBDAMART, m, m)
            prp = os.path.join(tmp, "%s.%s.idv" % (tag, m.replace("@", "_")))
            flow("test " + m, lambda: e.test(model, data, prp), prp)
        e = Evaluator(RankerType.LAMBDAMART, "NDCG@10", "NDCG@10")
        flow("score", lambda: e.score(model, data, os.path.join(tmp, tag + ".score")), os.path.join(tmp, tag + ".score"))
        flow("rank", lambda: e.rank(model, data, os.path.join(tmp, tag + ".indri")), os.path.join(tmp, tag + ".indri"))
    for name, v in out.items():       # the log names the -idv file, which differs between the two runs by its tag only
        if name.endswith(".log"):
            out[name] = [ln.replace(tag, "TAG") for ln in v]
    return out


def both_paths(model_text, data, tmp_path, caplog, monkeypatch, metrics=TEST_METRICS):
    model = str(tmp_path / "model.txt")
    with open(model, "w", encoding="ascii") as f:
        f.write(model_text)
    calls = []
    real = N.eval_lists
    monkeypatch.setattr(N, "eval_lists", lambda *a, **kw: (calls.append(len(a[0])), real(*a, **kw))[1])
    monkeypatch.setattr(Evaluator, "batch", True)
    got = run_flows(model, data, str(tmp_path), "run_batch", caplog, metrics)
    n_batch = len(calls)
    monkeypatch.setattr(Evaluator, "batch", False)
    want = run_flows(model, data, str(tmp_path), "run_lists", caplog, metrics)
    assert len(calls) == n_batch, "the list by list path must not reach rl_eval_lists"
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    return got, calls


@pytest.mark.parametrize("family", sorted(MODELS))
def test_flows_are_byte_identical_batch_and_list_by_list(family, tmp_path, caplog, monkeypatch):
    data = os.path.join(LETOR, FIXTURE[family] + ".train.txt")
    got, calls = both_paths(MODELS[family](), data, tmp_path, caplog, monkeypatch)
    assert len(calls) == len(TEST_METRICS) + 1              # one call per test flow, one for rank; score needs none
    for m in TEST_METRICS:
        idv = got["test " + m].decode().splitlines()
        assert idv[-1].split("   ")[1] == "all" and len(idv) >= 8
        assert any(ln.startswith(idv[0].split("   ")[0] + " on test data: ") for ln in got["test %s.log" % m])
    assert got["score"].count(b"\n") == got["rank"].count(b"\n") > 100 and b" Q0 " in got["rank"]


def test_chunked_scoring_equals_one_chunk(tmp_path, caplog, monkeypatch):
    data = os.path.join(LETOR, "lmart_err.train.txt")
    one, _ = both_paths(MODELS["trees"](), data, tmp_path, caplog, monkeypatch, metrics=("NDCG@10",))
    monkeypatch.setattr(Ranker, "EVAL_ROW_BYTES", 40 * 6 * 4)       # about 40 documents of this file's 6-column rows a call
    rows = []
    r = RankerFactory().loadRankerFromString(MODELS["trees"]())
    monkeypatch.setattr(type(r), "_evalDocs", lambda self, dps, f=type(r)._evalDocs: (rows.append(len(dps)), f(self, dps))[1])
    many, _ = both_paths(MODELS["trees"](), data, tmp_path, caplog, monkeypatch, metrics=("NDCG@10",))
    assert many == one and len(rows) > 10 and max(rows) <= 60


def test_a_list_with_a_nan_score_takes_the_host_path_alone(tmp_path, caplog, monkeypatch):
    data = os.path.join(LETOR, "lmart_err.train.txt")
    f3 = sorted(float(ln.split()[4].split(":")[1]) for ln in open(data))
    assert f3[0] < f3[1]                                    # one document has the file's smallest feature 3: it alone reaches the NaN leaf
    trees = [T.flatten(T.S(3, np.float32(f3[0]), T.L(np.nan), T.L(1.0)))] + _trees_b()
    got, calls = both_paths(tree_text(trees), data, tmp_path, caplog, monkeypatch)
    n_docs = got["score"].count(b"\n")
    assert got["score"].count(b"\tNaN\n") == 1
    assert calls and all(0 < n_docs - c <= 40 for c in calls), (n_docs, calls)       # every call went without that one list


def test_the_missing_feature_error_is_the_per_list_path_s(tmp_path, caplog, monkeypatch):
    data = os.path.join(LETOR, "lmart_err.train.txt")       # 5 features; the models ask for feature 9
    assert not DataPoint.missingZero
    want = "RankLibError: Error in DenseDataPoint::getFeatureValue(): requesting unspecified feature, fid=9"
    for text in (tree_text([T.flatten(T.S(9, 0.5, T.L(0.0), T.L(1.0)))]), "## Coordinate Ascent\n1:0.5 9:0.25",
                 "## RankNet\n1 9\n0\n0 0 1.0\n0 1 0.5\n0 2 0.25\n"):
        got, _ = both_paths(text, data, tmp_path, caplog, monkeypatch, metrics=("NDCG@10",))
        assert got["test NDCG@10"] == got["score"] == got["rank"] == want
