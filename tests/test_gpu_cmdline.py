"""The evaluator flows DESIGN.md 22 adds, on the GPU: several -load (the models of a -kcv run, model f for fold f) and the flows without a
model.  The yardstick of the k-fold flows is the one-model flows that existed before them: the file is cut into 3 / 3 / 4 lists here, by
hand, model f runs on piece f list by list, and the three outputs one after the other are what the new flows must write, byte for byte,
with Evaluator.batch on and off.  No tolerance anywhere."""
import functools
import logging

import numpy as np
import pytest

import net_restatement as NR
import tree_models as T
from ranklib_amd import combiner, evaluator, normalizer
from ranklib_amd.evaluator import Evaluator
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import RankerFactory, RankerType, java_double_str, java_round
from ranklib_amd.metric import MetricScorerFactory

pytestmark = pytest.mark.gpu

LENS = [1, 20, 7, 3, 12, 5, 16, 2, 9, 4]                    # 10 lists of 1 .. 20 documents
CUTS = [(0, 3), (3, 6), (6, 10)]                            # FeatureManager.prepareCV(10 lists, 3): 10 // 3 = 3 a fold, the last takes the rest
METRICS = ("NDCG@10", "MAP", "ERR@10")


@functools.lru_cache(maxsize=None)
def list_texts():
    """6 features from a grid of four values, so that every model ties documents; list 3 has no relevant document"""
    rng = np.random.default_rng(22)
    out = []
    for q, n in enumerate(LENS):
        lines = []
        for j in range(n):
            label = 0 if q == 3 else int(rng.integers(0, 5))
            vals = rng.integers(0, 4, 6) / 2.0
            lines.append("%d qid:q%d %s #doc%d_%d\n" % (label, q, " ".join("%d:%s" % (f + 1, v) for f, v in enumerate(vals)), q, j))
        out.append("".join(lines))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def model_texts():
    """three families over three different feature sets: trees on 1 3 5, a Coordinate Ascent line on 2 4 6, a RankNet on 1 2 6"""
    trees = [T.flatten(T.S(1, 0.5, T.S(3, 1.0, T.L(0.5), T.L(-0.25)), T.S(5, 0.5, T.L(0.125), T.L(1.0)))),
             T.flatten(T.S(3, 0.0, T.L(0.25), T.L(-0.5))), T.flatten(T.S(5, 1.0, T.L(0.0), T.L(0.75)))]
    net = NR.random_net("RankNet", [1, 2, 6], [2], np.random.default_rng(5))
    return (T.model_text(trees, np.array([0.1, 1.0, 0.5], np.float32)),
            "## Coordinate Ascent\n## Restart = 5\n2:0.5 4:-0.25 6:0.125",
            net.model())


@pytest.fixture
def files(tmp_path):
    lt = list_texts()
    paths = dict(whole=str(tmp_path / "whole.txt"), pieces=[], models=[])
    with open(paths["whole"], "w") as f:
        f.write("".join(lt))
    for i, (a, b) in enumerate(CUTS):
        p = str(tmp_path / ("piece%d.txt" % i))
        with open(p, "w") as f:
            f.write("".join(lt[a:b]))
        paths["pieces"].append(p)
    for i, text in enumerate(model_texts()):
        p = str(tmp_path / ("f%d.model.txt" % (i + 1)))
        with open(p, "w", encoding="ascii") as f:
            f.write(text)
        paths["models"].append(p)
    return paths


def read(path):
    with open(path, "rb") as f:
        return f.read()


def set_norm(monkeypatch, norm):
    monkeypatch.setattr(Evaluator, "normalize", bool(norm))
    if norm:
        monkeypatch.setattr(Evaluator, "nml", normalizer.create(norm))


def one_model_flows(files, tmp_path, metric):
    """today's flows, model f on piece f, list by list: (the per-list -idv lines, the score file, the Indri file) of the three pieces
    one after the other"""
    idv, score, indri = [], b"", b""
    for f, (model, piece) in enumerate(zip(files["models"], files["pieces"])):
        e = Evaluator(RankerType.LAMBDAMART, metric, metric)
        prp, sc, run = (str(tmp_path / ("y%d.%s" % (f, x))) for x in ("idv", "score", "indri"))
        e.test(model, piece, prp)
        lines = read(prp).decode().splitlines()
        assert lines[-1].split("   ")[1] == "all" and len(lines) == CUTS[f][1] - CUTS[f][0] + 1
        idv += lines[:-1]
        e.score(model, piece, sc)
        e.rank(model, piece, run)
        score += read(sc)
        indri += read(run)
    return idv, score, indri


@pytest.mark.parametrize("norm", [None, "zscore"])
@pytest.mark.parametrize("metric", METRICS)
def test_k_fold_flows_equal_the_one_model_flows_on_the_pieces(metric, norm, files, tmp_path, monkeypatch, caplog):
    set_norm(monkeypatch, norm)
    monkeypatch.setattr(Evaluator, "batch", False)
    idv, score, indri = one_model_flows(files, tmp_path, metric)
    assert len(idv) == 10 and score.count(b"\n") == indri.count(b"\n") == sum(LENS)
    # three models give three different outputs: the last model alone, on the whole file, does not write this
    e = Evaluator(RankerType.LAMBDAMART, metric, metric)
    e.score(files["models"][2], files["whole"], str(tmp_path / "last.score"))
    assert read(str(tmp_path / "last.score")) != score
    total = 0.0
    for ln in idv:
        total += float(ln.split("   ")[2])
    assert all(java_double_str(float(ln.split("   ")[2])) == ln.split("   ")[2] for ln in idv)      # (the text holds every double exactly)
    all_line = "%s   all   %s" % (idv[0].split("   ")[0], java_double_str(total / 10))
    for batch in (True, False):
        monkeypatch.setattr(Evaluator, "batch", batch)
        for what, test_arg in (("file", files["whole"]), ("files", files["pieces"])):
            e = Evaluator(RankerType.LAMBDAMART, metric, metric)
            prp = str(tmp_path / ("new.%s.%s.idv" % (batch, what)))
            caplog.clear()
            with caplog.at_level(logging.INFO, logger="ranklib_amd"):
                got = e.test(files["models"], test_arg, prp)
            assert read(prp).decode().splitlines() == idv + [all_line], (batch, what)
            assert got == total / 10
            log = [r.getMessage() for r in caplog.records]
            assert ("Preparing 3-fold test data... " in log) == (what == "file")
            assert "%s on test data: %s" % (idv[0].split("   ")[0], java_round(got, 4)) in log
            assert "Per-ranked list performance saved to: " + prp in log
            sc, run = str(tmp_path / ("new.%s.%s.score" % (batch, what))), str(tmp_path / ("new.%s.%s.indri" % (batch, what)))
            e.score(files["models"], test_arg, sc)
            e.rank(files["models"], test_arg, run)
            assert read(sc) == score and read(run) == indri, (batch, what)


def test_main_with_three_loads_writes_the_method_s_file(files, tmp_path):
    want = str(tmp_path / "method.idv")
    Evaluator(RankerType.LAMBDAMART, "NDCG@10", "NDCG@10").test(files["models"], files["whole"], want)
    got = str(tmp_path / "main.idv")
    argv = [x for m in files["models"] for x in ("-load", m)] + ["-test", files["whole"], "-idv", got, "-metric2T", "NDCG@10"]
    assert evaluator.main(argv) == 0
    assert read(got) == read(want) and read(got).count(b"\n") == 11
    sc = str(tmp_path / "main.score")
    assert evaluator.main([x for m in files["models"] for x in ("-load", m)] + ["-rank", files["whole"], "-score", sc]) == 0
    assert read(sc).count(b"\n") == sum(LENS)
    with pytest.raises(Exception, match="3 models were given and only 2 test files"):
        evaluator.main(argv + ["-test", files["pieces"][0]])


# ---- without a model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS + ("P@3", "RR@5", "Best@2"))
def test_the_file_s_own_order(metric, files, tmp_path, monkeypatch):
    scorer = MetricScorerFactory().createScorer(metric)
    samples = FeatureManager.readInput(files["whole"])
    vals = [scorer.scoreOne(rl) for rl in samples]           # the scorer classes on the lists as read
    total = 0.0
    for v in vals:
        total += v
    want = "".join("%s   %s   %s\n" % (scorer.name(), rl.getID(), java_double_str(v)) for rl, v in zip(samples, vals))
    want += "%s   all   %s\n" % (scorer.name(), java_double_str(total / 10))
    assert len(set(vals)) > 2
    for batch in (True, False):
        monkeypatch.setattr(Evaluator, "batch", batch)
        prp = str(tmp_path / ("own.%s.idv" % batch))
        e = Evaluator(RankerType.LAMBDAMART, metric, metric)
        assert e.test(None, files["whole"], prp) == total / 10
        assert read(prp).decode() == want, batch
        assert Evaluator(RankerType.LAMBDAMART, metric, metric).test(files["whole"]) == total / 10     # test(testFile) :879-883


def bits(v):
    return np.float64(v).view(np.int64)


@pytest.mark.parametrize("metric", METRICS)
def test_score_file_of_a_model_equals_the_model_s_test(metric, files, tmp_path, monkeypatch):
    model = files["models"][0]
    sc = str(tmp_path / "model.score")
    Evaluator(RankerType.LAMBDAMART, metric, metric).score(model, files["whole"], sc)
    numbers = [ln.split("\t")[2] for ln in read(sc).decode().splitlines()]
    assert len(numbers) == sum(LENS) and len(set(numbers)) < len(numbers)        # ties
    bare = str(tmp_path / "bare.txt")
    with open(bare, "w") as f:
        f.write("\n".join(numbers) + "\n\n  \n7.5\n")       # blank lines are skipped, surplus numbers ignored
    monkeypatch.setattr(Evaluator, "batch", False)
    want = Evaluator(RankerType.LAMBDAMART, metric, metric).test(model, files["whole"])
    for batch in (True, False):
        monkeypatch.setattr(Evaluator, "batch", batch)
        got = Evaluator(RankerType.LAMBDAMART, metric, metric).testWithScoreFile(files["whole"], bare)
        assert bits(got) == bits(want), (batch, got, want)
    # a NaN among the scores: its list takes the host path, the result is the list-by-list one
    numbers[25] = "NaN"
    with open(bare, "w") as f:
        f.write("\n".join(numbers) + "\n")
    res = {}
    for batch in (True, False):
        monkeypatch.setattr(Evaluator, "batch", batch)
        res[batch] = Evaluator(RankerType.LAMBDAMART, metric, metric).testWithScoreFile(files["whole"], bare)
    assert bits(res[True]) == bits(res[False])


def test_input_order_as_an_indri_run(tmp_path):
    src = str(tmp_path / "three.txt")
    with open(src, "w") as f:
        f.write("0 qid:7 1:0.5 # docA\n2 qid:7 1:0.25 #docB #x\n1 qid:7 1:1.0\n1 qid:8 1:0.0 #docD\n")
    out = str(tmp_path / "three.indri")
    Evaluator(RankerType.LAMBDAMART, "NDCG@10", "NDCG@10").rank(src, out)
    assert read(out).decode() == ("7 Q0 docA 1 1.0 indri\n7 Q0 docB x 2 0.9999 indri\n7 Q0  3 0.9998 indri\n8 Q0 docD 1 1.0 indri\n")
    assert evaluator.main(["-rank", src, "-indri", out + "2"]) == 0 and read(out + "2") == read(out)


def test_combined_forest_loads_with_one_bag_per_file(tmp_path):
    header = ("## Random Forests\n## No. of bags = 1\n## Sub-sampling = 1.0\n## Feature-sampling = 0.3\n## No. of trees = 1\n## No. of leaves = 10\n"
              "## No. of threshold candidates = 256\n## Learning rate = 0.1\n\n")
    d = tmp_path / "bags"
    d.mkdir()
    blocks = []
    for name, tree in (("a.txt", T.S(2, 0.25, T.L(-1.0), T.L(2.0))), ("b.txt", T.S(1, 1.0, T.L(0.0), T.L(0.375)))):
        text = T.model_text([T.flatten(tree)], [1.0])
        blocks.append(text[text.index("<ensemble>"):])
        (d / name).write_text(header + blocks[-1])
    (d / "x.progress").write_text("not a model\n")
    out = str(tmp_path / "forest.txt")
    combiner.main([str(d), out])
    r = RankerFactory().loadRankerFromFile(out)
    assert r.name() == "Random Forests" and r.getEnsembles() == blocks and sorted(r.getFeatures()) == [1, 2]
