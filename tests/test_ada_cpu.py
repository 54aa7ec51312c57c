"""AdaRank (-ranker 3) without a GPU: utilities/Sorter's unstable order, the restatement of AdaRank.learn, the model text, RankerFactory,
the CLI's statics, and the refusal without a device."""
import numpy as np
import pytest

import ada_restatement as AR
from conftest import has_gpu
from ranklib_amd import _native as N
from ranklib_amd import evaluator, learning
from ranklib_amd._native import RankLibError
from ranklib_amd.learning import AdaRank, CoorAscent, RankerFactory

_STATICS = ("nIteration", "tolerance", "trainWithEnqueue", "maxSelCount", "device")


@pytest.fixture(autouse=True)
def _restore_statics():
    saved = {k: getattr(AdaRank, k) for k in _STATICS}
    ca_tol = CoorAscent.tolerance
    yield
    for k, v in saved.items():
        setattr(AdaRank, k, v)
    CoorAscent.tolerance = ca_tol


def test_sorter_is_the_unstable_selection_sort():
    assert AR.sorter_sort([1.0, 1.0, 2.0]) == [2, 1, 0]                    # labels [0, 1, 0] rank as 2, 1 (label 1), 1 (label 0)
    assert list(learning.stable_desc_order([1.0, 1.0, 2.0])) == [2, 0, 1]
    # three tie groups, worked by hand: the 1s come out as 4 before 1, a stable sort gives 1 before 4
    v = [3.0, 1.0, 3.0, 2.0, 1.0, 2.0, 3.0]
    assert AR.sorter_sort(v) == [0, 2, 6, 3, 5, 4, 1]
    assert list(learning.stable_desc_order(v)) == [0, 2, 6, 3, 5, 1, 4]
    assert AR.sorter_sort([]) == [] and AR.sorter_sort([5.0]) == [0]
    assert AR.sorter_sort([-0.0, 0.0]) == [0, 1]                           # equal under the Java's <


def test_sorter_numpy_form_matches_the_transcription():
    rng = np.random.default_rng(3)
    for n in (2, 3, 7, 16, 40, 101):
        for levels in (1, 2, 3, 50):
            v = list(rng.integers(0, levels, n).astype(np.float64))
            full = AR.sorter_sort(v)
            assert AR.sorter_sort_np(v) == full
            for steps in (1, 3, 10):
                assert AR.sorter_sort_np(v, steps)[:min(steps, n)] == full[:min(steps, n)]


def test_weak_ranker_order_changes_map():
    sc = AR.CR.LiteralScorer("MAP", 0)
    lab = [0.0, 1.0, 0.0]
    M = AR.weak_table(np.array([[1.0], [1.0], [2.0]], np.float32), lab, [0, 3], ["q"], sc, "MAP", 0)
    assert M[0, 0] == 0.5                                                  # Sorter: labels 0, 1, 0
    assert sc.m.score([lab[i] for i in learning.stable_desc_order([1.0, 1.0, 2.0])], "q") == 1.0 / 3


def _data(rng, lengths, F, levels=3, labels=3):
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    X = (rng.integers(0, levels, (qoff[-1], F)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    lab = rng.integers(0, labels, qoff[-1]).astype(np.float32)
    return X, lab, qoff, ["q%d" % i for i in range(len(lengths))]


def test_restatement_runs_both_phases():
    rng = np.random.default_rng(5)
    tr = _data(rng, rng.integers(2, 12, 21), 4)
    r = AR.learn(tr, metric="NDCG", k=5, nIteration=40)
    kinds = [t[1] for t in r["trace"]]
    assert kinds[0] == AR.PHASE and AR.ROUND in kinds
    assert len(r["fid"]) == len(r["weight"]) and all(0 <= f < 4 for f in r["fid"])
    r2 = AR.learn(tr, metric="MAP", k=0, nIteration=40, trainWithEnqueue=False, maxSelCount=2)
    assert [t[1] for t in r2["trace"]].count(AR.PHASE) == 1


def test_perfect_feature_is_refused_by_the_restatement():
    lab = np.array([1, 0, 1, 0], np.float32)
    X = np.array([[1.0, 0.3], [0.0, 0.9], [1.0, 0.1], [0.0, 0.5]], np.float32)
    with pytest.raises(AR.NonFiniteAlpha):
        AR.learn((X, lab, np.array([0, 2, 4], np.int32), ["a", "b"]), metric="MAP", k=0)


def test_model_text_and_round_trip():
    ada = AdaRank()
    ada.rankers, ada.rweight = [1, 3, 1], [0.5, -0.25, 1e-5]
    text = ada.model()
    assert text == ("## AdaRank\n## Iteration = 500\n## Train with enqueue: Yes\n## Tolerance = 0.002\n"
                    "## Max consecutive selection count = 5\n1:0.5 3:-0.25 1:1.0E-5")
    r = RankerFactory().loadRankerFromString(text)
    assert isinstance(r, AdaRank) and r.name() == "AdaRank"
    assert r.rankers == [1, 3, 1] and r.rweight == [0.5, -0.25, 1e-5] and r.getFeatures() == [1, 3, 1]
    assert r.model() == text
    AdaRank.trainWithEnqueue, AdaRank.nIteration = False, 7
    assert "## Iteration = 7\n## Train with enqueue: No\n" in r.model()
    with pytest.raises(RankLibError):
        RankerFactory().loadRankerFromString("## AdaRank\n## Iteration = 500\n\n")
    with pytest.raises(RankLibError):
        AdaRank().loadFromString("## AdaRank\n1:0.5 x")
    assert RankerFactory().createRanker(learning.RankerType.ADARANK).name() == "AdaRank"
    assert isinstance(RankerFactory().createRanker("ADARANK"), AdaRank)


def test_cli_sets_the_statics():
    with pytest.raises(RankLibError):                      # the reader refuses the missing file after the flags are parsed
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "3", "-round", "7", "-noeq", "-max", "2", "-tolerance", "0.01"])
    assert (AdaRank.nIteration, AdaRank.trainWithEnqueue, AdaRank.maxSelCount, AdaRank.tolerance) == (7, False, 2, 0.01)
    assert CoorAscent.tolerance == 0.01


def test_metric_is_checked_first():
    with pytest.raises(RankLibError):
        N.AdaRankTrainer(metric="BEST")


@pytest.mark.skipif(has_gpu(), reason="the refusal without a device")
def test_no_device_fails_with_no_cpu_fallback(tmp_path):
    with pytest.raises(RankLibError) as e:
        N.AdaRankTrainer()
    assert "no CPU fallback" in str(e.value)
    data = tmp_path / "d.txt"
    data.write_text("1 qid:1 1:1 2:0\n0 qid:1 1:0 2:1\n")
    with pytest.raises(RankLibError) as e:
        evaluator.main(["-train", str(data), "-ranker", "3"])
    assert "no CPU fallback" in str(e.value) and "builds -ranker 6" not in str(e.value)
