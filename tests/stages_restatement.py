"""rl_model_predict_stages / rl_model_eval_stages restated with what the tests already have -- TEST INFRASTRUCTURE ONLY.

A model of T trees has stages t = 1 .. T; stage t is the ensemble of the first t trees with their weights.  A document's stage score is
tree_models.eval_ensemble_np(trees[:t], weights[:t], rows) -- the prefix of Ensemble.eval's float chain -- and a list's stage value is
what eval_lists_restatement.eval_lists returns for those scores widened to f64, the ideal DCGs resolved once over the whole file.  A
(stage, list) cell whose scores hold a NaN returns the flag and 0.0 instead of a value.  tests/test_stages_cpu.py holds this against
hand-derived tables; the GPU tests compare the kernels with it."""
import numpy as np

import eval_lists_restatement as ER
import tree_models as TM


def stage_scores(trees, weights, rows, stages):
    """f32 [len(stages)][n_docs]"""
    return np.stack([TM.eval_ensemble_np(trees[:t], weights[:t], rows) for t in stages])


def eval_stages(trees, weights, rows, labels, qoff, metric, k, stages, err_max=16.0, qkey=None, ideal_dcg=None, rel_doc_count=None,
                scores=None, pos=None):
    """(f64 values [S][Q], uint8 NaN flags [S][Q], f64 ideal [Q]) with the arguments of _native.Model.eval_stages behind the model.
    scores / pos: stage_scores(...) and stage_positions(...) of an earlier call on the same model and file (a test that scores one
    file under many metrics walks and ranks it once)."""
    qoff = [int(v) for v in qoff]
    nl = len(qoff) - 1
    sc = stage_scores(trees, weights, rows, stages) if scores is None else scores
    if pos is None:
        pos = stage_positions(sc, qoff)
    vals, nan = np.zeros((len(stages), nl), np.float64), np.zeros((len(stages), nl), np.uint8)
    ideal = None
    for s in range(len(stages)):
        row = sc[s].astype(np.float64)
        for q in range(nl):
            nan[s, q] = np.isnan(row[qoff[q]:qoff[q + 1]]).any()
        v, _, ideal = ER.eval_lists(np.where(np.isnan(row), 0.0, row), labels, qoff, metric, k, err_max=err_max, qkey=qkey,
                                    ideal_dcg=ideal_dcg, rel_doc_count=rel_doc_count, pos=pos[s])
        vals[s] = np.where(nan[s] != 0, 0.0, v)
    return vals, nan, ideal


def stage_positions(sc, qoff):
    """int32 [S][n_docs]: every document's position in its list's stable descending ranking at every stage (a NaN reads as 0.0: its
    list is flagged and not compared)"""
    qoff = [int(v) for v in qoff]
    pos = np.zeros(sc.shape, np.int32)
    for s in range(sc.shape[0]):
        row = np.where(np.isnan(sc[s]), 0.0, sc[s].astype(np.float64))
        for q in range(len(qoff) - 1):
            pos[s, qoff[q]:qoff[q + 1]] = ER.positions(row[qoff[q]:qoff[q + 1]])
    return pos


def same_bits(got, want):
    """None, or what differs between two f64 arrays compared as bit patterns"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if got.shape != want.shape:
        return "shape %r != %r" % (got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    if bad.size == 0:
        return None
    i = tuple(bad[0])
    return "%d of %d values differ, first at %r: %r != %r" % (len(bad), want.size, i, got[i], want[i])
