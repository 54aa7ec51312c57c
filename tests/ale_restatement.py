"""rl_model_predict_ale restated with what the tests already have -- TEST INFRASTRUCTURE ONLY.  The definition of include/rlhip.h
 as plain loops: a document's own value and interval, its two scores through partial_restatement's materialised matrix
and tree_models.eval_ensemble_np, the count and the sum of every cell in the fixed order."""
import numpy as np

import partial_restatement as PD
import tree_models as TM

bits32, bits64 = PD.bits32, PD.bits64


def own_values(rows, column):
    rows = np.asarray(rows, np.float32)
    return rows[:, column].copy() if column < rows.shape[1] else np.zeros(len(rows), np.float32)


def interval_of(v, z):
    """1 + #{j in 1 .. K-1 : z_j < v} where z_0 <= v <= z_K, else 0"""
    return 1 + sum(1 for j in range(1, len(z) - 1) if z[j] < v) if z[0] <= v <= z[-1] else 0


def ale_scores(trees, weights, rows, columns, edges):
    """(int32 interval [C][n], f32 lo [C][n], f32 hi [C][n]): both scores on the materialised matrix; an outside document keeps its value"""
    ivs, los, his = [], [], []
    for c, z in zip(columns, edges):
        z, v = np.asarray(z, np.float32), own_values(rows, int(c))
        iv = np.array([interval_of(x, z) for x in v], np.int32)
        at = np.maximum(iv, 1)
        ivs.append(iv)
        los.append(TM.eval_ensemble_np(trees, weights, PD.materialise(rows, int(c), np.where(iv > 0, z[at - 1], v))))
        his.append(TM.eval_ensemble_np(trees, weights, PD.materialise(rows, int(c), np.where(iv > 0, z[at], v))))
    return np.stack(ivs), np.stack(los), np.stack(his)


def cell_sums(iv, lo, hi, K):
    """(int64 count [K], f64 S [K]) of one column, the definition's order as a plain loop"""
    count, total = np.zeros(K, np.int64), np.zeros(K, np.float64)
    with np.errstate(all="ignore"):
        d = np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)
        for p0 in range(0, len(iv), PD.SUM_BLOCK):
            part = np.zeros(K, np.float64)
            for i in range(p0, min(len(iv), p0 + PD.SUM_BLOCK)):
                if iv[i]:
                    part[iv[i] - 1] = part[iv[i] - 1] + d[i]
                    count[iv[i] - 1] += 1
            for k in range(K):
                total[k] = total[k] + part[k]
    return count, total

