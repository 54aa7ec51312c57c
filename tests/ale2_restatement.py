"""rl_model_predict_ale2 restated with what the tests already have -- TEST INFRASTRUCTURE ONLY.  The definition of include/rlhip.h
 as plain loops: a document's own two intervals (ale_restatement.interval_of), its four scores through
partial_restatement's materialised matrix applied twice and tree_models.eval_ensemble_np, the count and the sum of every cell in the
three-level fixed order."""
import numpy as np

import ale_restatement as AR
import partial_restatement as PD
import tree_models as TM

SUPER = 64
bits32, bits64 = PD.bits32, PD.bits64


def intervals(v, z):
    """interval_of of every value, taken once per distinct bit pattern"""
    u, inv = np.unique(bits32(v), return_inverse=True)
    return np.array([AR.interval_of(x, z) for x in u.view(np.float32)], np.int32)[inv]


def ale2_scores(trees, weights, rows, pairs, edges):
    """(int32 cell [P][n], f32 corner [P][4][n]): the four scores on the materialised matrices; an outside document keeps its values"""
    cells, corners = [], []
    for (a, b), (za, zb) in zip(pairs, edges):
        za, zb = np.asarray(za, np.float32), np.asarray(zb, np.float32)
        va, vb = AR.own_values(rows, int(a)), AR.own_values(rows, int(b))
        k, l = intervals(va, za), intervals(vb, zb)
        inside = (k > 0) & (l > 0)
        ka, la = np.maximum(k, 1), np.maximum(l, 1)
        cells.append(np.where(inside, (k - 1) * (len(zb) - 1) + (l - 1), -1).astype(np.int32))
        corners.append(np.stack([TM.eval_ensemble_np(trees, weights, PD.materialise(PD.materialise(rows, int(a), np.where(inside, za[ka - 1 + ua], va)),
                                                                                    int(b), np.where(inside, zb[la - 1 + ub], vb)))
                                 for ua in (0, 1) for ub in (0, 1)]))
    return np.stack(cells), np.stack(corners)


def cell_sums(cell, corner, cells):
    """(int64 count [cells], f64 S [cells]) of one pair: partials of 256 documents, super-partials of 64 partials, the total"""
    count, total = np.zeros(cells, np.int64), np.zeros(cells, np.float64)
    s = np.asarray(corner, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = (s[3] - s[1]) - (s[2] - s[0])
        for q0 in range(0, len(cell), SUPER * PD.SUM_BLOCK):
            sup = np.zeros(cells, np.float64)
            for p0 in range(q0, min(len(cell), q0 + SUPER * PD.SUM_BLOCK), PD.SUM_BLOCK):
                part = np.zeros(cells, np.float64)
                for i in range(p0, min(len(cell), p0 + PD.SUM_BLOCK)):
                    if cell[i] >= 0:
                        part[cell[i]] = part[cell[i]] + d[i]
                        count[cell[i]] += 1
                sup = sup + part
            total = total + sup
    return count, total
