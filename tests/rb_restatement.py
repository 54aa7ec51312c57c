"""A literal restatement of learning/boosting/RankBoost.java init() and learn() (:143-346) for the RankBoost tests.

init(): every training list is replaced by getCorrectRanking() (utilities/Sorter.sort on the labels: ada_restatement.sorter_sort, the
unstable selection sort), the crucial pairs are counted, sweight[i][j][k] is dense (1 / totalCorrectPairs on crucial pairs, 0.0 elsewhere
above the diagonal), the thresholds are doubles (the -1E6 / 1E6 start values, the repeated subtraction, fmin - 1.0E8; or every feature
value for nThreshold <= 0), tSortedIdx and the per-list feature orders come from utilities/MergeSorter (ca_restatement.merge_sort_desc).
learn(): updatePotential, the three-level candidate loop of learnWeakRanker with `last[]` and the strict `r > maxR` carried across
features, alpha_t through SimpleMath.ln, D_t[j][k] = sweight * Math.exp(alpha_t * (h(k) - h(j))) with Z_t one running double over every
pair of every list, the metrics through ca_restatement's LiteralScorer on eval() recomputed from scratch, the best prefix on validation
data, then sweight /= Z_t.  log and exp are Python's math module.

`vector=True` keeps the same dense state and the same orders of every sum with numpy (np.cumsum is a serial accumulation; exp is still
math.exp, looked up per distinct argument): for lists too long for Python loops.  tests/test_rb_cpu.py holds the two forms equal.

The trace has the records rlhip's rl_rb_trace returns: (iteration, feature index, threshold, maxR, R_t, alpha_t, Z_t, train score,
validation score).
"""
import math

import numpy as np

import ca_restatement as CR
from ada_restatement import sorter_sort


class NonFiniteRound(Exception):
    """alpha_t, exp(alpha_t) or Z_t is not finite (or Z_t is 0), or no pair is crucial: rlhip refuses (the Java goes on)"""

    def __init__(self, round_, what):
        super().__init__("round %d: %s" % (round_, what))
        self.round = round_


def correct_ranking(X, lab, qoff):
    """every list in getCorrectRanking()'s order: (X, labels) permuted, and the permutation (new position -> input row)"""
    perm = []
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        perm += [a + i for i in sorter_sort([float(v) for v in lab[a:b]])]
    perm = np.array(perm, np.int64)
    return X[perm], lab[perm], perm


def thresholds(X, nThreshold):
    """thresholds[f] as a list of doubles (:188-243); X in list order, float32"""
    n, F = X.shape
    if nThreshold <= 0:
        return [[float(X[i, f]) for i in range(n)] for f in range(F)]
    out = []
    for f in range(F):
        fmax, fmin = -1E6, 1E6
        for i in range(n):
            v = float(X[i, f])
            if v > fmax:
                fmax = v
            if v < fmin:
                fmin = v
        step = abs(fmax - fmin) / nThreshold
        t = [0.0] * (nThreshold + 1)
        t[0] = fmax
        for j in range(1, nThreshold):
            t[j] = t[j - 1] - step
        t[nThreshold] = fmin - 1.0E8
        out.append(t)
    return out


def _ln(x):
    return math.log(x) / math.log(math.e)                   # SimpleMath.ln


def _eval(X, rankers, weights):
    """RankBoost.eval (:348-355) of every row: 0.0 + w0 * h0(x) + ... in f64, left to right"""
    out = []
    for row in X:
        s = 0.0
        for (f, thr), w in zip(rankers, weights):
            s += w * (1 if float(row[f]) > thr else 0)
        out.append(s)
    return out


def _eval_np(X, rankers, weights):
    s = np.zeros(X.shape[0], np.float64)
    for (f, thr), w in zip(rankers, weights):
        s = s + w * (X[:, f].astype(np.float64) > thr).astype(np.float64)
    return [float(v) for v in s]


def learn(train, valid=None, metric="NDCG", k=10, nIteration=300, nThreshold=10, err_max=16.0, vector=False, keep_potentials=0,
          ideal=None, rel_doc_count=None, valid_rel_doc_count=CR.SAME):
    """train / valid: (X [n, F] float32, labels, qoff, qid list).  Returns dict(fid, thr, weight, train, valid, trace, restored,
    pots): restored = the best prefix on validation data is shorter than the full model; pots[t - 1] = the potentials of round t in
    the corrected order (keep_potentials rounds); a non-finite round raises NonFiniteRound."""
    sc = CR.LiteralScorer(metric, k, err_max, ideal, rel_doc_count, valid_rel_doc_count)      # -qrel: see ca_restatement
    X0, lab0, qoff, qid = train
    X, lab, _ = correct_ranking(X0, lab0, qoff)                               # init() :152
    F, Q = X.shape[1], len(qoff) - 1
    ev = _eval_np if vector else _eval
    lists = [(int(qoff[q]), int(qoff[q + 1])) for q in range(Q)]
    total = 0
    for a, b in lists:
        n = b - a
        for j in range(n - 1):
            kk = n - 1
            while kk >= j + 1 and lab[a + j] > lab[a + kk]:
                total += 1
                kk -= 1
    if total == 0:
        raise NonFiniteRound(1, "no crucial pair: 1.0 / totalCorrectPairs divides by zero")
    sweight = []
    for a, b in lists:
        n = b - a
        if vector:
            l = lab[a:b].astype(np.float64)
            sweight.append(np.where(np.triu(l[:, None] > l[None, :], 1), 1.0 / total, 0.0))
        else:
            sweight.append([[(1.0 / total if lab[a + j] > lab[a + kk] else 0.0) if kk > j else 0.0 for kk in range(n)] for j in range(n)])
    th = thresholds(X, nThreshold)
    tsorted = [CR.merge_sort_desc(t) for t in th]
    ssorted = [[CR.merge_sort_desc([float(v) for v in X[a:b, f]]) for a, b in lists] for f in range(F)]
    wRankers, rWeight, best_len, bestValid = [], [], 0, 0.0
    trace, pots = [], []
    Z_t = 1.0
    for t in range(1, nIteration + 1):
        potential = []                                                        # updatePotential :75-89
        for i, (a, b) in enumerate(lists):
            n = b - a
            sw = sweight[i]
            if vector:
                potential.append([float(np.cumsum(np.concatenate(([0.0], sw[j, j + 1:], -sw[:j, j])))[-1]) for j in range(n)])
                continue
            pp = []
            for j in range(n):
                p = 0.0
                for kk in range(j + 1, n):
                    p += sw[j][kk]
                for kk in range(j):
                    p -= sw[kk][j]
                pp.append(p)
            potential.append(pp)
        if t <= keep_potentials:
            pots.append(np.array([p for pp in potential for p in pp], np.float64))
        bestFid, maxR, bestThreshold = -1, -10.0, -1.0                        # learnWeakRanker :96-141
        for f in range(F):
            last = [-1] * Q
            r = 0.0
            for e in tsorted[f]:
                tv = th[f][e]
                for q, (a, b) in enumerate(lists):
                    sk = ssorted[f][q]
                    l = last[q] + 1
                    while l < b - a:
                        if float(X[a + sk[l], f]) > tv:
                            r += potential[q][sk[l]]
                            last[q] = l
                        else:
                            break
                        l += 1
                if r > maxR:
                    maxR, bestThreshold, bestFid = r, tv, f
        if bestFid == -1:
            break
        R_t = Z_t * maxR
        den = Z_t - R_t
        ratio = (Z_t + R_t) / den if den != 0.0 else math.inf
        if not (ratio > 0.0) or math.isinf(ratio):
            raise NonFiniteRound(t, "alpha_t = 0.5 ln(%r / %r), maxR = %r" % (Z_t + R_t, den, maxR))
        alpha_t = 0.5 * _ln(ratio)
        try:
            math.exp(alpha_t)
        except OverflowError:
            raise NonFiniteRound(t, "exp(alpha_t) with alpha_t = %r" % alpha_t)
        wRankers.append((bestFid, bestThreshold))
        rWeight.append(alpha_t)
        Z_t = 0.0                                                             # :282-297
        for i, (a, b) in enumerate(lists):
            n = b - a
            h = [1 if float(X[a + j, bestFid]) > bestThreshold else 0 for j in range(n)]
            if vector:
                if n < 2:
                    continue
                hv = np.array(h, np.float64)
                arg = alpha_t * (hv[None, :] - hv[:, None])
                u, inv = np.unique(arg, return_inverse=True)
                D = sweight[i] * np.array([math.exp(v) for v in u])[inv].reshape(n, n)
                D = np.triu(D, 1)
                Z_t = float(np.cumsum(np.concatenate(([Z_t], D[np.triu_indices(n, 1)])))[-1])
                sweight[i] = D
                continue
            D = [[0.0] * n for _ in range(n)]
            for j in range(n - 1):
                for kk in range(j + 1, n):
                    D[j][kk] = sweight[i][j][kk] * math.exp(alpha_t * (h[kk] - h[j]))
                    Z_t += D[j][kk]
            sweight[i] = D
        if not math.isfinite(Z_t) or Z_t == 0.0:
            raise NonFiniteRound(t, "Z_t = %r" % Z_t)
        ts = sc.score(ev(X, wRankers, rWeight), lab, qoff, qid)
        vs = 0.0
        if valid is not None:
            vs = sc.score(ev(valid[0], wRankers, rWeight), valid[1], valid[2], valid[3], valid=True)
            if vs > bestValid:
                bestValid, best_len = vs, len(wRankers)
        trace.append((t, bestFid, bestThreshold, maxR, R_t, alpha_t, Z_t, ts, vs))
        for i, (a, b) in enumerate(lists):                                    # :319-327
            n = b - a
            if vector:
                sweight[i] = sweight[i] / Z_t
                continue
            for j in range(n - 1):
                for kk in range(j + 1, n):
                    sweight[i][j][kk] /= Z_t
    restored = False
    if valid is not None and best_len > 0:                                    # :333-338
        restored = best_len < len(wRankers)
        wRankers, rWeight = wRankers[:best_len], rWeight[:best_len]
    ts = sc.score(ev(X, wRankers, rWeight), lab, qoff, qid)
    vs = sc.score(ev(valid[0], wRankers, rWeight), valid[1], valid[2], valid[3], valid=True) if valid is not None else None
    return dict(fid=[f for f, _ in wRankers], thr=[v for _, v in wRankers], weight=rWeight, train=ts, valid=vs, trace=trace,
                restored=restored, pots=pots)
