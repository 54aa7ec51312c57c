"""A literal restatement of learning/boosting/AdaRank.java learn() (:97-262) for the AdaRank tests.

The loop below is the Java's, line for line: the candidate choice over the features list (:74-95), the enqueue / rollback phase and the
queue phases (:107-126, :234-243), the "F. REM." removals (:152-174), the best model on validation data, the stop (:189-194) and the sample
weights (:197-199).  Weak rankers rank a list with utilities/Sorter.sort(double[], false) (the selection sort with swaps, transcribed
below); the ensemble ranks with utilities/MergeSorter (ca_restatement.merge_sort_desc) on eval() = 0.0 + w0 x[f0] + w1 x[f1] + ...,
recomputed from scratch for every ranking.  The metrics are ca_restatement's LiteralScorer's; log and exp are Python's math module.

The trace has the records rlhip's rl_ada_trace returns: (iteration, kind, feature index, status, alpha, train score, validation score).
"""
import math

import numpy as np

import ca_restatement as CR

ROUND, ROLLBACK, PHASE = 0, 1, 2
OK, DAMN, FREM = 0, 1, 2


class NonFiniteAlpha(Exception):
    """alpha_t = 0.5 ln(num / denom) is not finite: rlhip refuses the round (the Java goes on)"""


def sorter_sort(vals):
    """utilities/Sorter.java sort(double[], false), transcribed: the index order"""
    idx = list(range(len(vals)))
    for i in range(len(vals) - 1):
        mx = i
        for j in range(i + 1, len(vals)):
            if vals[idx[mx]] < vals[idx[j]]:
                mx = j
        idx[i], idx[mx] = idx[mx], idx[i]
    return idx


def sorter_sort_np(vals, steps=None):
    """the same order with numpy: step i takes the first position >= i that holds the maximum (np.argmax returns the first), swaps it into
    slot i; only the first `steps` positions are final when steps < len(vals) - 1"""
    v = np.asarray(vals, np.float64).copy()
    idx = np.arange(len(v))
    n = len(v) - 1 if steps is None else min(steps, len(v) - 1)
    for i in range(n):
        m = i + int(np.argmax(v[i:]))
        v[i], v[m] = v[m], v[i]
        idx[i], idx[m] = idx[m], idx[i]
    return list(idx)


def _steps(metric, k, n):
    size = n if (k > n or k <= 0) else k
    return n - 1 if metric == "MAP" else size


def weak_table(X, lab, qoff, qid, sc, metric, k):
    """M[f][q] = scorer.score(WeakRanker(f).rank(list q)), lists in order for each feature"""
    F, Q = X.shape[1], len(qoff) - 1
    M = np.zeros((F, Q), np.float64)
    for f in range(F):
        for q in range(Q):
            a, b = int(qoff[q]), int(qoff[q + 1])
            order = sorter_sort_np(X[a:b, f], _steps(metric, k, b - a))
            M[f, q] = sc.m.score([float(lab[a + i]) for i in order], qid[q])
    return M


def _eval(X, rankers, rweight):
    """AdaRank.eval (:265-271) of every row: 0.0 + w0 * x[f0] + ... in f64, left to right"""
    out = []
    for row in X:
        s = 0.0
        for f, w in zip(rankers, rweight):
            s += w * float(row[f])
        out.append(s)
    return out


def _per_list(sc, cache, lab, qoff, qid):
    m = []
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        order = CR.merge_sort_desc(cache[a:b])
        m.append(sc.m.score([float(lab[a + i]) for i in order], qid[q]))
    return m


def learn(train, valid=None, metric="NDCG", k=10, nIteration=500, tolerance=0.002, trainWithEnqueue=True, maxSelCount=5, err_max=16.0,
          ideal=None, rel_doc_count=None, valid_rel_doc_count=CR.SAME):
    """train / valid: (X [n, F] float32, labels, qoff, qid list).  Returns dict(fid, weight, train, valid, trace, M, restored):
    restored = the best model on validation data replaced a different final ensemble."""
    sc = CR.LiteralScorer(metric, k, err_max, ideal, rel_doc_count, valid_rel_doc_count)      # -qrel: see ca_restatement
    X, lab, qoff, qid = train
    F, Q = X.shape[1], len(qoff) - 1
    M = weak_table(X, lab, qoff, qid, sc, metric, k)
    st = dict(used=set(), queue=[], lastFeature=-1, lastCount=0, backupTrainScore=0.0, lastTrainedScore=-1.0, bestValid=0.0)
    sweight = [float(np.float32(1.0) / np.float32(Q))] * Q                 # init() :212, a float division
    backup = list(sweight)
    rankers, rweight, bestRankers, bestWeights = [], [], [], []
    trace = []

    def learn_phase(start, withEnqueue):
        nonlocal sweight, backup, rankers, rweight, bestRankers, bestWeights
        t = start
        while t <= nIteration:
            best, bestScore = -1, -1.0                                      # learnWeakRanker :74-95
            for f in range(F):
                if f in st["queue"] or f in st["used"]:
                    continue
                s = 0.0
                for j in range(Q):
                    s += M[f, j] * sweight[j]
                if bestScore < s:
                    bestScore, best = s, f
            if best < 0:
                break
            if withEnqueue:
                if best == st["lastFeature"]:                               # :108-119
                    st["queue"].append(st["lastFeature"])
                    rankers.pop()
                    rweight.pop()
                    sweight = list(backup)
                    st["bestValid"] = 0.0
                    st["lastTrainedScore"] = st["backupTrainScore"]
                    trace.append((t, ROLLBACK, best, 0, 0.0, 0.0, 0.0))
                    t += 1
                    continue
                st["lastFeature"] = best
                backup = list(sweight)
                st["backupTrainScore"] = st["lastTrainedScore"]
            num = denom = 0.0
            for i in range(Q):
                tmp = M[best, i]
                num += sweight[i] * (1.0 + tmp)
                denom += sweight[i] * (1.0 - tmp)
            if denom == 0.0 or num / denom <= 0.0 or math.isinf(num / denom):
                raise NonFiniteAlpha("round %d, feature %d, num %r, denom %r" % (t, best, num, denom))
            rankers.append(best)
            alpha = 0.5 * (math.log(num / denom) / math.log(math.e))       # SimpleMath.ln
            rweight.append(alpha)
            m = _per_list(sc, _eval(X, rankers, rweight), lab, qoff, qid)
            trainedScore = total = 0.0
            for tmp in m:
                total += math.exp(-alpha * tmp)
                trainedScore += tmp
            trainedScore /= Q
            delta = trainedScore + tolerance - st["lastTrainedScore"]
            status = OK if delta > 0 else DAMN
            if not withEnqueue:                                             # :152-174
                if trainedScore != st["lastTrainedScore"]:
                    st["lastCount"] = 0
                    st["used"].clear()
                elif st["lastFeature"] == best:
                    st["lastCount"] += 1
                    if st["lastCount"] == maxSelCount:
                        status = FREM
                        st["lastCount"] = 0
                        st["used"].add(st["lastFeature"])
                else:
                    st["lastCount"] = 0
                    st["used"].clear()
                st["lastFeature"] = best
            vs = 0.0
            if valid is not None:                                           # :177-183
                vs = sc.score(_eval(valid[0], rankers, rweight), valid[1], valid[2], valid[3], valid=True)
                if vs > st["bestValid"]:
                    st["bestValid"] = vs
                    bestRankers, bestWeights = list(rankers), list(rweight)
            trace.append((t, ROUND, best, status, alpha, trainedScore, vs))
            if delta <= 0:                                                  # :189-194
                rankers.pop()
                rweight.pop()
                break
            st["lastTrainedScore"] = trainedScore
            for i in range(Q):
                sweight[i] *= math.exp(-alpha * m[i]) / total
            t += 1
        return t

    if trainWithEnqueue:                                                    # :234-243
        trace.append((1, PHASE, -1, 1, 0.0, 0.0, 0.0))
        t = learn_phase(1, True)
        for i in range(len(st["queue"]) - 1, -1, -1):
            f = st["queue"].pop(i)
            trace.append((t, PHASE, f, 0, 0.0, 0.0, 0.0))
            t = learn_phase(t, False)
    else:
        trace.append((1, PHASE, -1, 0, 0.0, 0.0, 0.0))
        learn_phase(1, False)
    restored = False
    if valid is not None and bestRankers:                                   # :247-252
        restored = (bestRankers, bestWeights) != (rankers, rweight)
        rankers, rweight = list(bestRankers), list(bestWeights)
    ts = sc.score(_eval(X, rankers, rweight), lab, qoff, qid)
    vs = sc.score(_eval(valid[0], rankers, rweight), valid[1], valid[2], valid[3], valid=True) if valid is not None else None
    return dict(fid=rankers, weight=rweight, train=ts, valid=vs, trace=trace, M=M, restored=restored)
