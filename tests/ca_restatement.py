"""Two restatements of learning/CoorAscent.java learn() (:67-202) for the Coordinate Ascent tests.

The training loop below is the Java's, line for line (weights, steps, keep / restore decisions, -reg penalty, restarts, validation),
with the shuffle drawn from java.util.Random(seed) through Collections.shuffle.  What the loop asks for -- `scorer.score(rank(samples))`
on the cached scores, and the cache updates themselves -- comes from one of two independent scorers:

    LiteralScorer  per list: utilities/MergeSorter.java transcribed, the metric classes of tests/np_restatement.py (+ P@k and RR@k),
                   a Python float sum over the lists; the cached scores are a Python list of floats updated one document at a time
    VectorScorer   numpy: one np.lexsort per evaluation, the metrics evaluated position by position over all lists at once, the
                   list-order serial sum as np.cumsum(...)[-1]; the cached scores are an f64 array

Both take the two things -qrel puts into a scorer before any list is scored, keyed by qid: `ideal` (NDCGScorer.loadExternalRelevanceJudgment,
:50-96: idealGains entries, so score() never computes that qid's own) and `rel_doc_count` (APScorer :45-66 and :86-94: a qid the map lacks
counts 0 relevant documents and its list scores 0.0; no map at all = every list's own count).  The Java holds ONE map for every list it
scores; rlhip's rl_*_set_external_judgments takes the counts per set, so `valid_rel_doc_count` restates a validation set fed differently
(SAME = the one map, None = the validation lists' own counts); score(..., valid=True) scores with it.

Both produce the trace rlhip's rl_ca_trace returns: (kind, restart, feature index, dir, j, improved, weight, score) per restart, pass,
trial, success and validation score (kinds as _native.CA_*).
"""
import math

import numpy as np

import np_restatement as R

RESTART, PASS, TRIAL, SUCCESS, VALID = 0, 1, 2, 3, 4
MASK48 = (1 << 48) - 1


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


class JavaRandom:
    """java.util.Random as its javadoc specifies it (48-bit LCG, nextInt(bound) with the rejection loop)"""

    def __init__(self, seed):
        self.seed = (int(seed) ^ 0x5DEECE66D) & MASK48

    def next(self, bits):
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & MASK48
        return _i32(self.seed >> (48 - bits))

    def nextInt(self, bound=None):
        if bound is None:
            return self.next(32)
        if bound <= 0:
            raise ValueError("bound must be positive")
        r = self.next(31)
        m = bound - 1
        if (bound & m) == 0:
            return _i32((bound * r) >> 31)
        u = r
        while True:
            r = u % bound
            if _i32(u - r + m) >= 0:
                return r
            u = self.next(31)


def shuffle(lst, rnd):
    """Collections.shuffle(list, rnd) for a RandomAccess list: for i = size; i > 1; i--: swap(i - 1, nextInt(i))"""
    for i in range(len(lst), 1, -1):
        j = rnd.nextInt(i)
        lst[i - 1], lst[j] = lst[j], lst[i - 1]
    return lst


# ------------------------------------------------------------------------------------------------------------------------------
def merge_sort_desc(lst):
    """utilities/MergeSorter.java:130-217, sort(list, false): natural runs, then pairwise merges; returns the index order"""
    n = len(lst)
    if n == 0:
        return []
    idx = list(range(n))
    tmp = [0] * n
    ph = [0] * (n // 2 + 3)
    p = 1
    i, k = 1, 0

    def merge(s1, e1, s2, e2, k0):       # :191-217 (descending: the left element wins ties)
        i1, i2, kk = s1, s2, k0
        while i1 <= e1 and i2 <= e2:
            if lst[idx[i1]] >= lst[idx[i2]]:
                tmp[kk] = idx[i1]; i1 += 1
            else:
                tmp[kk] = idx[i2]; i2 += 1
            kk += 1
        while i1 <= e1:
            tmp[kk] = idx[i1]; i1 += 1; kk += 1
        while i2 <= e2:
            tmp[kk] = idx[i2]; i2 += 1; kk += 1

    while True:
        start = i - 1
        while i < n and lst[i] <= lst[i - 1]:
            i += 1
        if i == n:
            tmp[k:i] = idx[start:i]
            k = i
        else:
            j = i + 1
            while j < n and lst[j] <= lst[j - 1]:
                j += 1
            merge(start, i - 1, i, j - 1, k)
            i = j + 1
            k = j
        ph[p] = k
        p += 1
        if k >= n:
            break
    idx[:] = tmp[:]
    while p > 2:
        if p % 2 == 0:
            ph[p] = n
            p += 1
        k = 0
        np_ = 1
        for w in range(0, p - 1, 2):
            merge(ph[w], ph[w + 1] - 1, ph[w + 1], ph[w + 2] - 1, k)
            k = ph[w + 2]
            ph[np_] = k
            np_ += 1
        p = np_
        idx[:] = tmp[:]
    return idx


class _P:                               # metric/PrecisionScorer.java:28-40
    def __init__(self, k):
        self.k = k

    def score(self, lab, qid):
        n = len(lab)
        size = n if (self.k > n or self.k <= 0) else self.k
        return float(sum(1 for i in range(size) if lab[i] > 0.0)) / size


class _RR:                              # metric/ReciprocalRankScorer.java:24-35
    def __init__(self, k):
        self.k = k

    def score(self, lab, qid):
        size = self.k if len(lab) > self.k else len(lab)
        for i in range(size):
            if lab[i] > 0.0:
                return float(np.float32(1.0) / np.float32(i + 1))
        return 0.0


SAME = "same"                           # valid_rel_doc_count: the validation lists are scored with rel_doc_count, as the Java's one scorer does

_GAIN = np.array([R.gain(i) for i in range(32)], np.float64)       # (1 << rel) - 1 on Java ints, by rel & 31


class LiteralScorer:
    def __init__(self, metric, k, err_max=16.0, ideal=None, rel_doc_count=None, valid_rel_doc_count=SAME):
        if metric == "ERR":
            self.m = R.ERR(k)
            self.m.MAX = err_max
        elif metric == "NDCG":
            self.m = R.NDCG(k, ideal)
        elif metric == "MAP":
            self.m = R.MAP(k, rel_doc_count)
        else:
            self.m = {"DCG": R.DCG, "P": _P, "RR": _RR}[metric](k)
        self.mv = self.m                # the validation lists' scorer: the same object (one idealGains cache), unless their counts differ
        if metric == "MAP" and valid_rel_doc_count is not SAME:
            self.mv = R.MAP(k, valid_rel_doc_count)

    def new_cache(self, n):
        return [0.0] * n

    def dot(self, X, w):                # rank() with current_feature == -1 (:207-213)
        out = []
        for row in X:
            s = 0.0
            for j in range(len(w)):
                s += w[j] * float(row[j])
            out.append(s)
        return out

    def update(self, cache, x, wc, div=None):     # updateCached / scaleCached
        out = [c + wc * float(v) for c, v in zip(cache, x)]
        if div is not None:
            out = [c / div for c in out]
        return out

    def score(self, cache, labels, qoff, qid, valid=False):
        m = self.mv if valid else self.m
        s = 0.0
        for q in range(len(qoff) - 1):
            a, b = int(qoff[q]), int(qoff[q + 1])
            order = merge_sort_desc(cache[a:b])
            s += m.score([float(labels[a + i]) for i in order], qid[q])
        return s / (len(qoff) - 1)


class VectorScorer:
    def __init__(self, metric, k, err_max=16.0, ideal=None, rel_doc_count=None, valid_rel_doc_count=SAME):
        self.metric, self.k, self.err_max = metric, k, err_max
        self.ideal = dict(ideal) if ideal else {}     # NDCGScorer.idealGains: keyed by qid, -qrel entries first, then filled in the order lists are first scored
        self.rdc = rel_doc_count
        self.vrdc = rel_doc_count if valid_rel_doc_count is SAME else valid_rel_doc_count

    def new_cache(self, n):
        return np.zeros(n, np.float64)

    def dot(self, X, w):
        s = np.zeros(X.shape[0], np.float64)
        for j in range(len(w)):
            s = s + w[j] * X[:, j].astype(np.float64)
        return s

    def update(self, cache, x, wc, div=None):
        out = cache + wc * x.astype(np.float64)
        return out if div is None else out / div

    def score(self, cache, labels, qoff, qid, valid=False):
        qoff = np.asarray(qoff, np.int64)
        Q = len(qoff) - 1
        n = np.diff(qoff)
        qdoc = np.repeat(np.arange(Q), n)
        order = np.lexsort((np.arange(len(cache)), -cache, qdoc))
        lab = np.asarray(labels, np.float32)[order]
        k = self.k
        size = np.where((k > n) | (k <= 0), n, k)
        res = np.zeros(Q, np.float64)
        if self.metric in ("NDCG", "DCG"):
            if self.metric == "NDCG":
                ideal = np.zeros(Q)
                for q in range(Q):
                    if qid[q] not in self.ideal:
                        rel = np.asarray(labels[qoff[q]:qoff[q + 1]], np.float32).astype(np.int64)
                        self.ideal[qid[q]] = R.ideal_dcg(list(rel), int(size[q]))
                    ideal[q] = self.ideal[qid[q]]
            dcg = np.zeros(Q)
            for p in range(int(size.max())):
                on = size > p
                rel = lab[qoff[:-1][on] + p].astype(np.int64)
                dcg[on] = dcg[on] + _GAIN[rel & 31] * R.discount(p)
            res = dcg if self.metric == "DCG" else np.where(ideal > 0.0, dcg / np.where(ideal > 0.0, ideal, 1.0), 0.0)
        elif self.metric == "MAP":
            ap, cnt = np.zeros(Q), np.zeros(Q, np.int64)
            if int(n.max()) > 4 * Q:      # a speed path for few long lists: list by list, the serial sum as np.cumsum (a non-relevant document adds 0.0: no change)
                for q in range(Q):
                    rel = lab[qoff[q]:qoff[q + 1]] > 0.0
                    c = np.cumsum(rel)
                    ap[q] = np.cumsum(np.where(rel, c / np.arange(1, len(c) + 1, dtype=np.float64), 0.0))[-1]
                    cnt[q] = c[-1]
            else:
                for p in range(int(n.max())):
                    on = n > p
                    rel = lab[qoff[:-1][on] + p] > 0.0
                    c = cnt[on] + rel
                    cnt[on] = c
                    ap[on] = np.where(rel, ap[on] + c / float(p + 1), ap[on])
            rdc = self.vrdc if valid else self.rdc
            rd = cnt if rdc is None else np.array([rdc.get(qid[q], 0) for q in range(Q)], np.int64)
            res = np.where(rd > 0, ap / np.maximum(rd, 1), 0.0)
        elif self.metric == "ERR":
            sc, pp = np.zeros(Q), np.ones(Q)
            for p in range(int(size.max())):
                on = size > p
                Rr = _GAIN[lab[qoff[:-1][on] + p].astype(np.int64) & 31] / self.err_max
                sc[on] = sc[on] + pp[on] * Rr / (p + 1)
                pp[on] = pp[on] * (1.0 - Rr)
            res = sc
        elif self.metric == "P":
            cnt = np.zeros(Q)
            for p in range(int(size.max())):
                on = size > p
                cnt[on] += lab[qoff[:-1][on] + p] > 0.0
            res = cnt / size
        elif self.metric == "RR":
            rsize = np.where(n > k, k, n)
            first = np.zeros(Q, np.int64)
            for p in range(int(max(rsize.max(), 0))):
                on = (rsize > p) & (first == 0)
                hit = lab[qoff[:-1][on] + p] > 0.0
                idx = np.nonzero(on)[0][hit]
                first[idx] = p + 1
            res = np.where(first > 0, (np.float32(1.0) / np.maximum(first, 1).astype(np.float32)).astype(np.float64), 0.0)
        return float(np.cumsum(res)[-1] / Q)


# ------------------------------------------------------------------------------------------------------------------------------
def _distance(w1, w2):                  # :350-364
    s1 = s2 = 0.0
    for a, b in zip(w1, w2):
        s1 += abs(a)
        s2 += abs(b)
    d = 0.0
    for a, b in zip(w1, w2):
        t = a / s1 - b / s2
        d += t * t
    return math.sqrt(d)


def _normalize(w):                      # :366-382
    s = 0.0
    for v in w:
        s += abs(v)
    if s > 0:
        for j in range(len(w)):
            w[j] /= s
    else:
        s = 1
        for j in range(len(w)):
            w[j] = 1.0 / len(w)
    return s


def learn(train, valid=None, metric="NDCG", k=10, nRestart=5, nMaxIteration=25, stepBase=0.05, stepScale=2.0, tolerance=0.001,
          regularized=False, slack=0.001, seed=0, err_max=16.0, literal=False, ideal=None, rel_doc_count=None, valid_rel_doc_count=SAME):
    """train / valid: (X [n, F] float32, labels, qoff, qid list).  Returns dict(weight, train, valid, trace)."""
    sc = (LiteralScorer if literal else VectorScorer)(metric, k, err_max, ideal, rel_doc_count, valid_rel_doc_count)
    X, lab, qoff, qid = train
    F = X.shape[1]
    cols = [X[:, f] for f in range(F)]
    weight = [1.0 / F] * F                                  # init()
    regVector = list(weight)
    bestModel, bestModelScore = None, 0.0
    trace = []
    rnd = JavaRandom(seed)
    for r in range(nRestart):
        consecutive_fails = 0
        weight = [float(np.float32(1.0) / np.float32(F))] * F
        cache = sc.dot(X, weight)
        startScore = sc.score(cache, lab, qoff, qid)
        trace.append((RESTART, r, -1, 0, 0, 0, 0.0, startScore))
        bestScore = startScore
        bestWeight = list(weight)
        npass = 0
        while (F > 1 and consecutive_fails < F - 1) or (F == 1 and consecutive_fails == 0):
            trace.append((PASS, r, -1, 0, npass, 0, 0.0, bestScore))
            npass += 1
            fids = shuffle(list(range(F)), rnd)
            for f in fids:
                origWeight = weight[f]
                totalStep = bestTotalStep = 0.0
                succeeds = False
                for s, d in enumerate((1, -1, 0)):
                    step = 0.001 * d
                    if origWeight != 0.0 and abs(step) > 0.5 * abs(origWeight):
                        step = stepBase * abs(origWeight)
                    totalStep = step
                    numIter = nMaxIteration
                    if d == 0:
                        numIter = 1
                        totalStep = -origWeight
                    for j in range(numIter):
                        w = origWeight + totalStep
                        cache = sc.update(cache, cols[f], step)
                        weight[f] = w
                        score = sc.score(cache, lab, qoff, qid)
                        if regularized:
                            score -= slack * _distance(weight, regVector)
                        imp = score > bestScore
                        if imp:
                            bestScore, bestTotalStep, succeeds = score, totalStep, True
                        trace.append((TRIAL, r, f, d, j, int(imp), w, score))
                        if j < nMaxIteration - 1:
                            step *= stepScale
                            totalStep += step
                    if succeeds:
                        break
                    elif s < 2:
                        cache = sc.update(cache, cols[f], -totalStep)
                        weight[f] = origWeight
                if succeeds:
                    weight[f] = origWeight + bestTotalStep
                    consecutive_fails = 0
                    tot = _normalize(weight)
                    cache = sc.update(cache, cols[f], bestTotalStep - totalStep, tot)
                    bestWeight = list(weight)
                    trace.append((SUCCESS, r, f, 0, 0, 0, weight[f], bestScore))
                else:
                    consecutive_fails += 1
                    cache = sc.update(cache, cols[f], -totalStep)
                    weight[f] = origWeight
            if bestScore - startScore < tolerance:
                break
        if valid is not None:
            bestScore = sc.score(sc.dot(valid[0], weight), valid[1], valid[2], valid[3], valid=True)
            trace.append((VALID, r, -1, 0, 0, 0, 0.0, bestScore))
        if bestModel is None or bestScore > bestModelScore:
            bestModelScore, bestModel = bestScore, bestWeight
    weight = list(bestModel)
    ts = sc.score(sc.dot(X, weight), lab, qoff, qid)
    vs = sc.score(sc.dot(valid[0], weight), valid[1], valid[2], valid[3], valid=True) if valid is not None else None
    return dict(weight=weight, train=ts, valid=vs, trace=trace)


def dot_scores(X, features, weight):
    """CoorAscent.eval over rows (X[:, fid] = feature fid): 0.0 + w[0] x[f0] + ... in f64"""
    s = np.zeros(X.shape[0], np.float64)
    for f, w in zip(features, weight):
        s = s + w * X[:, f].astype(np.float64)
    return s
