"""Literal restatement of LambdaRank training in plain Python -- TEST INFRASTRUCTURE ONLY.

LambdaRank.java's four overrides (batchFeedForward :34-65, batchBackPropagate :68-83, internalReorder :86-88 = Ranker.rank :88-95,
computePairWeight :91-102) and estimateLoss (:105-128, the count), the pairWeight != null arms of Neuron.computeDelta (:111-120) and
updateDelta (:128-150), and the scorers' swapChange (NDCGScorer.java:132-160, DCGScorer.java:74-90, APScorer.java:108-162 with its
rdCount, ERRScorer.java:76-115), on the network objects net_restatement.Net.wire() makes.  The forward pass, updateWeight, the seeded
draw, the scores and the mis-ordered count are ranknet_restatement's: LambdaRank inherits them.  Python floats are Java doubles,
numpy.float32 the Java floats (the pair weight and the target value), widened where the Java widens them.

epoch_vector is the same pass over weight matrices with the pair loops as numpy element-wise f64 operations and np.cumsum for the serial
sums, for lists too long for the literal form; tests/test_lambdarank_cpu.py holds both equal bit for bit.
"""
import numpy as np

import ca_restatement as CR
import np_restatement as R
import ranknet_restatement as RN
from listnet_restatement import RestoreError
from np_restatement import jexp

TRAINABLE = ("NDCG", "DCG", "MAP", "ERR")


# ---- Ranker.rank: MergeSorter.sort(double[], false), finite scores -----------------------------------------------------------------------
def rank(scores):
    """positions -> documents: descending, the left one wins on >= (stable)"""
    return sorted(range(len(scores)), key=lambda j: -scores[j])


# ---- the scorers' swapChange --------------------------------------------------------------------------------------------------------------
def map_swap_change(lab_ranked, rd_count):       # APScorer.java:108-162; rd_count: None = no -qrel (the list's own count)
    n = len(lab_ranked)
    labels, relCount, count = [], [], 0
    for l in lab_ranked:
        labels.append(1 if l > 0 else 0)
        count += labels[-1]
        relCount.append(count)
    rdCount = count if rd_count is None else rd_count
    changes = [[0.0] * n for _ in range(n)]
    if rdCount == 0 or count == 0:
        return changes
    for i in range(n - 1):
        for j in range(i + 1, n):
            change = 0.0
            if labels[i] != labels[j]:
                diff = labels[j] - labels[i]
                change += float((relCount[i] + diff) * labels[j] - relCount[i] * labels[i]) / (i + 1)
                for k in range(i + 1, j):
                    if labels[k] > 0:
                        change += float(diff) / (k + 1)
                change += float(-relCount[j] * diff) / (j + 1)
            changes[j][i] = changes[i][j] = change / rdCount
    return changes


class Scorer:
    """the train metric as LambdaRank uses it: swapChange on a re-ranked list.  sc is the run's ca_restatement.LiteralScorer, so NDCG's
    idealGains cache is the one score() fills, as in the Java"""

    def __init__(self, sc, metric, k, rel_doc_count):
        assert metric in TRAINABLE
        self.sc, self.metric, self.k, self.rdc = sc, metric, k, rel_doc_count

    def rd(self, qid):
        return None if self.rdc is None else self.rdc.get(qid, 0)

    def swap_change(self, lab_ranked, qid):
        with np.errstate(all="ignore"):
            if self.metric == "MAP":
                return map_swap_change(lab_ranked, self.rd(qid))
            return self.sc.m.swap_change([float(v) for v in lab_ranked], qid)

    def swap_abs_vector(self, lab_ranked, qid):
        """|swapChange| as an [n, n] array, element-wise over j (and np.cumsum for MAP's serial chain)"""
        lab = np.asarray(lab_ranked, np.float32)
        n = len(lab)
        C = np.zeros((n, n), np.float64)
        size = self.k if n > self.k else n
        J = np.arange(n)
        with np.errstate(all="ignore"):
            if self.metric in ("NDCG", "DCG"):
                rel = [int(v) for v in lab]
                g = np.array([float(R.gain(r)) for r in rel], np.float64)
                d = np.array([R.discount(i) for i in range(n)], np.float64)
                ideal = 1.0
                if self.metric == "NDCG":
                    ideal = self.sc.m.ideal_gains.get(qid)
                    if ideal is None:
                        ideal = R.ideal_dcg(rel, size)
                for i in range(max(size, 0)):
                    if self.metric == "NDCG" and not ideal > 0:
                        break
                    v = (d[i] - d[i + 1:]) * (g[i] - g[i + 1:])
                    C[i, i + 1:] = v / ideal if self.metric == "NDCG" else v
            elif self.metric == "MAP":
                lb = (lab > 0).astype(np.int64)
                rc = np.cumsum(lb)
                count = int(rc[-1]) if n else 0
                rd = count if self.rd(qid) is None else self.rd(qid)
                if rd != 0 and count != 0:
                    for i in range(n - 1):
                        diff = 1 - 2 * int(lb[i])                                  # labels[j] - labels[i] where they differ
                        lj = 1 - int(lb[i])
                        c0 = float((int(rc[i]) + diff) * lj - int(rc[i]) * int(lb[i])) / (i + 1)
                        terms = np.where(lb[i + 1:] > 0, float(diff) / (J[i + 1:] + 1), 0.0)      # k = i + 1 .. n - 1; + 0.0 changes a sign at most
                        pre = np.cumsum(np.concatenate([[0.0, c0], terms]))[1:]    # pre[m]: the chain up to k = i + m
                        last = (-rc[i + 1:] * diff).astype(np.float64) / (J[i + 1:] + 1)
                        ch = (pre[:n - 1 - i] + last) / rd
                        C[i, i + 1:] = np.where(lb[i + 1:] != lb[i], ch, 0.0)
            else:
                m = self.sc.m
                labels, Rv, npp = np.zeros(n, np.int64), np.zeros(n, np.float64), np.zeros(n, np.float64)
                p = 1.0
                for i in range(size):
                    labels[i] = int(lab[i])
                    Rv[i] = m.R(int(labels[i]))
                    npp[i] = p * (1.0 - Rv[i])
                    p *= npp[i]
                for i in range(size):
                    base = 1.0 if i == 0 else npp[i - 1]
                    v1 = 1.0 / (i + 1) * base
                    j = J[i + 1:]
                    change = v1 * (Rv[j] - Rv[i])
                    pv = base * (Rv[i] - Rv[j])
                    for k in range(i + 1, n):                                       # past `size`: + p * 0 / (1 + k), p *= 1
                        on = j > k
                        if not on.any():
                            break
                        change = np.where(on, change + pv * Rv[k] / (1 + k), change)
                        pv = np.where(on, pv * (1.0 - Rv[k]), pv)
                        if k >= size and np.all(np.isfinite(pv)):
                            break                                                   # only +-0 is added from here on
                    change = change + (npp[j - 1] * (1.0 - Rv[j]) * Rv[i] / (1.0 - Rv[i]) - npp[j - 1] * Rv[j]) / (j + 1)
                    C[i, i + 1:] = np.where(labels[j] == labels[i], 0.0, change)
            C = np.abs(C)
            return C + C.T                                  # the lower triangle and the diagonal are 0: x + 0.0 is x


# ---- one list, literally -----------------------------------------------------------------------------------------------------------------
def batchFeedForward(net, Xr, labr):             # LambdaRank.java:34-65 on the re-ranked list
    n = len(labr)
    RN.batchFeedForward(net, Xr, labr, 0, n)     # addInput + propagate(i) of every document; its RankNet pair map is not used
    pairMap, targetValue = [], []
    for i in range(n):
        li = np.float32(labr[i])
        pm, tv = [], []
        for j in range(n):
            lj = np.float32(labr[j])
            if li > lj or li < lj:
                pm.append(j)
                tv.append(np.float32(1) if li > lj else np.float32(0))
        pairMap.append(pm)
        targetValue.append(tv)
    return pairMap, targetValue


def computePairWeight(pairMap, labr, changes):   # :91-102
    weight = []
    with np.errstate(all="ignore"):
        for i in range(len(pairMap)):
            row = []
            for j in pairMap[i]:
                sign = 1 if np.float32(labr[i]) > np.float32(labr[j]) else -1
                row.append(np.float32(np.float32(abs(changes[i][j])) * np.float32(sign)))
            weight.append(row)
    return weight


def computeDelta(nr, pairMap, pairWeight, targetValue, current):        # Neuron.java:97-123, the LambdaRank arm
    nr.delta_i = 0.0
    nr.deltas_j = [0.0] * len(pairMap[current])
    for k in range(len(pairMap[current])):
        j = pairMap[current][k]
        weight = pairWeight[current][k]
        pij = float(targetValue[current][k]) - 1.0 / (1.0 + jexp(-(nr.outputs[current] - nr.outputs[j])))
        lambda_ = float(weight) * pij
        nr.delta_i += lambda_
        nr.deltas_j[k] = lambda_ * RN.computeDerivative(nr.outputs[j])
    nr.delta_i *= RN.computeDerivative(nr.outputs[current])


def updateDelta(nr, pairMap, pairWeight, current):                      # Neuron.java:128-150
    nr.delta_i = 0.0
    nr.deltas_j = [0.0] * len(pairMap[current])
    for k in range(len(pairMap[current])):
        j = pairMap[current][k]
        weight = pairWeight[current][k]
        errorSum = 0.0
        for s in nr.outLinks:
            errorSum += s.target.deltas_j[k] * s.weight
            if k == 0:
                nr.delta_i += s.target.delta_i * s.weight
        if k == 0:
            nr.delta_i *= float(weight) * RN.computeDerivative(nr.outputs[current])
        nr.deltas_j[k] = errorSum * float(weight) * RN.computeDerivative(nr.outputs[j])


def batchBackPropagate(net, pairMap, pairWeight, targetValue, learningRate):      # LambdaRank.java:68-83
    L = net.layers
    for i in range(len(pairMap)):
        for nr in L[-1]:
            computeDelta(nr, pairMap, pairWeight, targetValue, i)
        for j in range(len(L) - 2, 0, -1):
            for nr in L[j]:
                updateDelta(nr, pairMap, pairWeight, i)
        for nr in L[-1]:
            RN.updateWeight(nr, pairMap, i, learningRate)
        for j in range(len(L) - 2, 0, -1):
            for nr in L[j]:
                RN.updateWeight(nr, pairMap, i, learningRate)


def _clear(net):
    for lay in net.layers:
        for nr in lay:
            nr.outputs = []


def epoch(net, X, lab, qoff, qid, lr, scorer, hook=None):
    """one pass of learn()'s inner loop (RankNet.java:296-302) with LambdaRank's overrides.  hook(q, net, pairMap, pairWeight, i) is
    called after every step's deltas, for the tests that look at them"""
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        RN.batchFeedForward(net, X, lab, a, b)                        # eval(doc) of every document: the same chain as propagate(i)
        order = rank(list(net.layers[-1][0].outputs))
        _clear(net)
        idx = [a + o for o in order]
        Xr, labr = X[idx], [lab[i] for i in idx]
        pairMap, targetValue = batchFeedForward(net, Xr, labr)
        pairWeight = computePairWeight(pairMap, labr, scorer.swap_change(labr, qid[q]))
        if hook is None:
            batchBackPropagate(net, pairMap, pairWeight, targetValue, lr)
        else:
            L = net.layers
            for i in range(len(pairMap)):
                for nr in L[-1]:
                    computeDelta(nr, pairMap, pairWeight, targetValue, i)
                for j in range(len(L) - 2, 0, -1):
                    for nr in L[j]:
                        updateDelta(nr, pairMap, pairWeight, i)
                hook(q, net, pairMap, pairWeight, i)
                for nr in L[-1]:
                    RN.updateWeight(nr, pairMap, i, lr)
                for j in range(len(L) - 2, 0, -1):
                    for nr in L[j]:
                        RN.updateWeight(nr, pairMap, i, lr)
        _clear(net)


# ---- the vector form --------------------------------------------------------------------------------------------------------------------
def epoch_vector(W, X, lab, qoff, qid, lr, scorer):
    """epoch() on the matrices W (changed in place)"""
    Xd = X.astype(np.float64)
    lab = np.asarray(lab, np.float32)
    nL = len(W)
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        n = b - a
        outs = RN.forward_vector(W, Xd[a:b])
        order = np.argsort(-outs[-1][0], kind="stable")
        outs = [[v[order] for v in lay] for lay in outs]
        Xr, labr = Xd[a:b][order], lab[a:b][order]
        dd = [[(lambda s: s * (1.0 - s))(RN._vlogistic(o)) for o in lay] for lay in outs]
        ones = np.ones((1, n), np.float64)
        SRC = [np.vstack([Xr.T, ones])] + [np.vstack(lay + [ones]) for lay in outs[:-1]]
        C = scorer.swap_abs_vector(labr, qid[q])
        o, ddo = outs[-1][0], dd[-1][0]
        for i in range(n):
            idx = np.nonzero((labr[i] > labr) | (labr[i] < labr))[0]
            P = len(idx)
            up = labr[i] > labr[idx]
            wt = (C[i, idx].astype(np.float32) * np.where(up, np.float32(1), np.float32(-1)).astype(np.float32)).astype(np.float32)
            wd = wt.astype(np.float64)
            pij = np.where(up, np.float32(1), np.float32(0)).astype(np.float64) - 1.0 / (1.0 + RN.vjexp(-(o[i] - o[idx])))
            lam = wd * pij
            di = [None] * nL
            dj = [None] * nL
            di[-1] = [RN._chain(lam) * ddo[i]]
            dj[-1] = [lam * ddo[idx]]
            for l in range(nL - 2, -1, -1):
                di[l], dj[l] = [], []
                for h in range(W[l].shape[0]):
                    es = np.zeros(P, np.float64)
                    d = 0.0
                    for t in range(W[l + 1].shape[0]):
                        es = es + dj[l + 1][t] * W[l + 1][t, h]
                        if P:
                            d += di[l + 1][t] * W[l + 1][t, h]
                    if P:
                        d *= float(wd[0]) * dd[l][h][i]
                    di[l].append(d)
                    dj[l].append((es * wd) * dd[l][h][idx])
            for l in range(nL):
                S = SRC[l]
                for t in range(W[l].shape[0]):
                    terms = dj[l][t][None, :] * S[:, idx]
                    sum_j = np.cumsum(np.concatenate([np.zeros((S.shape[0], 1), np.float64), terms], axis=1), axis=1)[:, -1]
                    W[l][t, :] += lr * (di[l][t] * S[:, i] - sum_j)


def learn(train, valid=None, metric="NDCG", k=10, n_iteration=3, lr=0.00005, hidden=(10,), seed=None, start=None, err_max=16.0,
          ideal=None, rel_doc_count=None, valid_rel_doc_count=CR.SAME, vector=True):
    """RankNet.learn() :290-334, which LambdaRank inherits; arguments and result as ranknet_restatement.learn's.  Raises OverflowError
    naming the epoch after which a weight is not finite (rlhip refuses there; the Java goes on)."""
    X, lab, qoff, qid = train
    F = X.shape[1]
    net = RN.build(F, hidden)
    if start is not None:
        RN.set_weights(net, start)
    else:
        RN.draw_weights(net, seed)
    W = RN.matrices(net)
    sc = CR.LiteralScorer(metric, k, err_max, ideal, rel_doc_count, valid_rel_doc_count)
    scorer = Scorer(sc, metric, k, rel_doc_count)
    totalPairs = RN.total_pairs(lab, qoff)
    bestModelOnValidation = []
    bestScoreOnValidationData = 0.0
    trace = []
    epoch_weights = [RN.flat_weights(W).copy()]              # the start, then the weights after every epoch (before any restore)
    for i in range(1, n_iteration + 1):
        with np.errstate(all="ignore"):
            if vector:
                epoch_vector(W, X, lab, qoff, qid, lr, scorer)
            else:
                epoch(net, X, lab, qoff, qid, lr, scorer)
                W = RN.matrices(net)
        if not np.all(np.isfinite(RN.flat_weights(W))):
            raise OverflowError("epoch %d" % i)
        epoch_weights.append(RN.flat_weights(W).copy())
        ev = RN.scores(W, X)
        tr = sc.score([float(v) for v in ev], lab, qoff, qid)
        mis = RN.misordered_pairs(ev, lab, qoff)             # LambdaRank.estimateLoss :105-120: the same count
        va, saved = 0.0, 0
        if valid is not None:
            Xv, lv, qv, qidv = valid
            va = sc.score([float(v) for v in RN.scores(W, Xv)], lv, qv, qidv, valid=True)
            if va > bestScoreOnValidationData:
                bestScoreOnValidationData = va
                bestModelOnValidation = [m.copy() for m in W]
                saved = 1
        trace.append((i, saved, mis, totalPairs, tr, va))
    if valid is not None:
        try:
            W = [bestModelOnValidation[l].copy() for l in range(len(W))]
        except Exception as ex:                              # noqa: BLE001
            raise RestoreError("Error in NeuralNetwork.restoreBestModelOnValidation(): %s" % ex)
    out = dict(trace=trace, weight=RN.flat_weights(W), matrices=W, train_scores=RN.scores(W, X), epoch_weights=epoch_weights)
    out["train"] = sc.score([float(v) for v in out["train_scores"]], lab, qoff, qid)
    if valid is not None:
        Xv, lv, qv, qidv = valid
        out["valid"] = sc.score([float(v) for v in RN.scores(W, Xv)], lv, qv, qidv, valid=True)
    return out


def model_text(flat, features, hidden, n_iteration):
    """RankNet.model() with LambdaRank's name()"""
    text = RN.model_text(flat, features, hidden, n_iteration)
    assert text.startswith("## RankNet\n")
    return "## LambdaRank\n" + text[len("## RankNet\n"):]


def quirk_data():
    """NDCG@2, F = 1, one hidden neuron, weights that keep the output rising with x, x falling inside each list: the given order is the
    ranked one.  List 0, labels (1, 1, 1, 0, 2): the first pair of step 2 is (2, 3), both positions >= k -- and then every pair of that
    step is past the cut-off, because a pair below it would have come first.  List 1, labels (0.5, 0, 2, 1, 0, 0): the first pair of
    step 0 is (0, 1), labels 0.5 and 0 with the same gain, so weight_0 is 0 while the pairs (0, 2) and (0, 3) weigh something."""
    lab = np.array([1, 1, 1, 0, 2, 0.5, 0, 2, 1, 0, 0], np.float32)
    X = np.array([[2.0], [1.5], [1.0], [0.5], [0.0], [2.5], [2.0], [1.5], [1.0], [0.5], [0.0]], np.float32)
    return (X, lab, np.array([0, 5, 11], np.int32), ["a", "b"]), [0.8, 0.1, 0.9, -0.2]
