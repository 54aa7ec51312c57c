"""Literal restatement of ListNet training in plain Python -- TEST INFRASTRUCTURE ONLY.

Synapse's draw (Synapse.java:29), ListNet.init / learn (ListNet.java:84-140), Neuron.computeOutput(i) (Neuron.java:78-87),
ListNeuron.computeDelta / updateWeight (ListNeuron.java:18-49) and RankNet.saveBestModelOnValidation / restoreBestModelOnValidation
(RankNet.java:191-223) with its exception, in the Java's loop order.  Python floats are Java doubles, numpy.float32 the Java floats, exp is
np_restatement.jexp (fdlibm's e_exp).  No network objects: ListNet's network is F inputs and a bias into one output neuron, so a Synapse
is an entry of `weight` (inLinks order = wire() order: inputs 0 .. F - 1, the bias last).

The one thing that is not the Java's is the seed: its Random is `new Random()`, static and shared; here every init() starts a fresh
java.util.Random(seed), as ranklib_amd.learning.ListNet does.
"""
import numpy as np

import ca_restatement as CR
import net_restatement as NR
from np_restatement import jexp
from ranklib_amd.learning import java_double_str


class JavaRandom(CR.JavaRandom):
    def nextFloat(self):               # next(24) / ((float)(1 << 24))
        return np.float32(self.next(24)) / np.float32(1 << 24)


class RestoreError(Exception):
    """RankLibError.create("Error in NeuralNetwork.restoreBestModelOnValidation(): ", ex) (RankNet.java:220-222)"""


def draw_weights(seed, n):
    """n Synapses made one after another: weight = (random.nextInt(2) == 0 ? 1 : -1) * random.nextFloat() / 10, an int times a float,
    divided by 10 as a FLOAT, stored in a double"""
    rnd = JavaRandom(seed)
    out = []
    for _ in range(n):
        sign = 1 if rnd.nextInt(2) == 0 else -1
        out.append(float(np.float32(np.float32(np.float32(sign) * rnd.nextFloat()) / np.float32(10))))
    return out


def feed_forward(X, weight, a, b):
    """ListNet.feedForward (:40-48) of the list [a, b): addInput + propagate per document; returns the output neuron's outputs"""
    F = X.shape[1]
    outputs = []
    for i in range(a, b):
        wsum = 0.0
        for k in range(F):
            wsum += float(X[i, k]) * weight[k]          # getSource().getOutput(i) * getWeight(): a float widened times a double
        wsum += float(np.float32(1.0)) * weight[F]      # the bias neuron's output is 1.0f
        outputs.append(1.0 / (1.0 + jexp(-wsum)))
    return outputs


def back_propagate(X, lab, weight, a, b, outputs, lr):
    """ListNeuron.computeDelta, then updateWeight for every inLink in order (weights changed in place)"""
    F, n = X.shape[1], b - a
    sumLabelExp = sumScoreExp = 0.0
    for i in range(n):
        sumLabelExp += jexp(float(np.float32(lab[a + i])))
        sumScoreExp += jexp(outputs[i])
    d1 = [jexp(float(np.float32(lab[a + i]))) / sumLabelExp for i in range(n)]
    d2 = [jexp(outputs[i]) / sumScoreExp for i in range(n)]
    for k in range(F + 1):
        dw = 0.0
        for l in range(n):
            dw += (d1[l] - d2[l]) * (float(X[a + l, k]) if k < F else float(np.float32(1.0)))
        dw *= lr
        weight[k] += dw


def epoch(X, lab, qoff, weight, lr):
    """one pass of learn()'s inner loop (:106-110)"""
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        back_propagate(X, lab, weight, a, b, feed_forward(X, weight, a, b), lr)


def epoch_vector(X, lab, qoff, weight, lr):
    """the same pass with the document loops as numpy element-wise f64 operations and np.cumsum for the serial sums (cumsum adds in index
    order, one rounding per element); the tests hold it equal to epoch() and use it where the literal loops would take minutes"""
    F = X.shape[1]
    Xd = X.astype(np.float64)
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        wsum = np.zeros(b - a, np.float64)
        for k in range(F):
            wsum = wsum + Xd[a:b, k] * weight[k]
        wsum = wsum + 1.0 * weight[F]
        out = 1.0 / (1.0 + NR.vexp(-wsum))
        el, es = NR.vexp(lab[a:b].astype(np.float32).astype(np.float64)), NR.vexp(out)
        d = el / np.cumsum(el)[-1] - es / np.cumsum(es)[-1]
        for k in range(F + 1):
            terms = d * Xd[a:b, k] if k < F else d * 1.0
            dw = float(np.cumsum(np.concatenate([[0.0], terms]))[-1])
            dw *= lr
            weight[k] += dw


def scores(X, weight):
    """RankNet.eval of every row (the forward pass, one output neuron)"""
    F = X.shape[1]
    wsum = np.zeros(X.shape[0], np.float64)
    Xd = X.astype(np.float64)
    for k in range(F):
        wsum = wsum + Xd[:, k] * weight[k]
    wsum = wsum + 1.0 * weight[F]
    return 1.0 / (1.0 + NR.vexp(-wsum))


def learn(train, valid=None, metric="NDCG", k=10, n_iteration=3, lr=0.00001, seed=None, start=None, err_max=16.0, ideal=None,
          rel_doc_count=None, valid_rel_doc_count=CR.SAME, vector=False):
    """train / valid: (X [N, F] float32, column j = input j, labels, qoff, qids).  start: the initial weights (else drawn from seed).
    Returns the trace [(epoch, saved, train score, valid score)], the final weights (the restored best with a validation set) and both final
    metric values, not rounded.  Raises RestoreError where the Java's restoreBestModelOnValidation throws."""
    X, lab, qoff, qid = train
    F = X.shape[1]
    weight = list(start) if start is not None else draw_weights(seed, F + 1)
    assert len(weight) == F + 1
    sc = CR.LiteralScorer(metric, k, err_max, ideal, rel_doc_count, valid_rel_doc_count)
    step = epoch_vector if vector else epoch
    bestModelOnValidation = []                               # init(): an empty list per layer (:91-95); one layer carries weights
    bestScoreOnValidationData = 0.0
    trace = []
    for i in range(1, n_iteration + 1):
        with np.errstate(all="ignore"):                      # a run that overflows says so through OverflowError below
            step(X, lab, qoff, weight, lr)
        if not all(np.isfinite(weight)):
            raise OverflowError("epoch %d" % i)              # rlhip refuses here; the Java goes on with NaN
        tr = sc.score([float(v) for v in scores(X, weight)], lab, qoff, qid)
        va, saved = 0.0, 0
        if valid is not None:
            Xv, lv, qv, qidv = valid
            va = sc.score([float(v) for v in scores(Xv, weight)], lv, qv, qidv, valid=True)
            if va > bestScoreOnValidationData:               # :117-120
                bestScoreOnValidationData = va
                bestModelOnValidation = list(weight)         # saveBestModelOnValidation: l.clear(); l.add(every outLink's weight)
                saved = 1
        trace.append((i, saved, tr, va))
    if valid is not None:                                    # restoreBestModelOnValidation :206-223
        try:
            c = 0
            for j in range(F + 1):                           # layer 0's neurons in order, one outLink each
                weight[j] = bestModelOnValidation[c]
                c += 1
        except Exception as ex:                              # noqa: BLE001
            raise RestoreError("Error in NeuralNetwork.restoreBestModelOnValidation(): %s" % ex)
    out = dict(trace=trace, weight=weight, train_scores=scores(X, weight))
    out["train"] = sc.score([float(v) for v in out["train_scores"]], lab, qoff, qid)
    if valid is not None:
        Xv, lv, qv, qidv = valid
        out["valid"] = sc.score([float(v) for v in scores(Xv, weight)], lv, qv, qidv, valid=True)
    return out


def model_text(weight, features, n_iteration):
    """ListNet.model() (:157-174) over RankNet.toString (:356-372) for the network without a hidden layer: one line per input neuron and
    one for the bias, each with its single outLink's weight"""
    F = len(features)
    out = "## ListNet\n## Epochs = %d\n## No. of features = %d\n" % (n_iteration, F)
    out += "".join(str(f) + ("" if i == F - 1 else " ") for i, f in enumerate(features)) + "\n0\n"
    for j in range(F + 1):
        out += "0 %d %s\n" % (j, java_double_str(weight[j]))
    return out
