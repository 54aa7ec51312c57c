"""NumPy restatement of the replay behind rl_adopt_model_text (ranklib_amd/csrc/rl_resume.inc) -- TEST INFRASTRUCTURE ONLY.

What a trainer holds after it has replayed the trees of a model on its own rows:

    walk      Split.eval: value <= threshold goes left (Split.java:115-125), on the raw float32 rows
    chain     modelScores[i] += learningRate * output (LambdaMART.java:203-210, :230-234): an f64 chain from 0.0 in tree order whose
              product is the DOUBLE product of the float learning rate and the float output
    metrics   after every tree the float mean over the lists of the scorer's value (LambdaMART.java:469-483), through the scorers of
              tests/np_restatement.py
    best/stop the strict > over the validation values in round order (:237-243) and the test of :248 at the last replayed round

Trees are dicts of flat pre-order arrays (feature ids, -1 = leaf; threshold; left; right; output) as every tree of the tests is.
"""
import numpy as np

import np_restatement as R

F32 = np.float32
BEST_ROUND_INIT = 2147483647 - 2          # LambdaMART.bestModelOnValidation  LambdaMART.java:50


def walk(tree, X, col_of):
    """the leaf output (float32) every row of X reaches"""
    X = np.asarray(X, F32)
    node = np.zeros(X.shape[0], np.int64)
    feat = np.asarray(tree["feature"])
    thr = np.asarray(tree["threshold"], F32)
    left, right = np.asarray(tree["left"]), np.asarray(tree["right"])
    while True:
        f = feat[node]
        at_split = f != -1
        if not at_split.any():
            break
        rows = np.nonzero(at_split)[0]
        cols = np.array([col_of[int(v)] for v in f[rows]], np.int64)
        with np.errstate(invalid="ignore"):
            goes_left = X[rows, cols] <= thr[node[rows]]                  # NaN compares false: right, like the Java
        node[rows] = np.where(goes_left, left[node[rows]], right[node[rows]])
    return np.asarray(tree["output"], F32)[node]


def chain_step(scores, lr, out):
    """s += (double)lr * (double)out, the product rounded once, the sum once"""
    return scores + np.float64(F32(lr)) * out.astype(np.float64)


def float_mean(scorer, scores, labels, qoff, qids):
    """float s = 0; for every list: s += score(list ranked by the scores); s / Q   (np_restatement.LambdaMART._metric)"""
    s = F32(0)
    Q = len(qoff) - 1
    for q in range(Q):
        cur, end = int(qoff[q]), int(qoff[q + 1])
        order = R.stable_desc([float(v) for v in scores[cur:end]])
        s = F32(float(s) + scorer.score([float(labels[cur + i]) for i in order], qids[q]))
    return F32(s / F32(Q))


def replay(trees, lr, scorer, X, labels, qoff, feature_ids=None, valid=None, early_stop=100):
    """-> dict(stages [T0][N] f64 scores after every tree, metrics [T0] float32, and with valid = (X, labels, qoff): vstages, vmetrics;
    best_round, best_score, stop)"""
    X = np.asarray(X, F32)
    col_of = {int(f): c for c, f in enumerate(feature_ids if feature_ids is not None else range(1, X.shape[1] + 1))}
    qids = ["q%d" % q for q in range(len(qoff) - 1)]
    scores = np.zeros(X.shape[0], np.float64)
    out = dict(stages=[], metrics=[], vstages=[], vmetrics=[], best_round=BEST_ROUND_INIT, best_score=0.0, stop=False)
    if valid is not None:
        Xv, lv, qv = valid
        vscores = np.zeros(len(lv), np.float64)
        vqids = ["v%d" % q for q in range(len(qv) - 1)]
    for r, tree in enumerate(trees):
        scores = chain_step(scores, lr, walk(tree, X, col_of))
        out["stages"].append(scores)
        out["metrics"].append(float_mean(scorer, scores, labels, qoff, qids))
        if valid is not None:
            vscores = chain_step(vscores, lr, walk(tree, Xv, col_of))
            out["vstages"].append(vscores)
            vm = float_mean(scorer, vscores, lv, qv, vqids)
            out["vmetrics"].append(vm)
            if float(vm) > out["best_score"]:                              # :237-243
                out["best_score"], out["best_round"] = float(vm), r
        out["stop"] = (r - out["best_round"]) > early_stop                 # :248
    return out
