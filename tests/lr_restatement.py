"""A literal restatement of learning/LinearRegRank.java learn() (:44-100), eval (:103-109), toString / model (:117-131), loadFromString
(:134-170) and solve (:188-239) for the Linear Regression tests.  Nothing is "fixed":

nVar is the largest feature id F of the training lists, so the regressors are features 1 .. F-1 and a constant, feature F is not fitted and
weight[F-1] is the constant's.  xTx[j][k] += x_j * t_k with t_k the DOUBLE x_k (or 1f for the last column): a float widened times a double,
exact in f64.  xTy[j] += x_j * label is a FLOAT product (np.float32 * np.float32), widened and added.  Every cell is its own running f64
sum over the documents in (list, document) order.  The ridge term is added only if lambda != 0.0.  solve() is Gaussian elimination without
pivoting in the Java's loop order.  eval() starts from weight[last] and pairs weight[i] with features[i]: with the default feature list
1 .. F the constant's weight is used twice.

accumulate_literal() is the Java's three nested loops; accumulate() adds np.outer(t, t) per document, which keeps every cell's own order
(a cell receives one addend per document, in document order, and the addend t_j * t_k is the same exact product).  The tests hold the two
equal.  xTx comes out bitwise symmetric (the same exact addends arrive in the same order on both sides); both functions ASSERT it.
"""
import numpy as np

import ca_restatement as CR
from ranklib_amd.learning import java_double_str


class NotReproduced(Exception):
    """a pivot that is 0 or not finite, or a weight that is not finite: rlhip refuses (the Java goes on with NaN)"""

    def __init__(self, column, what):
        super().__init__("column %d: %s" % (column, what))
        self.column = column


def _assert_symmetric(xtx):
    assert np.array_equal(xtx.view(np.int64), xtx.T.copy().view(np.int64)), "xTx is not bitwise symmetric"


def accumulate_literal(X, lab, nVar):
    """:58-83 as written: Python floats are Java doubles, np.float32 the Java floats"""
    xTx = [[0.0] * nVar for _ in range(nVar)]
    xTy = [0.0] * nVar
    for i in range(X.shape[0]):
        label = np.float32(lab[i])
        fv = [np.float32(X[i, j]) for j in range(nVar - 1)]          # point.getFeatureValue(j + 1)
        xTy[nVar - 1] += float(label)
        for j in range(nVar - 1):
            xTy[j] += float(np.float32(fv[j] * label))              # float * float, rounded to float, then widened
            for k in range(nVar):
                t = float(fv[k]) if k < nVar - 1 else float(np.float32(1))
                xTx[j][k] += float(fv[j]) * t                        # float widened * double
        for k in range(nVar - 1):
            xTx[nVar - 1][k] += float(fv[k])
        xTx[nVar - 1][nVar - 1] += float(np.float32(1))
    xtx, xty = np.array(xTx, np.float64).reshape(nVar, nVar), np.array(xTy, np.float64)
    _assert_symmetric(xtx)
    return xtx, xty


def accumulate(X, lab, nVar):
    """the same sums, one np.outer per document"""
    X = np.asarray(X, np.float32)
    lab = np.asarray(lab, np.float32)
    xtx, xty = np.zeros((nVar, nVar), np.float64), np.zeros(nVar, np.float64)
    t = np.ones(nVar, np.float64)
    y = np.zeros(nVar, np.float32)
    for i in range(X.shape[0]):
        t[:nVar - 1] = X[i, :nVar - 1]
        xtx += np.outer(t, t)
        y[:nVar - 1] = X[i, :nVar - 1] * lab[i]                      # np.float32 products
        y[nVar - 1] = lab[i]
        xty += y.astype(np.float64)
    _assert_symmetric(xtx)
    return xtx, xty


def solve(A, B):
    """:188-239.  The k loop of a row update is element-wise (a multiply and a subtraction per element, each rounded), so numpy rows keep it;
    the back-substitution is a serial chain and stays a loop."""
    a = np.array(A, np.float64)
    b = [float(v) for v in B]
    n = len(b)
    with np.errstate(all="ignore"):
        for j in range(n - 1):
            pivot = float(a[j, j])
            if pivot == 0.0 or not np.isfinite(pivot):
                raise NotReproduced(j, "pivot %r" % pivot)
            for i in range(j + 1, n):
                multiplier = float(a[i, j]) / pivot
                a[i, j + 1:] = a[i, j + 1:] - a[j, j + 1:] * multiplier
                b[i] -= b[j] * multiplier
        if float(a[n - 1, n - 1]) == 0.0 or not np.isfinite(a[n - 1, n - 1]):
            raise NotReproduced(n - 1, "pivot %r" % float(a[n - 1, n - 1]))
        x = [0.0] * n
        x[n - 1] = b[n - 1] / float(a[n - 1, n - 1])
        for i in range(n - 2, -1, -1):
            val = b[i]
            row = a[i]
            for j in range(i + 1, n):
                val -= float(row[j]) * x[j]
            x[i] = val / float(row[i])
    for i, v in enumerate(x):
        if not np.isfinite(v):
            raise NotReproduced(i, "weight %r" % v)
    return x


def eval_scores(X, features, weight, missing_zero=True):
    """:103-109 for every row of X (column f - 1 = feature id f; an id beyond the columns reads 0, as under -missingZero)"""
    if len(features) > len(weight):
        raise IndexError("features.length > weight.length: ArrayIndexOutOfBoundsException")
    s = np.full(X.shape[0], weight[len(weight) - 1], np.float64)
    for i, f in enumerate(features):
        col = X[:, f - 1].astype(np.float64) if 1 <= f <= X.shape[1] else np.zeros(X.shape[0])
        s = s + weight[i] * col
    return s


def learn(train, valid=None, metric="NDCG", k=10, lam=1E-10, features=None, err_max=16.0, ideal=None, rel_doc_count=None,
          valid_rel_doc_count=CR.SAME):
    """train / valid: (X [N, F] float32 with column f - 1 = feature f, labels, qoff, qids).  Returns xtx / xty (before the ridge term), the
    weights, both sets' document scores and the two metric values (not rounded)."""
    X, lab, qoff, qid = train
    nVar = X.shape[1]
    features = list(range(1, nVar + 1)) if features is None else list(features)
    xtx, xty = accumulate(X, lab, nVar)
    a = xtx.copy()
    if lam != 0.0:
        for i in range(nVar):
            a[i, i] += lam
    weight = solve(a, xty)
    sc = (CR.VectorScorer if X.shape[0] > 1500 else CR.LiteralScorer)(metric, k, err_max, ideal, rel_doc_count, valid_rel_doc_count)
    out = dict(xtx=xtx, xty=xty, weight=weight, features=features)
    out["train_scores"] = eval_scores(X, features, weight)
    out["train"] = sc.score(_cache(sc, out["train_scores"]), lab, qoff, qid)
    if valid is not None:
        Xv, lv, qv, qidv = valid
        out["valid_scores"] = eval_scores(Xv, features, weight)
        out["valid"] = sc.score(_cache(sc, out["valid_scores"]), lv, qv, qidv, valid=True)
    return out


def _cache(sc, scores):
    return scores if isinstance(sc, CR.VectorScorer) else [float(v) for v in scores]


def to_string(weight, features):
    """:117-123"""
    out = "0:" + java_double_str(weight[0]) + " "
    for i in range(len(features)):
        out += str(features[i]) + ":" + java_double_str(weight[i]) + ("" if i == len(weight) - 1 else " ")
    return out


def model_text(weight, features, lam):
    return "## Linear Regression\n## Lambda = " + java_double_str(lam) + "\n" + to_string(weight, features)


def load(text):
    """:134-170: (features, weight) -- weight has len(features) + 1 entries, the key 0 value last"""
    line = [c.strip() for c in text.split("\n") if c.strip() and not c.strip().startswith("##")][0]
    pairs = [tok.split(":") for tok in line.split(" ") if tok.strip()]
    weight = [0.0] * len(pairs)
    features = [0] * (len(pairs) - 1)
    idx = 0
    for key, val in pairs:
        if int(key) > 0:
            features[idx] = int(key)
            weight[idx] = float(val)
            idx += 1
        else:
            weight[len(weight) - 1] = float(val)
    return features, weight
