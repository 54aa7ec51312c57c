"""Inputs the linear-ranker tests share (Coordinate Ascent, AdaRank, RankBoost, Linear Regression): data with a chosen label set, the
external judgments -qrel would load (idealGains / relDocCount maps keyed by qid), and the two ways they are handed over -- per list to a
rlhip trainer (rl_*_set_external_judgments: NaN = qid not in the file, count 0 = qid not in the file), by map to a restatement.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np
import pytest

import np_restatement as R

WRAPPED = (0, 1, 2, 31, 32, 33)          # (1 << rel) - 1 on Java ints: 31 -> 2147483647, 32 -> 0, 33 -> 1
FRACTIONAL = (0, 0.5, 1, 1.5, 2.99)      # label > 0 (MAP, P, RR) and (int) label (NDCG, DCG, ERR) disagree on 0.5
LENGTH_CLASSES = (3, 16, 17, 384, 385, 1500, 5001, 9, 200, 2)     # every class of k_ca_trials / k_ada_weak, one list of the longest


def data(rng, lengths, F, labels=(0, 1, 2), levels=4, qid=None, prefix="q"):
    """(X, labels, qoff, qid): feature values on a small grid with exact zeros (ties), labels drawn from `labels`"""
    qoff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    X = (rng.integers(0, levels, (qoff[-1], F)).astype(np.float32) * np.float32(0.37)).astype(np.float32)
    X[rng.random(X.shape) < 0.1] = 0.0
    lab = rng.choice(np.array(labels, np.float32), int(qoff[-1])).astype(np.float32)
    return X, lab, qoff, list(qid) if qid is not None else ["%s%d" % (prefix, i) for i in range(len(lengths))]


def _by_qid(sets):
    out = {}
    for s in sets:
        if s is None:
            continue
        _, lab, qoff, qid = s
        for q, name in enumerate(qid):
            out.setdefault(name, []).append(lab[qoff[q]:qoff[q + 1]])
    return out


def ideal_map(sets, k, rng, factors=(0.5, 1.0, 2.0), missing=1.0 / 3):
    """qid -> external ideal DCG: the largest own ideal DCG@k among the qid's lists times a factor (so 0.5 is below some list's DCG, 2.0
    above every one); a share `missing` of the qids gets no entry"""
    out = {}
    for name, labs in _by_qid(sets).items():
        f = factors[int(rng.integers(len(factors)))]
        if rng.random() < missing:
            continue
        own = max(R.ideal_dcg([int(v) for v in l], min(k, len(l)) if k > 0 else len(l)) for l in labs)
        out[name] = own * f if own > 0 else 1.5
    return out


def count_map(sets, rng, missing=0.2):
    """qid -> external relevant-document count: 0, the largest own count among the qid's lists, or a larger one; some qids get no entry"""
    out = {}
    for name, labs in _by_qid(sets).items():
        kind = int(rng.integers(3))
        if rng.random() < missing:
            continue
        own = max(int(np.sum(l > 0)) for l in labs)
        out[name] = (0, own, own + 1 + int(rng.integers(4)))[kind]
    return out


def restrict(m, s):
    """the entries of m for the qids of set s"""
    return {q: v for q, v in m.items() if q in set(s[3])}


def per_list(m, qid, kind):
    """the map as rl_*_set_external_judgments takes it"""
    if kind == "ideal":
        return np.array([m.get(q, np.nan) for q in qid], np.float64)
    return np.array([m.get(q, 0) for q in qid], np.int32)


def judgments(metric, m, train, valid, where):
    """(per-list arrays for feed(), keyword arguments for a restatement's learn()) for map m given to the training set only ("train"), the
    validation set only ("valid") or both ("both").  The ideal-DCG cache is one for both sets (NDCGScorer.idealGains), so the restatement
    gets the union; the counts belong to the set they were given to, the other set keeps its own counts."""
    mt = restrict(m, train) if where in ("train", "both") else None
    mv = restrict(m, valid) if where in ("valid", "both") and valid is not None else None
    if metric == "NDCG":
        arrays = dict(ideal_tr=None if mt is None else per_list(mt, train[3], "ideal"),
                      ideal_va=None if mv is None else per_list(mv, valid[3], "ideal"))
        return arrays, dict(ideal=dict(mt or {}, **(mv or {})))
    arrays = dict(rdc_tr=None if mt is None else per_list(mt, train[3], "count"), rdc_va=None if mv is None else per_list(mv, valid[3], "count"))
    return arrays, dict(rel_doc_count=mt, valid_rel_doc_count=mv)


def feed(t, train, valid=None, ideal_tr=None, ideal_va=None, rdc_tr=None, rdc_va=None):
    """set_train / set_validation with qkeys shared across the sets by qid, then the external judgments"""
    X, lab, qoff, qid = train
    keys = {}
    t.set_train(X, lab, qoff, qkey=np.array([keys.setdefault(q, len(keys)) for q in qid], np.int32))
    if valid is not None:
        Xv, lv, qv, qidv = valid
        t.set_validation(Xv, lv, qv, qkey=np.array([keys.setdefault(q, len(keys)) for q in qidv], np.int32))
    if ideal_tr is not None or rdc_tr is not None:
        t.set_external_judgments(False, ideal_tr, rdc_tr)
    if ideal_va is not None or rdc_va is not None:
        t.set_external_judgments(True, ideal_va, rdc_va)
    return t


REFUSAL_COUNTS = np.array([9, 0, 9, 9], np.int32)
REFUSAL_MAP = {"q0": 9, "q2": 9, "q3": 9}                # the same as a restatement takes them (lists q0 .. q3; q1 counts 0)


def forwarded_refusals(new_trainer, tr, error):
    """rl_{ca,ada,rb,lr}_set_external_judgments are one function on the handles' shared ranking context (lin_set_external_judgments,
    rl_linear.inc): RL_ERR_STATE (-3) before set_train, for a validation set that was never given and after learn(); RL_ERR_INVALID (-1)
    for a negative count; a later set_train discards the judgments (ca_store).
    tr holds four lists q0 .. q3.  Returns (the trainer that learned with REFUSAL_COUNTS, the one whose judgments were discarded)."""
    t = new_trainer()
    with pytest.raises(error) as e:
        t.set_external_judgments(False, None, np.ones(4, np.int32))
    assert "status -3" in str(e.value)
    feed(t, tr)
    with pytest.raises(error) as e:
        t.set_external_judgments(False, None, np.array([1, 2, -1, 0], np.int32))
    assert "status -1" in str(e.value)
    with pytest.raises(error) as e:
        t.set_external_judgments(True, None, np.ones(4, np.int32))
    assert "status -3" in str(e.value)
    t.set_external_judgments(False, None, REFUSAL_COUNTS)
    t.learn()
    with pytest.raises(error) as e:
        t.set_external_judgments(False, None, np.ones(4, np.int32))
    assert "status -3" in str(e.value)
    t2 = new_trainer()
    feed(t2, tr, rdc_tr=REFUSAL_COUNTS)
    feed(t2, tr)
    t2.learn()
    return t, t2


def shared_sets(rng, F=5, labels=(0, 1, 2), n_train=45, n_valid=15, hi=31):
    """45 training lists of 1-30 documents with repeated qids (q0 .. q36) and 15 validation lists q30 .. q44: q30 .. q36 name lists of both"""
    tr = data(rng, rng.integers(1, hi, n_train), F, labels, qid=["q%d" % (i % 37) for i in range(n_train)])
    va = data(rng, rng.integers(1, hi, n_valid), F, labels, qid=["q%d" % (i + 30) for i in range(n_valid)])
    return tr, va


def write_letor(path, X, lab, qoff, qid0=0):
    """a LETOR file with qids qid0, qid0 + 1, ..."""
    with open(path, "w") as f:
        for q in range(len(qoff) - 1):
            for i in range(qoff[q], qoff[q + 1]):
                feats = " ".join("%d:%s" % (j + 1, repr(float(X[i, j]))) for j in range(X.shape[1]))
                f.write("%d qid:%d %s # d%d\n" % (int(lab[i]), qid0 + q, feats, i))


def write_qrel(path, rng, sizes, skip=3):
    """TREC-style judgments for qids 0 .. len(sizes) - 1 (sizes: their lists' lengths) but each `skip`-th: more documents than the list
    holds, labels 0 .. 4, so both the ideal DCG and the relevant-document count differ from the list's own"""
    with open(path, "w") as f:
        for q in range(len(sizes)):
            if q % skip == skip - 1:
                continue
            for d in range(int(sizes[q]) + 6):
                f.write("%d 0 doc%d %d\n" % (q, d, int(rng.integers(0, 5))))
