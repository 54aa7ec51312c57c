"""-m gpu: the XE-NDCG objective (rl_set_objective, k_lambda_xe) against tests/xe_restatement.py, == on bit views only.  The kernel
through rl_debug_xe_lambdas: about 300 documents in lists of 1, 2 and 5 .. 15 at the default tile and at 64 (several blocks, the last partial), a
150-document list at tile 64 (the long path: two chunk boundaries, a last chunk of 22), lists that fill a tile exactly, a score 800 above its list
in a tile and in the long list (the guard, exp underflowing to 0).  The trainer: 8 trees of 6 leaves, every round's tree, lambdas, weights, scores
and metrics; it reads RLHIP_XE_TILE when it is created.  RL_FLAG_FAST_LEAF is not restated: np_restatement's leaf rule sits inside its round()."""
import numpy as np
import pytest

import np_restatement as R
import xe_restatement as XR
from ranklib_amd import _native as N
from ranklib_amd import synth

pytestmark = pytest.mark.gpu

T, LEAVES, FEATS = 8, 6, 8
LENS = dict(mixed=[1, 2] * 3 + [int(v) for v in np.random.default_rng(4).integers(5, 16, 29)] + [1], long=[10, 150, 7], fill=[64, 30, 34, 5], guard=[12, 150, 9])
CASES = {"ndcg10": dict(n=300, metric="NDCG", k=10), "map": dict(n=300, metric="MAP", k=0), "n1100": dict(n=1100, metric="NDCG", k=10)}
_REF = {}


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,tile,rnd,seed", [
    ("mixed", 0, 0, 1), ("mixed", 64, 0, 1), ("mixed", 0, 3, 2), ("mixed", 64, 3, 2), ("long", 64, 0, 1), ("long", 64, 3, 2), ("fill", 64, 0, 1), ("guard", 64, 3, 2)])
def test_the_kernel_is_the_restatement_bit_for_bit(name, tile, rnd, seed):
    rng = np.random.default_rng(5)
    qoff = np.concatenate([[0], np.cumsum(LENS[name])]).astype(np.int32)
    s, lab = rng.normal(size=qoff[-1]), rng.integers(0, 5, qoff[-1]).astype(np.float32)
    assert name != "mixed" or 250 <= len(s) <= 400
    if name == "guard":
        s[[3, 12 + 70]] += 800.0
    lam, w = N.debug_xe_lambdas(s, lab, qoff, seed=seed, round=rnd, tile=tile)
    rl, rw = XR.lambdas(s, lab, list(qoff), seed, rnd)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(w)) and np.any(lam != 0)
    assert np.array_equal(_u64(lam), _u64(rl)), (name, np.flatnonzero(_u64(lam) != _u64(rl))[:8])
    assert np.array_equal(_u64(w), _u64(rw)), name


def _data(c):
    return synth.make_dataset(c["n"], FEATS, "ns", seed_offset=11), synth.make_dataset(120, FEATS, "ns", seed_offset=12)


def _ref(name):
    """the restatement's rounds: [(tree, lambda, w, scores, valid scores, train metric, valid metric)]"""
    if name not in _REF:
        c = CASES[name]
        (X, lab, qoff), valid = _data(c)
        m = XR.XeLambdaMART(X, lab, qoff, n_trees=T, n_leaves=LEAVES, k=c["k"], metric=c["metric"])
        m.xe_seed = 9
        m.set_validation(*valid)
        m.init()
        _REF[name] = []
        for _ in range(T):
            root, tm, vm, _ = m.round()
            _REF[name].append((R.flatten_tree(root), list(m.pseudo), list(m.weights), list(m.model_scores), list(m.valid_scores), tm, vm))
    return _REF[name]


def _trainer(c, objective="xendcg", **kw):
    (X, lab, qoff), valid = _data(c)
    g = N.Trainer(**dict(dict(n_trees=T, n_leaves=LEAVES, metric=c["metric"], metric_k=c["k"]), **kw))
    g.set_train(X, lab, qoff)
    g.set_validation(*valid)
    if objective is not None:
        g.set_objective(objective, 9)
    g.init()
    return g


@pytest.mark.parametrize("tile", [None, 64], ids=["tile_default", "tile_64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_run_is_the_restatement_bit_for_bit(name, tile, monkeypatch):
    if tile is not None:
        monkeypatch.setenv("RLHIP_XE_TILE", str(tile))
    g = _trainer(CASES[name])
    for m, (tree, lam, w, sc, vsc, tm, vm) in enumerate(_ref(name)):
        t, gtm, gvm, _ = g.boost_round()
        t, (feat, thr, _, _, out) = t.trimmed(), tree
        assert list(t["feature"]) == feat and np.array_equal(_u32(t["threshold"]), _u32(thr)) and np.array_equal(_u32(t["output"]), _u32(out)), (name, "tree %d" % m)
        assert len(feat) > 1 and np.array_equal(_u64(g.array("LAMBDA")), _u64(lam)) and np.array_equal(_u64(g.array("WEIGHT")), _u64(w)), (name, "lambdas of round %d" % m)
        assert np.array_equal(_u64(g.array("SCORE")), _u64(sc)) and np.array_equal(_u64(g.array("VALID_SCORE")), _u64(vsc)), (name, "scores after round %d" % m)
        assert (_u32(gtm), _u32(gvm)) == (_u32(tm), _u32(vm)), (name, "metrics of round %d" % m)
    g.close()


def test_the_pairwise_objective_set_explicitly_is_the_plain_run():
    runs = []
    for objective in (None, "lambda", "xendcg"):
        g = _trainer(CASES["ndcg10"], objective=objective)
        ms = [g.boost_round(want_tree=False)[1:3] for _ in range(T)]
        runs.append((ms, g.model_text(), _u64(g.array("SCORE")).tolist()))
        g.close()
    assert runs[0] == runs[1] and runs[0][1] != runs[2][1]


def test_what_the_objective_refuses():
    (X, lab, qoff), _ = _data(CASES["ndcg10"])
    L = N.lib()
    assert L.rl_set_objective(None, 1, 0) == -1 and b"null trainer" in L.rl_last_error()
    for kw, objective, match in ((dict(), 2, "unknown objective 2"), (dict(ranker="MART"), "xendcg", "MART fits residuals")):
        g = N.Trainer(n_trees=T, n_leaves=LEAVES, **kw)
        with pytest.raises(N.RankLibError, match=match):
            g.set_objective(objective)
        g.close()
    g = _trainer(CASES["ndcg10"])
    with pytest.raises(N.RankLibError, match="before rl_init"):
        g.set_objective("lambda")
    g.close()
    lab31 = lab.copy()
    lab31[17] = 31.0
    for labels, sharded, match in ((lab, True, "sharded"), (lab31, False, "relevance label 31 of document 17 is above 30")):
        g = N.Trainer(n_trees=T, n_leaves=LEAVES)
        g.set_train(X, labels, qoff)
        if sharded:
            g.dist_init_callback(0, 1, lambda arr, op: None, lambda src: src)
        g.set_objective("xendcg")
        with pytest.raises(N.RankLibError, match=match):
            g.init()
        g.close()
