"""-m gpu: DART training (rl_set_dart, k_dart_drop) against tests/dart_restatement.py, computed once per case.  Every comparison
is == on bit views.  Shapes: 12 trees of 6 leaves on 8 features; about 300 documents in lists of 5 .. 15 with a validation set, and once
1 061 documents (k_dart_drop's second block, its last tile partial).  Every case runs with RLHIP_DART_CHUNK 1, 2 and unset: a trainer reads its
knobs when it is created, so the same process serves all three.
"""
import numpy as np
import pytest

import dart_restatement as DR
from ranklib_amd import _native as N
from ranklib_amd import synth

pytestmark = pytest.mark.gpu

T, LEAVES, FEATS, SEED = 12, 6, 8, 7
CASES = {
    "ndcg10": dict(n=300, metric="NDCG", k=10, ranker="LAMBDAMART", rate=0.5, max_drop=0),
    "mart": dict(n=300, metric="NDCG", k=10, ranker="MART", rate=0.5, max_drop=0),
    "map": dict(n=300, metric="MAP", k=0, ranker="LAMBDAMART", rate=0.5, max_drop=0),
    "few_drops": dict(n=300, metric="NDCG", k=10, ranker="LAMBDAMART", rate=0.12, max_drop=0),
    "max_drop_1": dict(n=300, metric="NDCG", k=10, ranker="LAMBDAMART", rate=0.5, max_drop=1),
    "two_blocks": dict(n=1061, metric="NDCG", k=10, ranker="LAMBDAMART", rate=0.5, max_drop=0),
}
_REF = {}


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _data(c):
    return synth.make_dataset(c["n"], FEATS, "ns", seed_offset=11), synth.make_dataset(120, FEATS, "ns", seed_offset=12)


def _ref(name):
    if name not in _REF:
        c = CASES[name]
        (X, lab, qoff), valid = _data(c)
        _REF[name] = DR.train(X, lab, qoff, T, LEAVES, 0.1, c["rate"], c["max_drop"], SEED, metric=c["metric"], k=c["k"], ranker=c["ranker"], valid=valid)
    return _REF[name]


def _trainer(c, rate=None, dart=True, **kw):
    (X, lab, qoff), valid = _data(c)
    g = N.Trainer(**dict(dict(n_trees=T, n_leaves=LEAVES, metric=c["metric"], metric_k=c["k"], ranker=c["ranker"]), **kw))
    g.set_train(X, lab, qoff)
    g.set_validation(*valid)
    if dart:
        g.set_dart(c["rate"] if rate is None else rate, c["max_drop"], SEED)
    g.init()
    return g


@pytest.mark.parametrize("chunk", [None, 1, 2], ids=["chunk_default", "chunk_1", "chunk_2"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_dart_run_is_the_restatement_bit_for_bit(name, chunk, monkeypatch):
    c, ref = CASES[name], _ref(name)
    ks = [len(d) for d in ref["dropped"]]
    assert ks[0] == 0
    if name == "few_drops":
        assert 0 in ks[1:] and max(ks) > 0, ks                                  # plain rounds and DART rounds in one run
    elif c["max_drop"] == 1:
        assert max(ks) == 1, ks
    else:
        assert max(ks) >= 5, ks                                                 # chunks of one and two trees turn over several times, the last chunk of two is partial
    if chunk is not None:
        monkeypatch.setenv("RLHIP_DART_CHUNK", str(chunk))
    g = _trainer(c)
    for m in range(T):
        _, tm, vm, stop = g.boost_round(want_tree=False)
        assert not stop
        assert list(g.dart_dropped(m)) == ref["dropped"][m], (name, m)
        assert np.array_equal(_u32(g.tree_weights()), _u32(ref["weights"][m])), (name, "weights after round %d" % m)
        assert (_u32(tm), _u32(vm)) == (_u32(ref["metrics"][m][0]), _u32(ref["metrics"][m][1])), (name, "metrics of round %d" % m)
    for m in range(T):
        t, (feat, thr, _, _, out) = g.get_tree(m).trimmed(), ref["trees"][m]
        assert list(t["feature"]) == feat and np.array_equal(_u32(t["threshold"]), _u32(thr)) and np.array_equal(_u32(t["output"]), _u32(out)), (name, "tree %d" % m)
    assert np.array_equal(_u64(g.array("SCORE")), _u64(ref["scores"])), name
    assert np.array_equal(_u64(g.array("VALID_SCORE")), _u64(ref["vscores"])), name
    g.close()


def test_rate_zero_is_the_plain_run():
    c = CASES["ndcg10"]
    runs = []
    for dart in (False, True):
        g = _trainer(c, rate=0.0, dart=dart)
        ms = [g.boost_round(want_tree=False)[1:3] for _ in range(T)]
        runs.append((ms, g.array("SCORE"), g.array("VALID_SCORE"), g.tree_weights(), g.finish(), g.model_text()))
        g.close()
    a, b = runs
    assert a[0] == b[0] and a[4] == b[4] and a[5] == b[5]
    for i in (1, 2):
        assert np.array_equal(_u64(a[i]), _u64(b[i]))
    assert np.array_equal(_u32(a[3]), _u32(np.full(len(a[3]), 0.1, np.float32))) and np.array_equal(_u32(a[3]), _u32(b[3]))


def test_the_weights_travel_through_the_model_text():
    c = CASES["ndcg10"]
    g = _trainer(c)
    for _ in range(T):
        g.boost_round(want_tree=False)
    g.finish()
    assert g.num_trees() == T                                     # no roll-back, whatever the best validation round was
    X = _data(c)[0][0]
    mine, text = g.predict(X), g.model_text()
    assert len(set(_u32(g.tree_weights()).tolist())) > 1
    g.close()
    rows = np.concatenate([np.zeros((len(X), 1), np.float32), X], axis=1)       # (column f holds feature id f, column 0 unused)
    assert np.array_equal(_u32(mine), _u32(N.Model(text).predict_rows(rows)))


def test_what_dart_refuses(monkeypatch):
    c = CASES["ndcg10"]
    L = N.lib()
    assert L.rl_set_dart(None, 0.5, 0, 0) == -1 and b"null trainer" in L.rl_last_error()
    g = N.Trainer(n_trees=T, n_leaves=LEAVES)
    for bad in (float("nan"), -0.1, 1.5):
        with pytest.raises(N.RankLibError, match="rate_drop"):
            g.set_dart(bad)
    g.close()
    g = _trainer(c)
    with pytest.raises(N.RankLibError, match="before rl_init"):
        g.set_dart(0.5)
    g.boost_round(want_tree=False)
    text = g.model_text()
    g.close()
    g = _trainer(c)
    for call in (g.adopt_model_text, g.refit_model_text):
        with pytest.raises(N.RankLibError, match="a DART trainer cannot"):
            call(text)
    g.close()
    for kw in (dict(flags=N.RL_FLAG_SERIAL_CHAIN), dict(n_leaves=2000)):
        with pytest.raises(N.RankLibError, match="not with RL_FLAG_SERIAL_CHAIN, RLHIP_SCORE_STREAM=0 or more than 1024 leaves"):
            _trainer(c, **kw)
    with pytest.raises(N.RankLibError, match=r"needs \d+ bytes of device memory"):
        _trainer(c, n_trees=2 ** 31 - 1)
    g = N.Trainer(n_trees=T, n_leaves=LEAVES)
    g.set_train(*_data(c)[0])
    g.dist_init_callback(0, 1, lambda arr, op: None, lambda src: src)
    g.set_dart(0.5)
    with pytest.raises(N.RankLibError, match="sharded"):
        g.init()
    g.close()
    monkeypatch.setenv("RLHIP_SCORE_STREAM", "0")
    with pytest.raises(N.RankLibError, match="RLHIP_SCORE_STREAM=0"):
        _trainer(c)
