"""The handle core the four linear rankers share (rl_linear.inc, _native._LinearTrainer), on the smallest data that reaches every shared
path: the state errors of each class name its own C API and no other ranker's, learn() runs once and needs a training set, a validation
set of another width is refused, close() twice is harmless, scores() has no validation value when no validation set was given; and the
one scoring kernel behind ca_predict / rb_predict / lr_predict gives exactly the f64 sums of the three eval() forms."""
import numpy as np
import pytest

from ranklib_amd import _native as N

pytestmark = pytest.mark.gpu

PREFIXES = ("rl_ca_", "rl_ada_", "rl_rb_", "rl_lr_")
TRAINERS = {
    "rl_ca_": lambda: N.CoorAscentTrainer(n_restart=1, n_max_iteration=1),
    "rl_ada_": lambda: N.AdaRankTrainer(n_iteration=2),
    "rl_rb_": lambda: N.RankBoostTrainer(n_iteration=2),
    "rl_lr_": lambda: N.LinearRegTrainer(),
}

# four training lists of 1, 2, 3 and 17 documents, two feature columns, labels 0 .. 2; one validation list of 3 documents
_rng = np.random.default_rng(20)
QOFF = np.array([0, 1, 3, 6, 23], np.int32)
X = _rng.integers(0, 5, (23, 2)).astype(np.float32) * np.float32(0.37)
LAB = (np.arange(23) % 3).astype(np.float32)
XV = _rng.integers(0, 5, (3, 2)).astype(np.float32) * np.float32(0.37)
LABV = np.array([0, 2, 1], np.float32)
QOFFV = np.array([0, 3], np.int32)


def _state_error(call):
    with pytest.raises(N.RankLibError) as e:
        call()
    msg = str(e.value)
    assert "status -3" in msg
    return msg


def _names_only(msg, prefix):
    assert prefix in msg and not any(p in msg for p in PREFIXES if p != prefix), msg


@pytest.mark.parametrize("prefix", PREFIXES)
def test_handle_states(prefix):
    t = TRAINERS[prefix]()
    _state_error(t.learn)                                          # no training set yet
    t.set_train(X, LAB, QOFF)
    with pytest.raises(N.RankLibError):
        t.set_validation(np.zeros((3, 3), np.float32), LABV, QOFFV)      # another column count
    t.set_validation(XV, LABV, QOFFV)
    t.learn()
    ts, vs = t.scores()
    assert np.isfinite(ts) and vs is not None and np.isfinite(vs)
    for call in (lambda: t.set_train(X, LAB, QOFF), lambda: t.set_validation(XV, LABV, QOFFV),
                 lambda: t.set_external_judgments(False, None, np.ones(4, np.int32)), t.learn):
        _names_only(_state_error(call), prefix)
    t.close()
    t.close()

    t = TRAINERS[prefix]()                                         # no validation set: scores() has none to give
    t.set_train(X, LAB, QOFF)
    t.learn()
    ts, vs = t.scores()
    assert np.isfinite(ts) and vs is None
    t.close()


def test_predict_sums_are_exact():
    """rows[:, f] holds feature id f (column 0 unused).  The ids repeat one feature and name one at and one beyond the row width (both
    read 0); Linear Regression's also hold a -1 (reads 0).  Expected: the eval() sums in index order, in NumPy f64."""
    rows = np.concatenate([np.zeros((23, 1), np.float32), X], axis=1)                   # width 3
    ids = np.array([1, 2, 1, 3, 7], np.int32)
    w = np.array([0.3, -1.7, 0.11, 5.0, 2.5], np.float64)
    thr = np.array([0.37, 0.5, 0.0, -1.0, 0.2], np.float64)

    def column(c):
        return rows[:, c].astype(np.float64) if 0 <= c < rows.shape[1] else np.zeros(len(rows), np.float64)

    s = np.zeros(len(rows), np.float64)
    for t in range(len(ids)):
        s = s + w[t] * column(ids[t])
    assert N.ca_predict(ids, w, rows).tobytes() == s.tobytes()

    s = np.zeros(len(rows), np.float64)
    for t in range(len(ids)):
        s = s + w[t] * (column(ids[t]) > thr[t]).astype(np.float64)                     # a threshold of -1.0 fires on a column that reads 0
    assert N.rb_predict(ids, thr, w, rows).tobytes() == s.tobytes()

    ids_lr = np.array([1, 2, 1, 3, -1], np.int32)
    w_lr = np.array([0.3, -1.7, 0.11, 5.0, 2.5, 0.625, -0.4], np.float64)              # more weights than features: the last is the bias
    s = np.full(len(rows), w_lr[-1], np.float64)
    for t in range(len(ids_lr)):
        s = s + w_lr[t] * column(ids_lr[t])
    assert N.lr_predict(ids_lr, w_lr, rows).tobytes() == s.tobytes()
