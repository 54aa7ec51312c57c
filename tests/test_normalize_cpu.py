"""The normaliser's restatement (tests/normalize_restatement.py) against ranklib_amd/normalizer.py list by list, the C entry's refusals and
exports, and the -kcv flow's count of normalisations per DataPoint.  No GPU: test_gpu_normalize.py holds the device equal to the restatement."""
import os
import re

import numpy as np
import pytest

import normalize_restatement as NR
from ranklib_amd import _native as N
from ranklib_amd import normalizer as NM
from ranklib_amd.evaluator import Evaluator
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, RankList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_lists(seed, F=6):
    """lists in the style of test_host_mirror.py's normaliser test: a constant column, one without a positive value, NaN cells, n = 1.  No
    negative zero (numpy's minimum / maximum do not order the two zeros; the restatement follows the Java there)"""
    rng = np.random.RandomState(seed)
    lens = [1, 2] + [int(rng.randint(1, 30)) for _ in range(10)]
    rows = []
    for n in lens:
        R = (rng.randn(n, F + 1) * rng.choice([1e-3, 1.0, 1e4])).astype(np.float32)
        R[:, 0] = np.nan
        R[:, 2] = 7.5
        R[:, 3] = -np.abs(R[:, 3]) - np.float32(1e-6)
        R[rng.rand(n) < 0.2, 4] = np.nan
        rows.append(R)
    X = np.concatenate(rows)
    qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert not np.any(NR.bits(X) == 0x80000000)
    return X, qoff


def as_lists(X, qoff, row_len=None):
    pts = [DataPoint.from_parsed(1.0, "q", "", X[d, :(X.shape[1] if row_len is None else row_len[d])].copy()) for d in range(len(X))]
    return [RankList(pts[qoff[q]:qoff[q + 1]]) for q in range(len(qoff) - 1)], pts


@pytest.mark.parametrize("fids", [None, [1, 2, 3, 4, 6, 3], [5, 2, 2, 1]], ids=["all", "dup", "unordered"])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_restatement_equals_the_normalizer_list_by_list(kind, fids, monkeypatch):
    monkeypatch.setattr(NM.Normalizer, "batch", False)
    X, qoff = random_lists(11)
    lists, pts = as_lists(X, qoff)
    nm = NM.create(kind)
    for rl in lists:
        nm.normalize(rl, fids)
    cols = sorted(set(fids)) if fids else list(range(1, X.shape[1]))
    want = NR.normalize_lists(X, qoff, cols, kind)
    for d, dp in enumerate(pts):
        assert np.array_equal(NR.bits(dp.fVals), NR.bits(want[d])), (kind, d)
    untouched = [c for c in range(X.shape[1]) if c not in cols]
    assert np.array_equal(NR.bits(want[:, untouched]), NR.bits(X[:, untouched]))
    one = qoff[:-1][np.diff(qoff) == 1]
    if kind != "linear":                      # a list of one document: zscore leaves it alone (std is NaN); sum sets x / |x|
        assert kind == "sum" or np.array_equal(NR.bits(want[one]), NR.bits(X[one]))


@pytest.mark.parametrize("kind", NR.KINDS)
def test_restatement_on_ragged_rows_with_a_feature_subset(kind, monkeypatch):
    monkeypatch.setattr(NM.Normalizer, "batch", False)
    X, qoff = random_lists(12)
    rng = np.random.RandomState(5)
    row_len = rng.randint(4, X.shape[1] + 1, len(X)).astype(np.int32)     # every row holds features 1 .. 3 at least
    lists, pts = as_lists(X, qoff, row_len)
    nm = NM.create(kind)
    for rl in lists:
        nm.normalize(rl, [3, 1])
    want = NR.normalize_lists(X, qoff, [3, 1], kind, row_len=row_len)
    for d, dp in enumerate(pts):
        assert np.array_equal(NR.bits(dp.fVals), NR.bits(want[d, :row_len[d]])), (kind, d)


@pytest.mark.parametrize("kind", NR.KINDS)
def test_times_is_that_many_applications(kind):
    X, qoff = random_lists(13)
    cols = [1, 2, 3, 4, 5, 6]
    step = X
    for t in range(1, 6):
        step = NR.normalize_lists(step, qoff, cols, kind)
        assert np.array_equal(NR.bits(NR.normalize_lists(X, qoff, cols, kind, times=t)), NR.bits(step)), (kind, t)


def test_java_min_and_max_order_the_zeros():
    f = np.float32
    pz, nz = np.array([0.0], f), np.array([-0.0], f)
    assert np.signbit(NR.java_min(pz, nz))[0] and np.signbit(NR.java_min(nz, pz))[0]
    assert not np.signbit(NR.java_max(pz, nz))[0] and not np.signbit(NR.java_max(nz, pz))[0]
    assert NR.java_min(np.array([NR.F32_MAX], f), np.array([np.inf], f))[0] == NR.F32_MAX
    assert NR.java_max(np.array([NR.F32_MIN], f), np.array([-1.0], f))[0] == NR.F32_MIN
    # both zeros in one column: min is -0.0, max stays Float.MIN_VALUE, every cell becomes (v - -0.0) / (MIN_VALUE - -0.0) = +0.0
    X = np.array([[np.nan, 0.0], [np.nan, -0.0], [np.nan, 0.0]], f)
    got = NR.normalize_lists(X, [0, 3], [1], "linear")
    assert np.array_equal(NR.bits(got[:, 1]), np.zeros(3, np.uint32))


# ---- the ABI entry ----------------------------------------------------------------------------------------------------------------------
def _lib():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return N.lib()


def test_library_exports_rl_normalize_lists_and_the_abi_version_stays():
    L = _lib()
    assert hasattr(L, "rl_normalize_lists") and hasattr(L, "rl_debug_normalize_times")
    assert L.rl_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    declared = sorted(set(re.findall(r"\b(rl_[a-z0-9_]+)\s*\(", hdr)))
    assert "rl_normalize_lists" in declared and "rl_debug_normalize_times" in declared and sorted(N.ABI_SYMBOLS) == declared
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bRL_NORM_([A-Z]+) = (\d+)", hdr)}
    assert got == N.RL_NORM_KIND == dict(sum=0, zscore=1, linear=2)


def _call(X, qoff, cols, kind=0, n_docs=None, stride=None, row_len=None, n_lists=None, n_cols=None, times=1):
    L = _lib()
    X = None if X is None else np.ascontiguousarray(X, np.float32)
    qoff = None if qoff is None else np.ascontiguousarray(qoff, np.int32)
    cols = None if cols is None else np.ascontiguousarray(cols, np.int32)
    row_len = None if row_len is None else np.ascontiguousarray(row_len, np.int32)
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    before = None if X is None else X.copy()
    rc = L.rl_normalize_lists(0, kind, p(X), 3 if n_docs is None else n_docs, 4 if stride is None else stride, p(row_len), p(qoff),
                              2 if n_lists is None else n_lists, p(cols), (0 if cols is None else len(cols)) if n_cols is None else n_cols, times)
    if rc != 0 and X is not None:
        assert np.array_equal(NR.bits(X), NR.bits(before)), "a refused call must not touch X"
    return rc, L.rl_last_error().decode()


def test_refusals_come_before_any_device_call(gpu_available):
    """every one of these is RL_ERR_INVALID (-1) with its own message, on a machine with a GPU and on one without: a call that got as far
    as the device would answer RL_ERR_NO_DEVICE (-5) here"""
    X, qoff, cols = np.arange(12, dtype=np.float32).reshape(3, 4), [0, 2, 3], [1, 3]
    for kw in (dict(X=None), dict(qoff=None), dict(cols=None, n_cols=2)):
        a = dict(X=X, qoff=qoff, cols=cols)
        a.update(kw)
        rc, msg = _call(a.pop("X"), a.pop("qoff"), a.pop("cols"), **a)
        assert rc == -1 and "null argument" in msg, (kw, rc, msg)
    for kw in (dict(n_docs=0), dict(n_lists=0), dict(n_cols=0), dict(times=0), dict(times=-3), dict(n_docs=-1)):
        rc, msg = _call(X, qoff, cols, **kw)
        assert rc == -1 and "must be >= 1" in msg, (kw, rc, msg)
    for s in (1, 0, -4):
        rc, msg = _call(X, qoff, cols, stride=s)
        assert rc == -1 and "stride" in msg, (s, rc, msg)
    for bad in ([1, 2, 3], [0, 2, 2], [0, 2, 4], [0, 3, 2], [0, 1, 2], [0, 0, 3]):
        rc, msg = _call(X, bad, cols)
        assert rc == -1 and "qoff" in msg, (bad, rc, msg)
    for k in (-1, 3, 100):
        rc, msg = _call(X, qoff, cols, kind=k)
        assert rc == -1 and "unknown normaliser" in msg, (k, rc, msg)
    for bad in ([0], [1, 4], [-2, 1], [2, 0]):
        rc, msg = _call(X, qoff, bad)
        assert rc == -1 and "is not a column of a row" in msg, (bad, rc, msg)
    rc, msg = _call(X, qoff, [1, 3, 1])
    assert rc == -1 and "duplicate feature id 1" in msg
    for bad in ([4, 0, 4], [4, 5, 4], [-1, 4, 4]):
        rc, msg = _call(X, qoff, cols, row_len=bad)
        assert rc == -1 and "row_len of row" in msg, (bad, rc, msg)
    rc, msg = _call(X, qoff, [2, 3, 1], row_len=[4, 4, 2])
    assert rc == -1 and "row 2 does not hold feature 2" in msg, msg          # the first requested feature, in the caller's order, it lacks
    rc, msg = _call(X, qoff, [1, 3], row_len=[4, 3, 1])
    assert rc == -1 and "row 1 does not hold feature 3" in msg, msg
    # a valid call reaches the device: without one there is no CPU fallback
    rc, msg = _call(X, qoff, [1, 2], row_len=[4, 3, 3], times=2)
    assert rc == (0 if gpu_available else -5), (rc, msg)
    if not gpu_available:
        assert "no CPU fallback" in msg or "gfx950" in msg
        with pytest.raises(N.RankLibError, match="status -5"):
            N.normalize_lists(X.copy(), qoff, [1, 2], "sum")


def test_native_normalize_lists_checks_its_arrays():
    _lib()
    X = np.zeros((3, 4), np.float32)
    with pytest.raises(N.RankLibError, match="kind must be one of"):
        N.normalize_lists(X, [0, 3], [1], "l2")
    for bad in (X.astype(np.float64), X[:, ::2], X.T, np.zeros(4, np.float32), [[0.0, 1.0]]):
        with pytest.raises(N.RankLibError, match="writable C-contiguous float32"):
            N.normalize_lists(bad, [0, 3], [1], "sum")
    ro = X.copy()
    ro.setflags(write=False)
    with pytest.raises(N.RankLibError, match="writable C-contiguous float32"):
        N.normalize_lists(ro, [0, 3], [1], "sum")
    with pytest.raises(N.RankLibError, match="row_len"):
        N.normalize_lists(X, [0, 3], [1], "sum", row_len=[4, 4])
    with pytest.raises(N.RankLibError, match="qoff must end at n_docs"):
        N.normalize_lists(X, [0, 2], [1], "sum", chunk_bytes=16)          # bad offsets reach the C call whole, whatever the budget


def test_without_a_device_normalize_all_is_the_list_by_list_path(gpu_available, monkeypatch):
    if gpu_available:
        pytest.skip("GPU present")
    X, qoff = random_lists(14)
    calls = []
    monkeypatch.setattr(N, "normalize_lists", lambda *a, **kw: calls.append(a))
    for kind in NR.KINDS:
        lists, pts = as_lists(X, qoff)
        nm = NM.create(kind)
        assert nm.normalizeBatch(lists) is False
        nm.normalizeAll(lists)
        want = NR.normalize_lists(X, qoff, list(range(1, X.shape[1])), kind)
        assert all(np.array_equal(NR.bits(dp.fVals), NR.bits(want[d])) for d, dp in enumerate(pts))
    assert not calls


# ---- -kcv: every list is normalised nFold * nFold times -----------------------------------------------------------------------------------
class CountingNormalizer(NM.Normalizer):
    def __init__(self):
        self.count = {}

    def name(self):
        return "count"

    def normalize(self, rl, fids=None):
        for dp in rl.rl:
            self.count[id(dp)] = self.count.get(id(dp), 0) + 1


@pytest.mark.parametrize("tvs", [-1.0, 0.75], ids=["plain", "tvs"])
@pytest.mark.parametrize("n_lists", [1, 2, 4, 7, 11])
@pytest.mark.parametrize("nFold", [2, 3, 5])
def test_kcv_normalises_every_data_point_nfold_squared_times(nFold, n_lists, tvs, monkeypatch):
    """the loop of Evaluator.evaluate_kcv (eval/Evaluator.java:816-822) as written, list by list: all folds once per fold, the folds sharing
    their DataPoints.  With a list count that is no multiple of nFold, and with fewer lists than folds"""
    rng = np.random.RandomState(nFold * 100 + n_lists)
    samples = [RankList([DataPoint.from_parsed(float(i % 2), "q%d" % q, "", np.ones(3, np.float32)) for i in range(int(rng.randint(1, 5)))])
               for q in range(n_lists)]
    trainingData, validationData, testData = FeatureManager.prepareCV(samples, nFold, tvs)
    per_list = {id(rl.rl[0]): 0 for rl in samples}
    for group in (trainingData, validationData, testData):
        for fold in group:
            for rl in fold:
                per_list[id(rl.rl[0])] += 1
    assert set(per_list.values()) == {nFold}                    # train, validation or test of every fold: exactly nFold fold lists
    nm = CountingNormalizer()
    monkeypatch.setattr(Evaluator, "nml", nm)
    monkeypatch.setattr(NM.Normalizer, "batch", False)
    ev = Evaluator.__new__(Evaluator)
    for _ in range(nFold):                                      # the loop of evaluate_kcv
        for group in (trainingData, validationData, testData):
            for fold in group:
                ev.normalizeLists(fold, [1, 2])
    assert len(nm.count) == sum(rl.size() for rl in samples)
    assert set(nm.count.values()) == {nFold * nFold}


def test_evaluate_kcv_runs_that_loop_when_batch_is_off(tmp_path, monkeypatch):
    """the same count through evaluate_kcv itself, up to the first training call"""
    path = str(tmp_path / "d.txt")
    with open(path, "w") as f:
        for q in range(7):
            for i in range(3):
                f.write("%d qid:%d 1:%g 2:%g\n" % (i % 2, q, 0.5 * i + q, 1.0 + i))
    nm = CountingNormalizer()
    monkeypatch.setattr(Evaluator, "nml", nm)
    monkeypatch.setattr(Evaluator, "normalize", True)
    monkeypatch.setattr(NM.Normalizer, "batch", False)

    class Stop(Exception):
        pass

    def stop(*a, **kw):
        raise Stop()
    monkeypatch.setattr(Evaluator, "_train", stop)
    ev = Evaluator.__new__(Evaluator)
    with pytest.raises(Stop):
        ev.evaluate_kcv(path, None, 3)
    assert len(nm.count) == 21 and set(nm.count.values()) == {9}
