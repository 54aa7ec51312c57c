"""rl_normalize_lists on the GPU against the flat restatement (tests/normalize_restatement.py, which test_normalize_cpu.py holds equal to
ranklib_amd/normalizer.py): every kind, the list lengths and column counts around a wavefront, columns built to break a normaliser, repeated
application, chunking; and Normalizer.normalizeAll / the evaluator's flows, batch against list by list.  No tolerance anywhere: every
comparison is on the uint32 bits of the whole matrix, so the cells that must not change are checked with the ones that must."""
import functools
import glob
import os

import numpy as np
import pytest

import normalize_restatement as NR
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd import learning
from ranklib_amd import normalizer as NM
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, RankList

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETOR = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "letor", "*.train.txt")))
LENGTHS = [1, 2, 3, 63, 64, 65, 300]


def same(got, want, tag, X=None):
    bad = np.argwhere(NR.bits(got) != NR.bits(want))
    assert not bad.size, (tag, len(bad), [(int(d), int(c), float(got[d, c]), float(want[d, c]), None if X is None else float(X[d, c]))
                                         for d, c in bad[:4]])


def gpu(X, qoff, cols, kind, **kw):
    G = X.copy()
    N.normalize_lists(G, qoff, cols, kind, **kw)
    return G


@functools.lru_cache(maxsize=None)
def shaped_file(n_cols, scattered):
    X, qoff, cols = NR.make_file(LENGTHS, n_cols, n_cols + (9 if scattered else 1), seed=n_cols * 2 + scattered, scattered=bool(scattered))
    for a in (X, qoff, cols):
        a.setflags(write=False)
    return X, qoff, cols


@pytest.mark.parametrize("scattered", [0, 1], ids=["dense", "scattered"])
@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 136])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_every_kind_list_length_and_column_count(kind, n_cols, scattered):
    """lists of 1, 2, 3, 63, 64, 65 and 300 documents in one file; the column counts put a wavefront inside one list, on a list's edge and
    across two lists; once every column of the row but 0, once an unordered subset of a wider row"""
    X, qoff, cols = shaped_file(n_cols, scattered)
    same(gpu(X, qoff, cols, kind), NR.normalize_lists(X, qoff, cols, kind), (kind, n_cols, scattered), X)


@pytest.mark.parametrize("n", [1, 2, 3, 65])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_columns_built_to_break_a_normaliser(kind, n):
    """one column per pattern: constant, zeros of either sign, no positive value, NaN cells and payloads, infinities, f32 subnormals, values
    near FLT_MAX, a quotient that is subnormal"""
    rng = np.random.RandomState(n)
    adv = NR.adversarial_columns(n, rng)
    names = sorted(adv)
    X = np.full((n, len(names) + 2), np.nan, np.float32)
    for j, name in enumerate(names):
        X[:, j + 1] = adv[name]
    X[:, -1] = 3.25                                   # not requested
    qoff, cols = np.array([0, n], np.int32), np.arange(1, len(names) + 1, dtype=np.int32)
    got, want = gpu(X, qoff, cols, kind), NR.normalize_lists(X, qoff, cols, kind)
    for j, name in enumerate(names):
        assert np.array_equal(NR.bits(got[:, j + 1]), NR.bits(want[:, j + 1])), (kind, n, name, X[:, j + 1], got[:, j + 1], want[:, j + 1])
    same(got, want, (kind, n))
    if kind != "linear":                              # nothing is set in a column of NaNs: the payloads survive
        j = names.index("nan payloads") + 1
        assert np.array_equal(NR.bits(got[:, j]), NR.bits(X[:, j]))


@functools.lru_cache(maxsize=None)
def random_file():
    """64 lists x 136 columns = 8704 (list, column) pairs of random lengths and scales: as many distinct operands of zscore's square root
    and of each division"""
    rng = np.random.RandomState(77)
    lengths = rng.randint(3, 24, 64)
    X, qoff, cols = NR.make_file(lengths, 136, 137, seed=78, adversarial=False)
    X *= (10.0 ** rng.uniform(-6, 6, (len(lengths), 137))).astype(np.float32).repeat(lengths, axis=0)
    X[:, 0] = np.nan
    for a in (X, qoff, cols):
        a.setflags(write=False)
    return X, qoff, cols


@pytest.mark.parametrize("kind", NR.KINDS)
def test_thousands_of_random_list_column_pairs(kind):
    X, qoff, cols = random_file()
    want = NR.normalize_lists(X, qoff, cols, kind)
    if kind == "zscore":                              # the operands are distinct: nothing degenerate hides a wrong rounding
        first = want[qoff[:-1], 1:]
        assert len(np.unique(first)) > 8000
    same(gpu(X, qoff, cols, kind), want, kind, X)


@pytest.mark.parametrize("times", [1, 2, 9, 25])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_times_is_that_many_applications(kind, times):
    X, qoff, cols = shaped_file(65, 1)
    X, qoff = X[:qoff[5]], qoff[:6]                   # lists of 1 .. 64 documents
    same(gpu(X, qoff, cols, kind, times=times), NR.normalize_lists(X, qoff, cols, kind, times=times), (kind, times), X)


@pytest.mark.parametrize("n_lists, n_cols", [(37, 5), (103, 5), (51, 1), (257, 1)])
def test_a_list_count_that_fills_the_last_block_partly(n_lists, n_cols):
    rng = np.random.RandomState(n_lists)
    X, qoff, cols = NR.make_file(rng.randint(1, 6, n_lists), n_cols, n_cols + 3, seed=n_lists, adversarial=False, scattered=True)
    for kind in NR.KINDS:
        same(gpu(X, qoff, cols, kind), NR.normalize_lists(X, qoff, cols, kind), (kind, n_lists, n_cols), X)


def test_rows_that_end_early_on_columns_that_were_not_requested():
    X, qoff, _ = NR.make_file([3, 17, 1, 40], 5, 12, seed=4, adversarial=False)
    cols = np.array([4, 1, 5], np.int32)
    row_len = np.random.RandomState(6).randint(6, 13, len(X)).astype(np.int32)
    for d in range(len(X)):
        X[d, row_len[d]:] = np.float32(-123.5)        # not part of the row: must come back as it went
    for kind in NR.KINDS:
        same(gpu(X, qoff, cols, kind, row_len=row_len), NR.normalize_lists(X, qoff, cols, kind, row_len=row_len), kind, X)
    row_len[20] = 5
    with pytest.raises(N.RankLibError, match="row 20 does not hold feature 5"):
        gpu(X, qoff, cols, "sum", row_len=row_len)


@pytest.mark.parametrize("kind", NR.KINDS)
def test_chunks_of_whole_lists_equal_one_call(kind):
    X, qoff, cols = shaped_file(63, 0)
    one = X.copy()
    assert N.normalize_lists(one, qoff, cols, kind, times=2) == 1
    same(one, NR.normalize_lists(X, qoff, cols, kind, times=2), kind, X)
    row = X.shape[1] * 4
    for budget, calls in ((1, len(LENGTHS)), (row * 64, 5), (row * 70, 4), (row * 140, 3)):
        # 64 rows: [1, 2, 3] [63] [64] [65] [300]; 70 rows: [1, 2, 3, 63] [64] [65] [300]; 140 rows: [1, 2, 3, 63, 64] [65] [300]
        G = X.copy()
        assert N.normalize_lists(G, qoff, cols, kind, times=2, chunk_bytes=budget) == calls, budget
        same(G, one, (kind, budget))


# ---- Normalizer.normalizeAll, batch against list by list ----------------------------------------------------------------------------------
@pytest.fixture
def spy(monkeypatch):
    """counts the rl_normalize_lists calls that reach the library"""
    L, calls = N.lib(), []
    real = L.rl_normalize_lists
    monkeypatch.setattr(L, "rl_normalize_lists", lambda *a: (calls.append(a), real(*a))[1])
    return calls


def read(path, native):
    saved = FeatureManager.native
    FeatureManager.native = native
    try:
        return FeatureManager.readInput(path)
    finally:
        FeatureManager.native = saved


def all_bits(lists):
    return [NR.bits(dp.fVals).copy() for rl in lists for dp in rl.rl]


@pytest.mark.parametrize("fids", [None, [3, 1, 4], [2, 4, 2, 1, 4]], ids=["all", "subset", "duplicates"])
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("path", LETOR, ids=[os.path.basename(p)[:-10] for p in LETOR])
def test_normalize_all_batch_equals_list_by_list(path, native, fids, spy, monkeypatch):
    for kind in NR.KINDS:
        nm = NM.create(kind)
        monkeypatch.setattr(NM.Normalizer, "batch", False)
        a = read(path, native)
        nm.normalizeAll(a, fids)
        assert not spy, "the list by list path must not reach rl_normalize_lists"
        monkeypatch.setattr(NM.Normalizer, "batch", True)
        b = read(path, native)
        before = all_bits(b)
        nm.normalizeAll(b, fids)
        assert len(spy) == 1, (kind, len(spy))
        del spy[:]
        wa, wb = all_bits(a), all_bits(b)
        assert len(wa) == len(wb) and all(np.array_equal(x, y) for x, y in zip(wa, wb)), kind
        assert any(not np.array_equal(x, y) for x, y in zip(before, wb))


def test_reader_made_rows_are_normalised_in_place_without_a_copy(spy):
    lists = read(LETOR[0], True)
    B = lists[0].rl[0].fVals.base
    assert isinstance(B, np.ndarray) and B.ndim == 2
    NM.create("sum").normalizeAll(lists)
    assert len(spy) == 1 and spy[0][2] == B.ctypes.data and spy[0][5] is not None      # X is the reader's matrix, row_len is given
    part = lists[3:9]                                                               # a run of lists from the middle: still one matrix
    NM.create("linear").normalizeAll(part)
    first = part[0].rl[0].fVals
    assert len(spy) == 2 and spy[1][2] == first.__array_interface__["data"][0]
    NM.create("linear").normalizeAll([lists[5], lists[2]])                          # out of order: copied rows
    assert len(spy) == 3 and not (B.ctypes.data <= spy[2][2] < B.ctypes.data + B.nbytes)


def ragged_lists():
    mk = lambda *v: DataPoint.from_parsed(1.0, "q", "", np.array((np.nan,) + v, np.float32))     # noqa: E731
    return [RankList([mk(1.0, 3.0, 5.0), mk(3.0, 1.0)]), RankList([mk(2.0, 2.0, 2.0), mk(4.0, 1.0, 0.5)])]


def test_a_ragged_file_falls_back_with_the_parent_s_error(spy, monkeypatch):
    texts, values = [], []
    for batch in (False, True):
        monkeypatch.setattr(NM.Normalizer, "batch", batch)
        for fids in (None, [1, 3]):
            with pytest.raises(learning.RankLibError) as e:
                NM.create("zscore").normalizeAll(ragged_lists(), fids)
            texts.append(str(e.value))
        # a subset that every row holds is no fallback
        lists = ragged_lists()
        NM.create("sum").normalizeAll(lists, [2, 1])
        values.append(all_bits(lists))
        assert len(spy) == (1 if batch else 0)
        del spy[:]
        empty = ragged_lists() + [RankList([])]
        with pytest.raises(learning.RankLibError) as e:
            NM.create("linear").normalizeAll(empty, [1])
        texts.append(str(e.value))
        assert not spy
    assert texts[:3] == texts[3:] and "unspecified feature" in texts[0] and "ranked list is empty" in texts[2]
    assert all(np.array_equal(x, y) for x, y in zip(*values))
    # lists of different feature counts, every feature: list by list (each list has its own ids)
    monkeypatch.setattr(NM.Normalizer, "batch", True)
    mk = lambda *v: DataPoint.from_parsed(1.0, "q", "", np.array((np.nan,) + v, np.float32))     # noqa: E731
    two = [RankList([mk(1.0, 3.0), mk(3.0, 1.0)]), RankList([mk(2.0, 2.0, 2.0), mk(4.0, 1.0, 0.5)])]
    NM.create("sum").normalizeAll(two)
    assert not spy and two[0].rl[0].fVals[1] == 0.25 and two[1].rl[1].fVals[3] == np.float32(0.2)


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def write_data(path, n_lists=9, seed=5):
    rng = np.random.RandomState(seed)
    with open(path, "w") as f:
        for q in range(n_lists):
            for _ in range(int(rng.randint(4, 12))):
                x = rng.rand(5) * [1, 10, 100, 1, 5]
                f.write("%d qid:%d %s\n" % (int(x[0] * 3 + x[3] > 2) + int(x[1] > 7), q, " ".join("%d:%.5g" % (j + 1, v) for j, v in enumerate(x))))


@pytest.fixture
def tree_statics(monkeypatch):
    """-tree and -leaf set the statics of LambdaMART and of RFRanker (eval/Evaluator.java:326-337) and nothing resets them: put back after"""
    for cls in (learning.LambdaMART, learning.RFRanker):
        for name in ("nTrees", "nTreeLeaves"):
            monkeypatch.setattr(cls, name, getattr(cls, name))
    for name in ("normalize", "nml"):                 # -norm's statics outlive main() too
        monkeypatch.setattr(evaluator.Evaluator, name, getattr(evaluator.Evaluator, name))


@pytest.mark.parametrize("kind", NR.KINDS)
def test_cli_training_on_normalised_lists_saves_the_same_model(kind, tmp_path, spy, monkeypatch, tree_statics):
    data = str(tmp_path / "data.txt")
    write_data(data)
    models = []
    for batch in (True, False):
        monkeypatch.setattr(NM.Normalizer, "batch", batch)
        out = str(tmp_path / ("m%d.txt" % batch))
        evaluator.main(["-train", data, "-ranker", "6", "-metric2t", "NDCG@10", "-tree", "3", "-leaf", "4", "-norm", kind, "-save", out])
        models.append(open(out, "rb").read())
        assert len(spy) == (1 if batch else 0)
        del spy[:]
    assert models[0] == models[1] and b"<ensemble>" in models[0]


def test_cli_kcv_normalises_the_file_once_for_all_folds(tmp_path, spy, monkeypatch, tree_statics):
    data = str(tmp_path / "data.txt")
    write_data(data, n_lists=10)
    models = []
    for batch in (True, False):
        monkeypatch.setattr(NM.Normalizer, "batch", batch)
        d = str(tmp_path / ("models%d" % batch))
        evaluator.main(["-train", data, "-ranker", "6", "-metric2t", "NDCG@10", "-tree", "3", "-leaf", "4", "-norm", "sum", "-kcv", "3",
                        "-kcvmd", d, "-kcvmn", "m.txt"])
        models.append([open(os.path.join(d, "f%d.m.txt" % (i + 1)), "rb").read() for i in range(3)])
        assert len(spy) == (1 if batch else 0)
        if batch:
            assert spy[0][10] == 9               # times = nFold * nFold
        del spy[:]
    assert models[0] == models[1] and len(set(models[0])) == 3
