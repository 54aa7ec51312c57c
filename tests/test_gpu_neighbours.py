"""rl_model_predict_neighbours on the GPU (the leaves' walk, k_near_match and k_near_merge, rl_near.inc) against plain NumPy on
the walk of tests/leaves_reference.py: equal leaves counted per pair, np.lexsort((index, -shared)) per query.  Integers only, no tolerance.
Every model runs on the default handle and under RLHIP_EVAL_GENERIC, as in tests/test_gpu_leaves.py, whose models, rows and leaves are shared."""
import functools
import os

import numpy as np
import pytest

import leaves_reference as LR
import test_gpu_leaves as GL
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import neighbours as NB

pytestmark = pytest.mark.gpu

QT, RT, TC = N.NEAR_QUERY_TILE, N.NEAR_REF_TILE, N.NEAR_TREE_CHUNK
MIXED = "shapes_%d" % GL.COUNTS[-1]                        # the 67 trees of mixed shape
NQ = (1, QT - 1, QT, QT + 1)                               # both sides of a block's queries
NR = (1, RT - 1, RT, RT + 1, 2 * RT + 1)                   # both sides of a step's references; three tiles, which one or two query tiles cut into three splits
BOTH = GL.BOTH


@functools.lru_cache(maxsize=None)
def subject(name):
    """(trees, query rows, reference rows, their leaves): GL.subject's 258 rows ask, the same rows in reverse order answer -- every
    query meets itself somewhere.  stumps: three stumps, counts in 0 .. 3, so nearly every decision is a tie the index rule decides."""
    if name == "stumps":
        rng = np.random.default_rng(41)
        g = TM.Gen(rng)
        trees = [TM.stump(g) for _ in range(3)]
        rows = np.ascontiguousarray(TM.probe_rows(rng, trees, 400, 13)[rng.permutation(400)][:GL.DOCS[-1]])
        lq = LR.leaves(trees, rows)
    else:
        trees, _, rows, lq = GL.subject(name)
    ref = np.ascontiguousarray(rows[::-1])
    lr = np.ascontiguousarray(lq[::-1])
    lr.setflags(write=False)
    return trees, rows, ref, lq, lr


@functools.lru_cache(maxsize=None)
def handle(name, generic):
    if name != "stumps":
        return GL.handle(name, generic)
    old = os.environ.pop("RLHIP_EVAL_GENERIC", None)       # the knobs are read inside rl_model_from_text
    os.environ.update({"RLHIP_EVAL_GENERIC": "1"} if generic else {})
    try:
        return N.Model(TM.model_text(subject(name)[0], np.ones(3, np.float32)))
    finally:
        os.environ.pop("RLHIP_EVAL_GENERIC", None)
        os.environ.update({} if old is None else {"RLHIP_EVAL_GENERIC": old})


def reference(lq, lr, k, skip_same=False):
    """(index [nq][k], shared [nq][k], the matrix [nq][nr]) of leaves lq [nq][trees] against lr [nr][trees]"""
    shared = (lq[:, None, :] == lr[None, :, :]).sum(-1)
    index, count = np.full((len(lq), k), -1, np.int32), np.zeros((len(lq), k), np.int32)
    for q in range(len(lq)):
        order = np.lexsort((np.arange(len(lr)), -shared[q]))
        order = (order[order != q] if skip_same else order)[:k]
        index[q, :len(order)], count[q, :len(order)] = order, shared[q, order]
    return index, count, shared


def same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert np.array_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:5])


@BOTH
@pytest.mark.parametrize("name", ["stumps", MIXED, "big"])
def test_neighbours_equal_the_reference_at_every_set_size_and_k(name, generic):
    _, rows, ref, lq, lr = subject(name)
    m = handle(name, generic)
    if name == "big":
        assert lq[:, 1].max() > 255                        # numbers that need their high byte
    for nq in NQ:
        for nr in NR:
            for k in {1, 5, N.NEAR_MAX_K, min(nr, N.NEAR_MAX_K), min(nr + 2, N.NEAR_MAX_K)}:      # k == nr and k > nr (the -1 / 0 padding) wherever 64 allows
                got = m.predict_neighbours(rows[:nq], ref[:nr], k)
                same(got, reference(lq[:nq], lr[:nr], k), (name, nq, nr, k))
                if k > nr:
                    assert (got[0][:, nr:] == -1).all() and (got[1][:, nr:] == 0).all()
    assert m.path() == N.MODEL_PATH_NEIGHBOURS
    leaves = m.predict_leaves(rows[:3])
    assert m.path() == (N.MODEL_PATH_TILED if not generic and name != "big" else N.MODEL_PATH_GENERIC) and np.array_equal(leaves, lq[:3])


@BOTH
@pytest.mark.parametrize("first,count", [(0, 1), (0, 2), (0, 3), (0, TC - 1), (0, TC), (0, TC + 1), (1, 2), (3, TC), (1, None), (0, None)])
def test_every_window_equals_the_reference_on_its_columns(first, count, generic):
    """1, 2 and 3 trees: the odd tail of the packing; both sides of the staged chunk; windows that start at an odd tree"""
    _, rows, ref, lq, lr = subject(MIXED)
    cols = slice(first, None if count is None else first + count)
    got = handle(MIXED, generic).predict_neighbours(rows[:QT + 1], ref[:RT + 1], 5, first, count, matrix=True)
    want = reference(lq[:QT + 1, cols], lr[:RT + 1, cols], 5)
    same(got, want, (first, count))
    assert np.array_equal(got[2], want[2])


@BOTH
@pytest.mark.parametrize("name", ["stumps", MIXED])
def test_no_document_is_its_own_neighbour_under_skip_same(name, generic):
    trees, rows, _, lq, _ = subject(name)
    m, n = handle(name, generic), 2 * RT + 1
    got = m.predict_neighbours(rows[:n], rows[:n], 5, skip_same=True)
    same(got, reference(lq[:n], lq[:n], 5, skip_same=True), name)
    assert (got[0] != np.arange(n)[:, None]).all()
    got = m.predict_neighbours(rows[:n], rows[:n], N.NEAR_MAX_K)           # without the flag it is, with every tree shared
    same(got, reference(lq[:n], lq[:n], N.NEAR_MAX_K), name)
    at = got[0] == np.arange(n)[:, None]
    full = (lq[:n, None, :] == lq[None, :n, :]).all(-1)                    # (three stumps: 64 earlier documents may share every tree too)
    crowded = np.array([full[q, :q].sum() >= N.NEAR_MAX_K for q in range(n)])
    assert np.array_equal(at.sum(1), 1 - crowded) and (got[1][at] == len(trees)).all() and not crowded[:N.NEAR_MAX_K].any()


@BOTH
@pytest.mark.parametrize("name", ["stumps", MIXED, "big"])
def test_the_matrix_and_the_chunked_call_change_nothing(name, generic):
    _, rows, ref, lq, lr = subject(name)
    m, nq, nr = handle(name, generic), 2 * QT + 2, 2 * RT + 1
    want = reference(lq[:nq], lr[:nr], 5)
    plain = m.predict_neighbours(rows[:nq], ref[:nr], 5)
    same(plain, want, name)
    index, shared, matrix = m.predict_neighbours(rows[:nq], ref[:nr], 5, matrix=True)
    assert matrix.dtype == np.uint16 and np.array_equal(matrix, want[2])
    same((index, shared), plain, name)
    # one byte of scratch: chunks of 64 queries and bands of 128 references, three of either
    index, shared, matrix = m.predict_neighbours(rows[:nq], ref[:nr], 5, matrix=True, scratch_bytes=1)
    same((index, shared), plain, name)
    assert np.array_equal(matrix, want[2])
    same(m.predict_neighbours(rows[:nq], rows[:nq], 5, skip_same=True, scratch_bytes=1), reference(lq[:nq], lq[:nq], 5, skip_same=True), name)


@BOTH
@pytest.mark.parametrize("nq", [1, QT + 1])
@pytest.mark.parametrize("name", ["stumps", MIXED])
def test_a_block_sweeps_several_reference_tiles(name, nq, generic):
    """65 reference tiles are more than the 63 splits a launch has: two tiles a split, so a block counts, scans and inserts twice over
    one list, and a last split of one tile (tests/test_neighbours_cpu.py pins that plan).  The 258 rows repeat, so every list is ties."""
    _, rows, _, lq, _ = subject(name)
    nr = 64 * RT + 1
    ref, lr = np.resize(rows, (nr, rows.shape[1])), np.resize(lq, (nr, lq.shape[1]))      # row i is rows[i % 258]: a query's own index holds its own row
    m = handle(name, generic)
    for k, skip in ((5, False), (N.NEAR_MAX_K, True)):
        want = reference(lq[:nq], lr, k, skip_same=skip)
        same(m.predict_neighbours(rows[:nq], ref, k, skip_same=skip), want, (name, nq, k, "lists"))
        index, shared, matrix = m.predict_neighbours(rows[:nq], ref, k, skip_same=skip, matrix=True)
        same((index, shared), want, (name, nq, k, "with the matrix"))
        assert np.array_equal(matrix, want[2])
    # scratch for 512 rows and their leaf numbers: the queries' share taken, bands of 3 tiles, 22 of them merged into the running lists
    same(m.predict_neighbours(rows[:nq], ref, 5, scratch_bytes=512 * (4 * rows.shape[1] + 2 * ((lq.shape[1] + 3) & ~3))), reference(lq[:nq], lr, 5), (name, nq, "bands"))


def test_the_refusals_that_need_a_model():
    _, rows, ref, _, _ = subject(MIXED)
    m, out = handle(MIXED, False), np.zeros(4, np.int32)
    for first, cnt, text in ((67, None, "first_tree = 67 is outside [0, 67)"), (32, 67, "n_trees = 67 from tree 32 leaves the model's 67 trees")):
        with pytest.raises(N.RankLibError, match="rl_model_predict_neighbours: " + text.replace("[", r"\[").replace(")", r"\)")):
            m.predict_neighbours(rows[:2], ref[:2], 1, first, cnt)
    for nq, nr in ((1 << 31, 2), (2, 1 << 31)):
        rc = N.lib().rl_model_predict_neighbours(m.h, rows.ctypes.data, nq, rows.ctypes.data, nr, rows.shape[1], 0, 0, 1, 0, 0, out.ctypes.data, out.ctypes.data, None)
        assert (rc, N.lib().rl_last_error().decode()) == (-4, "rl_model_predict_neighbours: more than 2^31 rows per call")


@pytest.mark.parametrize("own", [False, True], ids=["reference", "self"])
def test_the_command_line_writes_the_reference_neighbours(tmp_path, own):
    from ranklib_amd.features import FeatureManager
    rng = np.random.default_rng(2)
    g = TM.Gen(rng, features=range(1, 7), thresholds=np.array([0.0, 0.5, 1.0, 6.0, 17.0, 31.55577], np.float32))
    trees = [TM.random_tree(g, 5), TM.random_tree(g, 3)]
    mf, out = str(tmp_path / "m.txt"), str(tmp_path / "near.tsv")
    with open(mf, "w", encoding="ascii") as f:
        f.write(TM.model_text(trees, np.full(2, 0.1, np.float32)))
    test = os.path.join(GL.ROOT, "tests", "golden", "letor", "small_ns.train.txt")
    assert NB.main(["-load", mf, "-test", test, "-k", "3", "-out", out] + (["-self"] if own else ["-reference", test])) == 0
    dps = [dp for rl in FeatureManager.readInput(test) for dp in rl.rl]
    lv = LR.leaves(trees, np.stack([np.nan_to_num(dp.fVals, nan=0.0) for dp in dps]).astype(np.float32))
    index, shared, _ = reference(lv, lv, 3, skip_same=own)
    assert len(np.unique(lv[:, 0])) > 1 and len(np.unique(index[:, 0])) > 1
    assert open(out).read() == "".join("%s\t%s\t%d\t%s\t%s\t%d\t%d\t2\n" % (dp.id, dp.description or "", j + 1, dps[i].id, dps[i].description or "",
                                                                         int(dps[i].label), s)
                                       for dp, ids, cnt in zip(dps, index, shared) for j, (i, s) in enumerate(zip(ids, cnt)) if i >= 0)
