"""rl_model_predict_leaves on the GPU (k_model_leaves_tiled and k_model_leaves, rl_leaves.inc) against the plain NumPy walk
of tests/leaves_reference.py.  Every comparison is of integers: there is no tolerance in this file.  Every model runs twice from the
same text, as the scoring tests run theirs: the default handle, and one made with RLHIP_EVAL_GENERIC set, which takes k_model_leaves."""
import functools
import os

import numpy as np
import pytest

import leaves_reference as LR
import tree_models as TM
import walk_cases as WC
from ranklib_amd import _native as N
from ranklib_amd import leaves as LV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 32            # kEvalTreeTile = RL_EVAL_PARTS x RL_EVAL_PER of ranklib_amd/csrc/rl_eval_pack_host.h: 4 walkers x 8 trees each
COUNTS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)      # trees of the hand-built family: both sides of the tile, and a third, partial tile
DOCS = (1, 63, 64, 65, 258)                               # both sides of a block of 64 documents, and five blocks
BOTH = pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])


@functools.lru_cache(maxsize=None)
def shapes():
    """what the scoring edges do not reach: a one-node tree (its leaf is always 0), a two-leaf tree, a left and a right chain of depth
    12, then trees of 2 .. 16 leaves mixed within every tile; rows that meet their thresholds"""
    rng = np.random.default_rng(38)
    g = TM.Gen(rng)
    trees = [TM.single_leaf(g), TM.stump(g), TM.chain(g, 12, "left"), TM.chain(g, 12, "right")]
    trees += [TM.random_tree(g, int(rng.integers(2, 17))) for _ in range(COUNTS[-1] - len(trees))]
    rows = TM.probe_rows(rng, trees, 400, 13)[rng.permutation(400)][:DOCS[-1]]
    return trees, np.ascontiguousarray(rows)


@functools.lru_cache(maxsize=None)
def subject(name):
    """(trees, weights, rows, the reference leaves [rows][trees]) of a case: WC.CASES, shapes_<T>, or big -- one tree of 300 leaves, whose
    numbers need their high byte and which the tiled packing refuses (599 nodes), between two small ones"""
    if name.startswith("shapes_"):
        trees, rows = shapes()
        trees = trees[:int(name[7:])]
    elif name == "big":
        rng = np.random.default_rng(300)
        g = TM.Gen(rng)
        trees = [TM.stump(g), TM.random_tree(g, 300), TM.random_tree(g, 5)]
        rows = TM.probe_rows(rng, trees, 400, 13)[rng.permutation(400)][:DOCS[-1]]
    else:
        trees, rows = WC.trees_of(name)[0], WC.rows(name)[:DOCS[-1]]
    w = TM.WEIGHTS[np.arange(len(trees)) % len(TM.WEIGHTS)]
    want = LR.leaves(trees, rows)
    want.setflags(write=False)
    return trees, w, rows, want


@functools.lru_cache(maxsize=None)
def handle(name, generic):
    trees, w, _, _ = subject(name)
    old = os.environ.pop("RLHIP_EVAL_GENERIC", None)       # the knobs are read inside rl_model_from_text
    try:
        if generic:
            os.environ["RLHIP_EVAL_GENERIC"] = "1"
        return N.Model(TM.model_text(trees, w))
    finally:
        os.environ.pop("RLHIP_EVAL_GENERIC", None)
        if old is not None:
            os.environ["RLHIP_EVAL_GENERIC"] = old


SUBJECTS = WC.CASES + tuple("shapes_%d" % t for t in COUNTS) + ("big",)


@BOTH
@pytest.mark.parametrize("name", SUBJECTS)
def test_leaves_equal_the_reference_in_both_layouts(name, generic):
    trees, _, rows, want = subject(name)
    m = handle(name, generic)
    m.predict_rows(rows[:1])
    scoring = m.path()                                     # the leaves' packing takes what the scorer's takes
    if name.startswith("shapes_"):
        assert scoring == (N.MODEL_PATH_GENERIC if generic else N.MODEL_PATH_TILED)
    if name == "big":
        assert scoring == N.MODEL_PATH_GENERIC and want[:, 1].max() > 255
    assert np.array_equal(m.leaf_counts(), LR.counts(trees))
    for n in DOCS:
        m.cover(rows[:1])                                  # another path in between: what follows is what predict_leaves itself reports
        assert m.path() == N.MODEL_PATH_COVER
        got = m.predict_leaves(rows[:n])
        assert m.path() == scoring, (name, n, m.path())
        assert got.dtype == np.uint16 and np.array_equal(got, want[:n]), (name, n, np.argwhere(got != want[:n])[:5])
        by_tree = m.predict_leaves(rows[:n], by_tree=True)
        assert np.array_equal(by_tree, want[:n].T), (name, n, np.argwhere(by_tree != want[:n].T)[:5])


@BOTH
@pytest.mark.parametrize("by_tree", [False, True], ids=["by_row", "by_tree"])
def test_every_window_equals_the_columns_of_the_full_result(generic, by_tree):
    name = "shapes_%d" % COUNTS[-1]
    _, _, rows, want = subject(name)
    m = handle(name, generic)
    for first in (0, 1, 3, TILE - 1, TILE, TILE + 1):           # (3 and TILE - 1: windows of two whole tiles, and of one and four trees more)
        for cnt in (0, 1, TILE):                           # 0: through the last tree
            cols = want[:65, first:] if cnt == 0 else want[:65, first:first + cnt]
            got = m.predict_leaves(rows[:65], first, cnt, by_tree)
            assert np.array_equal(got, cols.T if by_tree else cols), (first, cnt)
    for first, cnt, text in ((COUNTS[-1], 0, "first_tree = 67 is outside [0, 67)"), (TILE, COUNTS[-1], "n_trees = 67 from tree 32 leaves the model's 67 trees")):
        with pytest.raises(N.RankLibError, match="rl_model_predict_leaves: " + text.replace("[", r"\[").replace(")", r"\)")):
            m.predict_leaves(rows[:2], first, cnt, by_tree)


@BOTH
def test_the_leaves_give_the_leaf_sums_bit_for_bit(generic):
    """s = s + (double) weight * (double) output of the leaf, tree after tree: rl_model_predict_leaf_sums' own chain over the returned leaves"""
    trees, w, rows, _ = subject("thresholds_deep")
    m = handle("thresholds_deep", generic)
    got = m.predict_leaves(rows)
    s = np.zeros(len(rows), np.float64)
    with np.errstate(all="ignore"):
        for k, t in enumerate(trees):
            outs = t["output"][t["feature"] == -1].astype(np.float64)
            s = s + np.float64(np.float32(w[k])) * outs[got[:, k]]
    assert np.array_equal(s.view(np.uint64), m.leaf_sums(rows).view(np.uint64))


def test_the_command_line_writes_the_reference_walk(tmp_path):
    from ranklib_amd.features import FeatureManager
    rng = np.random.default_rng(2)
    g = TM.Gen(rng, features=range(1, 7), thresholds=np.array([0.0, 0.5, 1.0, 6.0, 17.0, 31.55577], np.float32))
    trees = [TM.random_tree(g, 5), TM.random_tree(g, 3)]
    mf, out, letor, npy = (str(tmp_path / n) for n in ("m.txt", "leaves.tsv", "onehot.txt", "leaves.npy"))
    with open(mf, "w", encoding="ascii") as f:
        f.write(TM.model_text(trees, np.full(2, 0.1, np.float32)))
    test = os.path.join(ROOT, "tests", "golden", "letor", "small_ns.train.txt")
    assert LV.main(["-load", mf, "-test", test, "-out", out, "-letor", letor, "-npy", npy]) == 0
    dps = [dp for rl in FeatureManager.readInput(test) for dp in rl.rl]
    rows = np.stack([np.nan_to_num(dp.fVals, nan=0.0) for dp in dps]).astype(np.float32)
    want = LR.leaves(trees, rows)
    assert len(np.unique(want[:, 0])) > 1 and np.array_equal(np.load(npy), want)
    assert open(out).read() == "".join("%s\t%d\t%d\n" % (dp.id, a, b) for dp, (a, b) in zip(dps, want))
    assert open(letor).read() == "".join("%d qid:%s %d:1 %d:1\n" % (int(dp.label), dp.id, 1 + a, 6 + b) for dp, (a, b) in zip(dps, want))
    assert LV.main(["-load", mf, "-test", test, "-from", "1", "-count", "1", "-out", out, "-letor", letor]) == 0
    assert open(letor).read() == "".join("%d qid:%s %d:1\n" % (int(dp.label), dp.id, 1 + b) for dp, b in zip(dps, want[:, 1]))
