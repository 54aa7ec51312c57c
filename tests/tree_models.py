"""Hand-built tree ensembles, their RankLib model text and an independent evaluation of them -- TEST INFRASTRUCTURE ONLY.

The scoring kernels (rl_model_*: k_model_eval_tiled, k_model_eval) are otherwise only tested on models this project trained itself, whose
trees all look alike.  Here trees are built node by node -- single leaves, stumps, balanced trees, chains, random shapes -- with any
threshold, output and weight a model file can hold, written as RankLib prints them, and evaluated by `eval_ensemble_np`: Split.eval
(learning/tree/Split.java:115-125) and Ensemble.eval (learning/tree/Ensemble.java:110-116) in plain numpy, vectorised over documents.  It
does not call the oracle; tests/test_tree_models_cpu.py holds the two against each other on every case below, without a GPU.

A tree is a dict of arrays in pre-order (the order Ensemble.create numbers the nodes in): feature (-1 = leaf), threshold, left, right
(-1 at a leaf), output.  CASES names every model and row set tests/test_gpu_model_eval.py scores.
"""
import collections
import functools

import numpy as np

from ranklib_amd.learning import java_double_str, java_float_str

# k_model_eval_tiled's shape (rl_model_eval.inc): documents of a block, trees of an LDS tile, trees of a walker wavefront, walkers, phases
DOCS, TILE, PER, PARTS, PHASES = 64, 32, 8, 4, 3
LDS_BUDGET = 160 * 1024
F32_MAX = np.float32(3.4028235e38)        # Float.MAX_VALUE
F32_MIN = np.float32(1.4e-45)             # Float.MIN_VALUE, the smallest subnormal
F32_MIN_NORMAL = np.float32(1.17549435e-38)
GRID = (np.arange(-32, 33) / 16.0).astype(np.float32)          # 65 exact values: ordinary thresholds that rows hit exactly


def tiled_lds_bytes(cols, maxn):
    """eval_tiled_lds: the staged rows [cols][DOCS], one tile of packed nodes, the double-buffered leaf outputs and weights, and the
    double-buffered walker assignment with the walkers' steps and phase ends"""
    return cols * DOCS * 4 + TILE * maxn * 8 + 2 * TILE * DOCS * 4 + 2 * TILE * 4 + 2 * (TILE + PARTS * (1 + PHASES))


def max_tiled_cols(maxn):
    """the widest staged row (max(row_stride, largest feature id + 1)) the tiled kernel's LDS budget admits"""
    return (LDS_BUDGET - tiled_lds_bytes(0, maxn)) // (DOCS * 4)


# ---- builder --------------------------------------------------------------------------------------------------------------------------
def L(out):
    return ("leaf", out)


def S(feature, threshold, left, right):
    return ("split", feature, threshold, left, right)


def flatten(nested):
    feat, thr, left, right, out = [], [], [], [], []

    def rec(nd):
        me = len(feat)
        feat.append(-1); thr.append(0.0); left.append(-1); right.append(-1); out.append(0.0)
        if nd[0] == "leaf":
            out[me] = nd[1]
        else:
            feat[me], thr[me] = nd[1], nd[2]
            left[me] = rec(nd[3])
            right[me] = rec(nd[4])
        return me

    rec(nested)
    with np.errstate(over="ignore"):
        return dict(feature=np.array(feat, np.int32), threshold=np.array(thr, np.float32), left=np.array(left, np.int32),
                    right=np.array(right, np.int32), output=np.array(out, np.float32))


def depth_of(tree):
    d = np.zeros(len(tree["feature"]), np.int64)
    for j in range(len(d)):                      # pre-order: a parent comes before its children
        if tree["feature"][j] != -1:
            d[tree["left"][j]] = d[tree["right"][j]] = d[j] + 1
    return int(d.max())


class Gen:
    """where a shape takes its splits and leaf outputs from"""

    def __init__(self, rng, features=range(1, 13), thresholds=GRID, outputs=None):
        self.rng, self.features, self.thresholds, self.outputs = rng, list(features), np.asarray(thresholds, np.float32), outputs

    def split(self):
        return int(self.rng.choice(self.features)), np.float32(self.rng.choice(self.thresholds))

    def out(self):
        if self.outputs is not None:
            return np.float32(self.rng.choice(self.outputs))
        return np.float32(self.rng.standard_normal())           # arbitrary bits: nine-digit outputs in the text


def single_leaf(g):
    return flatten(L(g.out()))


def stump(g):
    f, t = g.split()
    return flatten(S(f, t, L(g.out()), L(g.out())))


def balanced(g, depth):
    def rec(d):
        if d == 0:
            return L(g.out())
        f, t = g.split()
        return S(f, t, rec(d - 1), rec(d - 1))
    return flatten(rec(depth))


def chain(g, depth, side):
    """`depth` splits on ONE feature, every split's `side` child the next split.  The thresholds are consecutive GRID values, falling down a
    left chain and rising down a right one, so a document leaves the chain at the level its value decides and documents spread over all
    of them (with independent splits one document in 2^depth would reach the bottom)."""
    assert depth <= len(GRID) and side in ("left", "right")
    f = g.split()[0]
    a = int(g.rng.integers(0, len(GRID) - depth + 1))
    ths = GRID[a:a + depth]
    if side == "left":
        ths = ths[::-1]
    nd = L(g.out())
    for t in ths[::-1]:
        nd = S(f, t, nd, L(g.out())) if side == "left" else S(f, t, L(g.out()), nd)
    return flatten(nd)


def random_tree(g, n_leaves):
    """grown by splitting a random leaf n_leaves - 1 times"""
    nodes = [["leaf"]]
    leaves = [0]
    for _ in range(n_leaves - 1):
        j = leaves.pop(int(g.rng.integers(0, len(leaves))))
        f, t = g.split()
        nodes[j] = ["split", f, t, len(nodes), len(nodes) + 1]
        leaves += [len(nodes), len(nodes) + 1]
        nodes += [["leaf"], ["leaf"]]

    def rec(j):
        nd = nodes[j]
        return L(g.out()) if nd[0] == "leaf" else S(nd[1], nd[2], rec(nd[3]), rec(nd[4]))
    return flatten(rec(0))


def _jfloat(v):
    """Float.toString.  java_float_str gives the shortest digits that round-trip; where those are ONE digit the Java prints the nearest
    decimal of two (Float.MIN_VALUE is "1.4E-45", not "1.0E-45"), which differs from "d.0" only among the smallest subnormals."""
    v = np.float32(v)
    if not np.isfinite(v):
        return java_double_str(float(v))             # NaN, Infinity, -Infinity read the same for both
    s = java_float_str(v)
    if "E" in s and s.split("E")[0].lstrip("-").endswith(".0") and len(s.split("E")[0].lstrip("-")) == 3:
        m, e = ("%.1e" % float(v)).split("e")
        s = m + "E" + str(int(e))
        assert np.float32(float(s)) == v
    return s


def model_text(trees, weights):
    """LambdaMART.model(): the header, Ensemble.toString (Ensemble.java:119-130) and Split.getString (Split.java:140-155).  Thresholds and
    weights are Float.toString, outputs Double.toString of the widened float, as the Java writes them."""
    assert len(trees) == len(weights)
    o = ["## LambdaMART\n## No. of trees = %d\n## No. of leaves = 10\n## No. of threshold candidates = 256\n## Learning rate = 0.1\n"
         "## Stop early = 100\n\n<ensemble>\n" % len(trees)]

    def node(t, j, ind):
        if t["feature"][j] == -1:
            o.append("%s<output>%s </output>\n" % (ind, java_double_str(float(np.float32(t["output"][j])))))
            return
        o.append("%s<feature>%d </feature>\n%s<threshold> %s </threshold>\n" % (ind, t["feature"][j], ind, _jfloat(t["threshold"][j])))
        for pos, c in (("left", t["left"][j]), ("right", t["right"][j])):
            o.append("%s<split pos=\"%s\">\n" % (ind, pos))
            node(t, int(c), ind + "\t")
            o.append("%s</split>\n" % ind)

    for i, t in enumerate(trees):
        o.append("\t<tree id=\"%d\" weight=\"%s\">\n\t\t<split>\n" % (i + 1, _jfloat(weights[i])))
        node(t, 0, "\t\t\t")
        o.append("\t\t</split>\n\t</tree>\n")
    o.append("</ensemble>\n")
    return "".join(o)


# ---- reference ------------------------------------------------------------------------------------------------------------------------
def eval_ensemble_np(trees, weights, rows):
    """Ensemble.eval of every row.  Split.eval: a node of feature -1 is a leaf; `value <= threshold` goes left, so NaN (either side) goes
    right; a column at or beyond the row's width reads 0 (DenseDataPoint.getFeatureValue under -missingZero).  Ensemble.eval:
    s = (float) ((double) s + (double) output * (double) weight), tree by tree in the ensemble's order."""
    rows = np.asarray(rows, np.float32)
    n, width = rows.shape
    ar = np.arange(n)
    s = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for t, w in zip(trees, weights):
            nd = np.zeros(n, np.int64)
            while True:
                f = t["feature"][nd]
                act = f != -1
                if not act.any():
                    break
                v = np.where(f < width, rows[ar, np.clip(f, 0, width - 1)], np.float32(0))
                nxt = np.where(v <= t["threshold"][nd], t["left"][nd], t["right"][nd])
                nd = np.where(act, nxt, nd)
            s = (s.astype(np.float64) + t["output"][nd].astype(np.float64) * np.float64(np.float32(w))).astype(np.float32)
    return s


def same_scores(got, want):
    """None, or what differs.  Outside NaN results: bit for bit.  Where the reference is NaN the other is NaN; payload and sign are not
    compared (x86 and the GPU produce different default NaNs from inf * 0)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return "shape %r != %r" % (got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.nonzero(np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32)))[0]
    if bad.size == 0:
        return None
    i = bad[0]
    return "%d of %d scores differ, first at %d: %r (%#010x) != %r (%#010x)" % (bad.size, want.size, i, got[i], got.view(np.uint32)[i],
                                                                                want[i], want.view(np.uint32)[i])


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
SPECIAL_VALUES = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, F32_MIN, -F32_MIN, 1e-40, -1e-40, F32_MIN_NORMAL, F32_MAX, -F32_MAX], np.float32)


def probe_pool(trees):
    """every threshold of the model and its two float neighbours (a threshold the text parser moved by an ulp routes one of them
    differently), then the special values"""
    th = np.unique(np.concatenate([t["threshold"][t["feature"] != -1] for t in trees] + [np.zeros(1, np.float32)]))
    th = th[~np.isnan(th)]
    with np.errstate(all="ignore"):
        near = np.concatenate([th, np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(-np.inf))])
    return near.astype(np.float32)


def probe_rows(rng, trees, n, width, special=0.1):
    """n rows of `width` columns drawn from probe_pool (one cell in ten from SPECIAL_VALUES); the first rows hold one pool value in every
    column, so every value meets every threshold.  Column 0 is 0, as in a DataPoint.  With the cases' 200 rows this prefix
    (len(pool) + 12 rows) is nearly or wholly the whole row set -- 200 of 200 on count_37, 180 on feature_0: right for scoring, next to
    nothing for attribution.  tests/walk_cases.py builds the row sets of the other walks' tests from the prefix and the mixed part."""
    pool = probe_pool(trees)
    rows = pool[rng.integers(0, len(pool), (n, width))]
    sp = rng.random((n, width)) < special
    rows[sp] = SPECIAL_VALUES[rng.integers(0, len(SPECIAL_VALUES), int(sp.sum()))]
    both = np.concatenate([SPECIAL_VALUES, pool])
    k = min(n, len(both))
    rows[:k] = both[:k, None]
    rows[:, 0] = 0.0
    return np.ascontiguousarray(rows, np.float32)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# tiled: the kernel the default build takes for this model at this row width
Case = collections.namedtuple("Case", "trees weights rows tiled")
N_DOCS = 200
WEIGHTS = np.array([0.1, 1.0, 0.5, -0.25, 3.0, 0.7, 1e-3, -1.0], np.float32)
CASES = {}


def _case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


def mixed_trees(g, nt):
    """depths mixed inside every walker's eight: single leaves, stumps, chains of 2 .. 12, balanced and random trees"""
    out = []
    for _ in range(nt):
        k = int(g.rng.integers(0, 6))
        if k == 0:
            out.append(single_leaf(g))
        elif k == 1:
            out.append(stump(g))
        elif k == 2:
            out.append(chain(g, int(g.rng.integers(2, 13)), "left"))
        elif k == 3:
            out.append(chain(g, int(g.rng.integers(2, 13)), "right"))
        elif k == 4:
            out.append(balanced(g, int(g.rng.integers(2, 5))))
        else:
            out.append(random_tree(g, int(g.rng.integers(2, 13))))
    return out


def _finish(rng, trees, weights=None, width=13, n=N_DOCS, tiled=True, rows=None):
    if weights is None:
        weights = WEIGHTS[rng.integers(0, len(WEIGHTS), len(trees))]
    if rows is None:
        rows = probe_rows(rng, trees, n, width)
    rows.setflags(write=False)
    return Case(trees, np.asarray(weights, np.float32), rows, tiled)


# tree counts against the tile (32) and the walkers (8): one partial tile, full tiles, and last tiles of 1 .. 9, 17 and 25 trees -- walkers
# holding 0, 1, 2, 3, 4, 5, 6, 7 and 8 trees, so the trees at positions 6, 4 and 2 of a walker (its phase ends) exist and do not
COUNTS = (1, 7, 8, 9, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 49, 57, 63, 64, 65, 97)
for _nt in COUNTS:
    def _count(nt=_nt):
        rng = _rng("count_%d" % nt)
        return _finish(rng, mixed_trees(Gen(rng), nt))
    CASES["count_%d" % _nt] = _count


def deepest_chain(g, side="left"):
    return chain(g, 39, side)               # 79 nodes: 32 * 79 packed nodes are the 2 560 words the block prefetches per tile


@_case("depth_extremes")
def _depth_extremes():
    rng = _rng("depth_extremes"); g = Gen(rng)
    trees = [single_leaf(g) if i % 3 == 0 else stump(g) for i in range(TILE)]
    trees[13] = deepest_chain(g, "left")
    trees[30] = deepest_chain(g, "right")
    return _finish(rng, trees)


@_case("depth_0_31")
def _depth_0_31():
    rng = _rng("depth_0_31"); g = Gen(rng)
    trees = [single_leaf(g) if d == 0 else chain(g, int(d), "left" if d % 2 else "right") for d in rng.permutation(TILE)]
    assert sorted(depth_of(t) for t in trees) == list(range(TILE))
    return _finish(rng, trees)


@_case("depth_equal")
def _depth_equal():
    rng = _rng("depth_equal"); g = Gen(rng)
    trees = [balanced(g, 4) if i % 2 else chain(g, 4, "left") for i in range(TILE)]
    assert {depth_of(t) for t in trees} == {4}
    return _finish(rng, trees)


@functools.lru_cache(maxsize=None)
def _deep_parts():
    rng = _rng("deep_at"); g = Gen(rng)
    others = [single_leaf(g) if i % 4 == 0 else stump(g) if i % 4 == 1 else random_tree(g, 2 + i % 5) for i in range(TILE - 1)]
    deep = deepest_chain(g)
    weights = WEIGHTS[rng.integers(0, len(WEIGHTS), TILE)]
    rows = probe_rows(rng, others + [deep], N_DOCS, 13)
    return others, deep, weights, rows


for _pos in range(TILE):                    # the one deep tree at each place of the tile in turn; the other trees and the rows stay
    def _deep_at(pos=_pos):
        others, deep, weights, rows = _deep_parts()
        return _finish(None, others[:pos] + [deep] + others[pos:], weights, rows=rows)
    CASES["deep_at_%d" % _pos] = _deep_at
DEPTH_CASES = ["depth_extremes", "depth_0_31", "depth_equal"] + ["deep_at_%d" % p for p in range(TILE)]


def _order_trees(rng, nt, outs):
    """stumps and depth-2 trees whose leaves walk through `outs` in order: any two leaves a document can reach differ"""
    g = Gen(rng); trees = []; k = 0
    for i in range(nt):
        t = stump(g) if i % 2 else balanced(g, 2)
        lv = np.nonzero(t["feature"] == -1)[0]
        t["output"][lv] = [outs[(k + j) % len(outs)] for j in range(len(lv))]
        k += len(lv) + 1
        trees.append(t)
    return trees


@_case("accum_order")
def _accum_order():
    # sums in which every reordering shows: 1e8 + 1 - 1e8 is 0 in float, 1e8 - 1e8 + 1 is 1; laid over 66 trees, so over the tile
    # boundaries 31 | 32 | 33 and 63 | 64 | 65 and over all four walkers.  The weights: 0, negatives, a subnormal and 1e30 among them.
    rng = _rng("accum_order")
    trees = _order_trees(rng, 66, np.array([1e8, 1.0, -1e8, 3.0, 16777216.0, 1.0, -16777216.0, 0.5, 1e-3, -1e8, 7.0, 1e8], np.float32))
    w = np.array([1.0, 0.5, -1.0, 3.0, 0.0, 1e-40, 0.1, -0.25, 2.0, 1.0, 1.0], np.float32)[np.arange(66) % 11]
    w[[31, 32, 33]] = [1.0, -1.0, 1.0]
    w[40] = 1e30; w[41] = -1e30              # 1e8 * 1e30 = 1e38 stays finite; the pair cancels only if nothing is added in between
    return _finish(rng, trees, w)


@_case("accum_specials")
def _accum_specials():
    # leaf outputs a model file can hold: -0.0 and Float.MIN_VALUE on every path (a negative subnormal weight turns MIN_VALUE into -0.0),
    # +-Float.MAX_VALUE and +-Infinity on one leaf of a few trees, so that documents end finite, infinite and NaN: MAX_VALUE twice
    # overflows, Infinity under weight 0 is NaN and so is Infinity - Infinity.
    rng = _rng("accum_specials")
    trees = _order_trees(rng, 66, np.array([1.0, -0.0, 0.25, F32_MIN, 2.0, -1.0, -F32_MIN, 0.0, 0.5, 3.0, F32_MIN_NORMAL], np.float32))
    w = np.array([1.0, 0.5, -1.0, 1e-40, 0.0, -1e-40, 2.0], np.float32)[np.arange(66) % 7]
    for i, out, wi in ((4, F32_MAX, 1.0), (6, -F32_MAX, 1.0), (12, F32_MAX, 0.5), (20, np.inf, 0.0), (31, F32_MAX, 1.0), (32, F32_MAX, 1.0),
                       (34, np.inf, 1.0), (50, -np.inf, 1.0), (64, -F32_MAX, -2.0)):
        t = trees[i]
        t["output"][np.nonzero(t["feature"] == -1)[0][-1]] = out
        w[i] = wi
    return _finish(rng, trees, w)


@_case("nan_leaf")
def _nan_leaf():
    # a NaN leaf output cannot be a packed leaf (`-inf <= NaN` is false): the default build takes the generic kernel
    rng = _rng("nan_leaf"); g = Gen(rng)
    trees = mixed_trees(g, 33)
    trees[17] = flatten(S(3, -1.0, L(np.nan), L(1.0)))
    return _finish(rng, trees, tiled=False)


THRESHOLDS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, F32_MAX, -F32_MAX, F32_MIN, -F32_MIN, F32_MIN_NORMAL, 1e-40, 0.1, 1.0 / 3.0,
                       1e-3, 9.999999e-4, 1e7, 9999999.0, 16777216.0, 0.30000001, 123456.79, -2.7182817], np.float32)


@_case("thresholds")
def _thresholds():
    # every threshold a model file can hold, each met by itself, by its two neighbours and by the special values (probe_rows)
    rng = _rng("thresholds")
    g = Gen(rng, thresholds=THRESHOLDS)
    trees = [flatten(S(1 + i % 12, t, L(g.out()), L(g.out()))) for i, t in enumerate(THRESHOLDS)]
    trees += [balanced(g, 3) for _ in range(TILE + 9 - len(trees))]
    return _finish(rng, trees)


@_case("col0_garbage")
def _col0_garbage():
    # the tiled kernel's leaves "read" column 0 after overwriting it with -infinity: what the rows hold there must not matter
    rng = _rng("col0_garbage"); g = Gen(rng)
    trees = mixed_trees(g, 37)
    rows = probe_rows(rng, trees, N_DOCS, 13)
    rows[:, 0] = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 123.0], np.float32)[np.arange(N_DOCS) % 7]
    return _finish(rng, trees, rows=rows)


@functools.lru_cache(maxsize=None)
def _width_parts():
    rng = _rng("width"); g = Gen(rng, features=[1, 3, 5, 12])
    trees = mixed_trees(g, 37)
    weights = WEIGHTS[rng.integers(0, len(WEIGHTS), len(trees))]
    rows = probe_rows(rng, trees, N_DOCS, 20)
    for c in range(20):
        if c not in (1, 3, 5, 12):
            rows[:, c] = np.nan              # columns no node reads, column 0 among them
    return trees, weights, rows


for _w in (20, 13, 12, 5, 2, 1):            # wider than the model, exactly maxcol + 1, and narrower down to one column: missing columns read 0
    def _width(w=_w):
        trees, weights, rows = _width_parts()
        return _finish(None, trees, weights, rows=np.ascontiguousarray(rows[:, :w]))
    CASES["width_%d" % _w] = _width


@_case("feature_0")
def _feature_0():
    # RankLib numbers features from 1, but a model file may say 0: the row's own column 0 is read, by the generic kernel
    rng = _rng("feature_0"); g = Gen(rng, features=range(0, 5))
    trees = mixed_trees(g, 33)
    trees[5] = flatten(S(0, 0.25, L(1.0), L(2.0)))
    rows = probe_rows(rng, trees, N_DOCS, 5)
    rows[:, 0] = rows[:, 1][::-1]
    return _finish(rng, trees, rows=rows, tiled=False)


# ---- the boundaries of kernel selection
@_case("nodes_79")
def _nodes_79():
    rng = _rng("nodes_79"); g = Gen(rng)
    trees = mixed_trees(g, 33); trees[32] = deepest_chain(g)
    assert max(len(t["feature"]) for t in trees) == 79
    return _finish(rng, trees)


@_case("nodes_81")
def _nodes_81():
    rng = _rng("nodes_81"); g = Gen(rng)
    trees = mixed_trees(g, 33); trees[32] = chain(g, 40, "left")          # 32 * 81 words are more than a block prefetches
    assert max(len(t["feature"]) for t in trees) == 81
    return _finish(rng, trees, tiled=False)


def _feat_edge(fid, tiled):
    rng = _rng("feat_%d" % fid)
    trees = mixed_trees(Gen(rng, features=[1, 2, fid - 1, fid]), 9)
    trees[4] = flatten(S(fid, 0.5, L(1.0), L(-1.0)))
    return _finish(rng, trees, width=fid + 1, tiled=tiled)


CASES["feat_254"] = lambda: _feat_edge(254, True)        # column offsets are 16 bits: (254 + 1) * 256 bytes is the last that fits
CASES["feat_255"] = lambda: _feat_edge(255, False)


def _lds_edge(extra, tiled):
    rng = _rng("lds")
    trees = [stump(Gen(rng)) for _ in range(33)]
    return _finish(rng, trees, width=max_tiled_cols(3) + extra, n=70, tiled=tiled)


CASES["lds_in"] = lambda: _lds_edge(0, True)             # the widest rows whose tile still fits the LDS budget with stumps
CASES["lds_out"] = lambda: _lds_edge(1, False)


@_case("docs")
def _docs():
    # scored at 1, 63, 64, 65 and 129 documents: a lone one, a tile of documents +- 1, two tiles + 1
    rng = _rng("docs")
    return _finish(rng, mixed_trees(Gen(rng), 37), n=129)


GRID_STRIDE_DOCS = 65536 * DOCS + 65         # more tiles than the tiled kernel's 65 536 blocks, more rows than the generic one's 8192 * 256 threads


@_case("grid_stride")
def _grid_stride():
    rng = _rng("grid_stride")
    trees = [flatten(S(1, 0.25, L(1e8), L(1.0))), flatten(L(-1e8)), flatten(S(1, -0.5, L(3.0), S(1, 1.0, L(0.5), L(-7.0))))]
    pool = np.concatenate([probe_pool(trees), SPECIAL_VALUES])
    rows = np.zeros((GRID_STRIDE_DOCS, 2), np.float32)
    rows[:, 1] = pool[rng.integers(0, len(pool), GRID_STRIDE_DOCS)]
    return _finish(rng, trees, np.array([1.0, 1.0, 0.5], np.float32), rows=rows)


@_case("device")
def _device():
    # predict_device: 13-column rows (52 bytes: a pointer one row in is not 16-byte aligned)
    rng = _rng("device")
    return _finish(rng, mixed_trees(Gen(rng), 41), n=150)


@functools.lru_cache(maxsize=None)
def case(name):
    """the case and its reference scores: built once, shared, never written to"""
    c = CASES[name]()
    want = eval_ensemble_np(c.trees, c.weights, c.rows)
    want.setflags(write=False)
    return c, want
