"""rl_model_predict_shap restated from the definitions of include/rlhip.h -- TEST INFRASTRUCTURE ONLY.  Exact
path-dependent TreeSHAP in its path form: every row meets every leaf of every tree.

    shap(trees, weights, covers, rows, columns, num)     [rows][C + 2]: the requested columns, rest, bias -- the COMPUTED FORM
    brute(trees, weights, covers, rows, columns)         the same from the v_S definition alone: Shapley values by subset enumeration

The computed form is ONE implementation, parametrised by the number type `num`: numpy.float64 (every operation rounded once, in the
stated order, nothing fused, nothing summed by a library routine: the bits the kernel must give) and fractions.Fraction (no rounding:
what the stated operations mean).  It works on all rows at a time -- arrays of float64, or object arrays of Fraction, one element per
row; every array operation is the scalar operation per row, so the order of operations of a row is the stated one.  brute() is
Fraction only.  Trees are the dicts of tests/tree_models.py, covers what contrib_restatement.covers gives.
"""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np

import contrib_restatement as CR
import tree_models as TM

P_LIMIT = 32                                     # kShapP: the distinct features one path may hold
U = 2.0 ** -52
# The worst gap of a row between the f64 run and the exact run, measured on the CPU by tests/test_shap_cpu.py (b).  A row's gap is the
# sum over its slots of |f64 - exact|, so it bounds every slot's error and, by the triangle inequality, the distance of the f64 slots'
# sum from the exact one (local accuracy is held to the same bound); in units of 2^-52 * (sum over the model's trees of sum over leaves
# of |W * out|).  3855.547, on the chain of 30 distinct features, whose unwind cancels the most: twelve of the 52 mantissa bits (a
# single slot of it: 1100 at most among those looked at; on the 257 rows of tests/test_gpu_shap.py the slots' sum is up to 18 033
# from the f64 leaf sum).  The small random models 0.738, count_37 0.090, nodes_81 0.107, nan_leaf 0.170, the depth-30 chains on one
# feature 0.192 and 0.051: nothing to speak of.  BOUND is the worst times 8, for host compilers that order the libm-free operations
# differently.
WORST_MEASURED = 3855.547
BOUND = 8 * WORST_MEASURED * U


def f64(x):
    return np.float64(x)


def frac(x):
    return Fraction(int(x)) if isinstance(x, (int, np.integer)) else Fraction(float(x))


def _arr(num, n, value):
    out = np.empty(n, np.float64 if num is f64 else object)
    out[:] = num(value)
    return out


def ratio(a, b):
    """the cover pair of a split's children under the empty-node rule"""
    a, b = int(a), int(b)
    return (1, 1) if a + b == 0 else (a, b)


def node_values(tree, cover, num):
    """val[j], children first, as contrib_restatement.node_values has them (the f64 run gives the same bits)"""
    val = [None] * len(tree["feature"])
    with np.errstate(all="ignore"):
        for j in range(len(val) - 1, -1, -1):
            if tree["feature"][j] == -1:
                val[j] = num(np.float64(tree["output"][j]))
                continue
            l, r = int(tree["left"][j]), int(tree["right"][j])
            a, b = ratio(cover[l], cover[r])
            val[j] = (num(a) * val[l] + num(b) * val[r]) / num(a + b)
    return val


def leaf_elements(tree, cover, num):
    """per leaf, in the pre-order of the model text: (leaf node, elements); an element is (feature, z, [(threshold, goes left), ...]) --
    the distinct features of the root-to-leaf path in order of first appearance, z the product in root-to-leaf order of the cover
    ratios c[child on the path] / (a + b) of the path's splits on the feature, and those splits' conditions"""
    feat, left, right = tree["feature"], tree["left"], tree["right"]
    parent = {}
    for j in range(len(feat)):
        if feat[j] != -1:
            parent[int(left[j])] = (j, True)
            parent[int(right[j])] = (j, False)
    out = []
    for leaf in range(len(feat)):
        if feat[leaf] != -1:
            continue
        steps, j = [], leaf
        while j in parent:
            p, goes_left = parent[j]
            steps.append((p, goes_left, j))
            j = p
        els = []
        for p, goes_left, child in reversed(steps):
            a, b = ratio(cover[int(left[p])], cover[int(right[p])])
            r = num(a if goes_left else b) / num(a + b)
            f = int(feat[p])
            for e in els:
                if e[0] == f:
                    e[1] = e[1] * r
                    e[2].append((tree["threshold"][p], goes_left))
                    break
            else:
                els.append([f, r, [(tree["threshold"][p], goes_left)]])
        out.append((leaf, els))
    return out


def max_path(trees):
    """rl_model_shap_limits' first value: the longest element list of the model"""
    return max((len(els) for t in trees for _, els in leaf_elements(t, np.zeros(len(t["feature"]), np.uint64), f64)), default=0)


@functools.lru_cache(maxsize=None)
def tables(num):
    """A[l][i] = (i+1)/(l+1), B[l][i] = (l-i)/(l+1), U[l][i] = (l+1)/(i+1), R[l][i] = (l+1)/(l-i) for 0 <= i < l <= P: one division each"""
    A, B, U, R = ({(l, i): fn(l, i) for l in range(1, P_LIMIT + 1) for i in range(l)} for fn in (
        lambda l, i: num(i + 1) / num(l + 1), lambda l, i: num(l - i) / num(l + 1), lambda l, i: num(l + 1) / num(i + 1),
        lambda l, i: num(l + 1) / num(l - i)))
    return A, B, U, R


def agrees(rows, feature, conds):
    """bool [rows]: the row's own decision equals the path's direction at every split of the element.  v = (f < row_stride) ? row[f] : 0;
    `v <= thr` goes left, anything else, a NaN included, goes right"""
    v = rows[:, feature] if feature < rows.shape[1] else np.zeros(len(rows), np.float32)
    ok = np.ones(len(rows), bool)
    with np.errstate(invalid="ignore"):
        for thr, goes_left in conds:
            ok &= (v <= np.float32(thr)) == goes_left
    return ok


def leaf_terms(o_bool, z, num):
    """the (row, leaf) recurrence.  o_bool: d bool arrays [rows]; z: d numbers.  Per element: (tot * (o - z) [rows], skipped [rows])"""
    d, n = len(z), len(o_bool[0]) if o_bool else 0
    A, B, U, R = tables(num)
    zero, one = num(0), num(1)
    o = [np.where(ob, _arr(num, n, 1), _arr(num, n, 0)) for ob in o_bool]
    w = [_arr(num, n, 1)]                                               # 1. start
    for l in range(1, d + 1):                                           # 2. extend
        w.append(_arr(num, n, 0))
        for i in range(l - 1, -1, -1):
            w[i + 1] = w[i + 1] + o[l - 1] * (w[i] * A[l, i])
            w[i] = (z[l - 1] * w[i]) * B[l, i]
    out = []
    for e in range(d):                                                  # 3. unwind
        ze = z[e]
        skipped = np.where(o_bool[e], ze == one, ze == zero)            # o_e == z_e: possible only at 0 and 1
        tot1, nxt = _arr(num, n, 0), w[d]
        for i in range(d - 1, -1, -1):
            tmp = nxt * U[d, i]
            tot1 = tot1 + tmp
            nxt = w[i] - (tmp * ze) * B[d, i]
        tot0 = _arr(num, n, 0)
        if ze != zero:                                                  # (where z_e == 0 every row of this arm is skipped)
            for i in range(d - 1, -1, -1):
                tot0 = tot0 + w[i] * R[d, i]
            tot0 = tot0 / ze
        tot = np.where(o_bool[e], tot1, tot0)
        out.append((tot * (o[e] - ze), skipped))
    return out


def terms(trees, weights, covers, rows, num=f64, abs_leaf=None):
    """what the slots' chains add, in their order and whatever the columns: per tree (W * val[root], [(feature, ((tot * (o - z)) * out) * W
    [rows], skipped [rows]) per leaf and element]).  abs_leaf: a list that receives, per tree, sum over its leaves of |W * out| as a
    float (what the accuracy bound is relative to)"""
    rows = np.asarray(rows, np.float32)
    out_ = []
    with np.errstate(all="ignore"):
        for t, wt, cov in zip(trees, weights, covers):
            W = num(np.float64(np.float32(wt)))
            mine, mag = [], 0.0
            for leaf, els in leaf_elements(t, cov, num):
                out = num(np.float64(t["output"][leaf]))
                mag += abs(float(W) * float(out))
                o_bool = [agrees(rows, f, conds) for f, _, conds in els]
                for (f, _, _), (x, skipped) in zip(els, leaf_terms(o_bool, [e[1] for e in els], num)):
                    mine.append((f, (x * out) * W, skipped))
            out_.append((W * node_values(t, cov, num)[0], mine))
            if abs_leaf is not None:
                abs_leaf.append(mag)
    return out_


def accumulate(terms_, n, columns, num=f64):
    """[n][C + 2]: every slot one serial chain, in tree order, then leaf order, then element order"""
    columns = [int(c) for c in columns]
    C = len(columns)
    slot_of = {f: s for s, f in enumerate(columns)}
    acc = [_arr(num, n, 0) for _ in range(C + 2)]
    with np.errstate(all="ignore"):
        for b, mine in terms_:
            acc[C + 1] = acc[C + 1] + b
            for f, x, skipped in mine:
                s = slot_of.get(f, C)
                acc[s] = np.where(skipped, acc[s], acc[s] + x)
    return np.stack(acc, axis=1) if n else np.zeros((0, C + 2), np.float64 if num is f64 else object)


def shap(trees, weights, covers, rows, columns, num=f64, abs_leaf=None):
    return accumulate(terms(trees, weights, covers, rows, num, abs_leaf), len(rows), columns, num)


# ---- the definition: Shapley values of S -> v_S(root) by enumeration, exact --------------------------------------------------------------
def value_of_set(tree, cover, row, S):
    feat, thr, left, right = tree["feature"], tree["threshold"], tree["left"], tree["right"]

    def rec(j):
        if feat[j] == -1:
            return frac(np.float64(tree["output"][j]))
        f, l, r = int(feat[j]), int(left[j]), int(right[j])
        if f in S:
            v = row[f] if f < len(row) else np.float32(0)
            return rec(l) if v <= thr[j] else rec(r)
        a, b = ratio(cover[l], cover[r])
        return (a * rec(l) + b * rec(r)) / Fraction(a + b)
    return rec(0)


def brute(trees, weights, covers, rows, columns):
    rows = np.asarray(rows, np.float32)
    columns = [int(c) for c in columns]
    C = len(columns)
    slot_of = {f: s for s, f in enumerate(columns)}
    out = np.empty((len(rows), C + 2), object)
    out[:] = Fraction(0)
    with np.errstate(invalid="ignore"):
        for t, wt, cov in zip(trees, weights, covers):
            W = frac(np.float64(np.float32(wt)))
            players = sorted({int(f) for f in t["feature"] if f != -1})
            k = len(players)
            for r, row in enumerate(rows):
                v = {S: value_of_set(t, cov, row, S) for m in range(k + 1) for S in map(frozenset, itertools.combinations(players, m))}
                out[r, C + 1] += W * v[frozenset()]
                for p in players:
                    phi = Fraction(0)
                    for S, vs in v.items():
                        if p not in S:
                            phi += Fraction(math.factorial(len(S)) * math.factorial(k - len(S) - 1), math.factorial(k)) * (v[S | {p}] - vs)
                    out[r, slot_of.get(p, C)] += W * phi
    return out


def as_float(a):
    return np.array([[float(x) for x in r] for r in a], np.float64).reshape(np.shape(a))


# ---- the LDS plan of k_model_shap (rl_shap_host.h) ----------------------------------------------------------------------------------------
LDS_BUDGET = 160 * 1024


def slot_limit(wd, docs=64):
    """shap_slot_limit: the accumulators [slots][docs + 1] f64 a block holds beside w[wd][docs] f64, wd = the model's longest path + 1"""
    return max(0, LDS_BUDGET - wd * docs * 8) // ((docs + 1) * 8)


# ---- the models the tests share -----------------------------------------------------------------------------------------------------------
def and_tree():
    """feature 1 at the root with left leaf 0; the right child splits on feature 2 with leaves 0 and 1; covers 2 | 1, 1"""
    trees = [TM.flatten(TM.S(1, 0.0, TM.L(0.0), TM.S(2, 0.0, TM.L(0.0), TM.L(1.0))))]
    bg = np.array([[0, -1.0, -1.0], [0, -1.0, 1.0], [0, 1.0, -1.0], [0, 1.0, 1.0]], np.float32)
    return trees, np.array([1.0], np.float32), bg


def distinct_chain(depth=30, seed=12, first=1):
    """`depth` splits on `depth` DISTINCT features first .. first + depth - 1, every split's left child the next split; thresholds
    from the top of TM.GRID, so a grid background thins out slowly down the chain and the deep covers are not all zero"""
    rng = np.random.default_rng(seed)
    out = lambda: np.float32(rng.standard_normal())                    # noqa: E731
    nd = TM.L(out())
    for f in range(first + depth - 1, first - 1, -1):
        nd = TM.S(f, np.float32(rng.choice(TM.GRID[56:64])), nd, TM.L(out()))
    return [TM.flatten(nd)], np.array([0.7], np.float32)
