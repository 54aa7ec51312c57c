"""rl_model_predict_shap_background restated from the definitions of include/rlhip.h -- TEST INFRASTRUCTURE ONLY.

    interv(trees, weights, rows, bg, columns, num)       [rows][C + 2]: the requested columns, rest, bias -- the COMPUTED FORM
    brute(trees, weights, rows, bg, columns)             the same from the MEANING alone: Shapley values of the hybrid-row game by subsets

The computed form is ONE implementation, parametrised by the number type `num` as tests/shap_restatement.py's is: numpy.float64 (the bits
the kernel must give) and fractions.Fraction (what the operations mean).  It works on all rows at a time, the background rows one after
the other, so the order of operations of a row is the stated one.  brute() is Fraction only.  Trees are the dicts of tests/tree_models.py.
"""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np

import contrib_restatement as CR
import shap_restatement as SR

f64, frac, P_LIMIT, U = SR.f64, SR.frac, SR.P_LIMIT, SR.U
# The worst gap of a row between the f64 run and the exact run, measured on the CPU by tests/test_interv_cpu.py (c): the sum over the
# row's slots of |f64 - exact| in units of 2^-52 * (sum over trees and leaves of |W * out|).  The small random models 0.266, count_37
# 0.048, nodes_81 0.071, nan_leaf 0.100, chain_left 0.028, chain_right 0.044, distinct_30 0.059.  BOUND is the worst times 8.
WORST_MEASURED = 0.266
BOUND = 8 * WORST_MEASURED * U


@functools.lru_cache(maxsize=None)
def table(num):
    """T[p][q] = 1 / (p C(p+q, p)) for 1 <= p, 0 <= q, p + q <= P: an exact integer denominator, one division; the other cells 0"""
    T = np.empty((P_LIMIT + 1, P_LIMIT + 1), np.float64 if num is f64 else object)
    T[:] = num(0)
    for p in range(1, P_LIMIT + 1):
        for q in range(P_LIMIT + 1 - p):
            T[p, q] = num(1) / num(p * math.comb(p + q, p))
    return T


def elements(tree):
    """per leaf, in the pre-order of the model text: (leaf node, [(feature, conditions)]); no cover is involved"""
    return [(leaf, [(f, conds) for f, _, conds in els]) for leaf, els in SR.leaf_elements(tree, np.zeros(len(tree["feature"]), np.uint64), f64)]


def terms(trees, weights, rows, bg, num=f64, abs_leaf=None):
    """what the slots' chains add, in their order and whatever the columns: (per tree [(feature, ((s_e * out) * W) [rows], touched [rows])
    per leaf and element], the bias before its division).  abs_leaf as shap_restatement.terms has it"""
    rows, bg = np.asarray(rows, np.float32), np.asarray(bg, np.float32)
    n, B, T = len(rows), len(bg), table(num)
    out_, bias = [], num(0)
    with np.errstate(all="ignore"):
        for t, wt in zip(trees, weights):
            W = num(np.float64(np.float32(wt)))
            mine, mag, zout = [], 0.0, [None] * B
            for leaf, els in elements(t):
                out = num(np.float64(t["output"][leaf]))
                mag += abs(float(W) * float(out))
                d = len(els)
                ox = np.array([SR.agrees(rows, f, conds) for f, conds in els], bool).reshape(d, n)      # bit e of xm, per row
                oz = np.array([SR.agrees(bg, f, conds) for f, conds in els], bool).reshape(d, B)        # bit e of zm, per background row
                for z in np.flatnonzero(oz.all(axis=0)):                # zm == full: the leaf z ends in
                    zout[z] = out
                zc = oz.T[:, :, None]                                   # [B][d][1] against ox [d][n]: what follows is per (z, row)
                plus, minus = ox[None] & ~zc, ~ox[None] & zc            # xm & ~zm, ~xm & zm
                a, b = plus.sum(axis=1), minus.sum(axis=1)
                active = (ox[None] | zc).all(axis=1) & (a + b > 0)      # z meets the leaf, and a + b > 0
                plus, minus = plus & active[:, None], minus & active[:, None]
                tp, tn = T[a, b], T[b, a]
                s = SR._arr(num, d * n, 0).reshape(d, n)
                for z in np.flatnonzero(active.any(axis=1)):            # the chains themselves: z after z
                    s = np.where(plus[z], s + tp[z], s)
                    s = np.where(minus[z], s - tn[z], s)
                touched = (plus | minus).any(axis=0)
                for e, (f, _) in enumerate(els):
                    mine.append((f, (s[e] * out) * W, touched[e]))
            m = num(0)
            for z in range(B):
                m = m + zout[z]
            bias = bias + m * W
            out_.append(mine)
            if abs_leaf is not None:
                abs_leaf.append(mag)
    return out_, bias, B


def accumulate(terms_, n, columns, num=f64):
    """[n][C + 2]: every slot one serial chain, in tree order, then leaf order, then element order, divided by B at the end"""
    per_tree, bias, B = terms_
    columns = [int(c) for c in columns]
    C = len(columns)
    slot_of = {f: s for s, f in enumerate(columns)}
    acc = [SR._arr(num, n, 0) for _ in range(C + 1)]
    with np.errstate(all="ignore"):
        for mine in per_tree:
            for f, x, touched in mine:
                s = slot_of.get(f, C)
                acc[s] = np.where(touched, acc[s] + x, acc[s])
        acc = [a / num(B) for a in acc] + [np.full(n, bias / num(B), acc[0].dtype)]  # the same bits in every row
    return np.stack(acc, axis=1) if n else np.zeros((0, C + 2), np.float64 if num is f64 else object)


def interv(trees, weights, rows, bg, columns, num=f64, abs_leaf=None):
    return accumulate(terms(trees, weights, rows, bg, num, abs_leaf), len(rows), columns, num)


# ---- the meaning: Shapley values of S -> v_S on hybrid rows, by enumeration, exact -------------------------------------------------------
def brute(trees, weights, rows, bg, columns):
    rows, bg = np.asarray(rows, np.float32), np.asarray(bg, np.float32)
    columns = [int(c) for c in columns]
    C = len(columns)
    slot_of = {f: s for s, f in enumerate(columns)}
    width = max(rows.shape[1], bg.shape[1])
    pad = lambda r: np.concatenate([r, np.zeros(width - len(r), np.float32)])      # noqa: E731  (a column beyond the stride reads 0)
    out = np.empty((len(rows), C + 2), object)
    out[:] = Fraction(0)
    with np.errstate(invalid="ignore"):
        for t, wt in zip(trees, weights):
            W = frac(np.float64(np.float32(wt)))
            players = sorted({int(f) for f in t["feature"] if f != -1})
            k = len(players)
            for r, x in enumerate(rows):
                for z in bg:
                    x_, z_ = pad(x), pad(z)

                    def value(S):
                        h = z_.copy()
                        for f in S:
                            if f < width:
                                h[f] = x_[f]
                        return frac(np.float64(t["output"][CR.walk(t, h)[-1]]))
                    v = {S: value(S) for m in range(k + 1) for S in map(frozenset, itertools.combinations(players, m))}
                    out[r, C + 1] += W * v[frozenset()]
                    for p in players:
                        phi = Fraction(0)
                        for S, vs in v.items():
                            if p not in S:
                                phi += Fraction(math.factorial(len(S)) * math.factorial(k - len(S) - 1), math.factorial(k)) * (v[S | {p}] - vs)
                        out[r, slot_of.get(p, C)] += W * phi
    return out / Fraction(len(bg))
