"""rl_model_predict_interactions restated from the definitions of include/rlhip.h -- TEST INFRASTRUCTURE ONLY.  SHAP
interaction values of a tree model in the path form of tests/shap_restatement.py: per leaf and conditioned element the recurrence of
exact TreeSHAP runs on the leaf's element list without that element.

    interactions(trees, weights, covers, rows, columns, num)     [rows][C + 2][C + 2] -- the COMPUTED FORM
    brute(trees, weights, covers, rows, columns)                 the same from the v_S definition alone: the Shapley interaction index
                                                                 by subset enumeration, the diagonal from shap_restatement.brute

The computed form is ONE implementation, parametrised by the number type as shap_restatement's is (numpy.float64: the bits the kernel
must give; fractions.Fraction: what the stated operations mean), and it reuses leaf_elements, leaf_terms, tables and shap from there.
Cell [i][j], i != j, both <= C, has i as the CONDITIONED slot and j as the ATTRIBUTED slot.
"""
import itertools
import math
from fractions import Fraction

import numpy as np

import shap_restatement as SR

f64, frac, U = SR.f64, SR.frac, SR.U
# The worst values measured on the CPU by tests/test_interact_cpu.py (b), the f64 run against its own Fraction run, in the unit of
# shap_restatement.WORST_MEASURED: 2^-52 * (sum over the model's trees of sum over leaves of |W * out|).
#   WORST_GAP    a row's gap is the sum over ALL cells of its matrix of |f64 - exact|, so it bounds every cell's error, every row sum's
#                distance from the exact SHAP value and the cells' sum's distance from the exact leaf sum.
#   WORST_ASYM   the largest |out[i][j] - out[j][i]| of a row: two f64 chains of one exact value.
# Both come from the chain of 30 distinct features (the unwind cancels, and here every leaf runs it once per conditioned element):
# the gap 20279.924 on a row that follows the chain far down and then leaves it, among four of test_shap_cpu.named_case's twelve rows
# (all twelve were looked at once: the others' gaps are 0.5 to 4 059); the asymmetry 453.336 on the 257 rows tests/test_gpu_interact.py
# walks, which needs no exact run (291.683 among the four).  The others, gap / asymmetry: the small random models 0.782 / 0.045,
# count_37 0.126 / 0.004, nodes_81 0.236 / 0.012, nan_leaf (its trees with finite leaves) 0.261 / 0.006, the depth-30 chains on one
# feature 0.192 / 0 and 0.051 / 0 (one element a leaf: no pair at all, the gap is the diagonal's, which is SHAP's).
# The bounds are the worst times 8, shap_restatement's margin, for host compilers that order the libm-free operations differently.
WORST_GAP = 20279.924
WORST_ASYM = 453.336
BOUND_GAP = 8 * WORST_GAP * U
BOUND_ASYM = 8 * WORST_ASYM * U


def pair_terms(trees, weights, covers, rows, num=f64, abs_leaf=None):
    """what the off-diagonal cells' chains add, in their order and whatever the columns: per tree the list, in leaf order, then
    conditioned element c in element order, then attributed element e in element order, of (feature_c, feature_e, x [rows], skipped
    [rows]) with x = (((tot * (o_e - z_e)) * out) * ((o_c - z_c) * 0.5)) * W, tot from the recurrence on the leaf's elements without c,
    and skipped where o_c == z_c or o_e == z_e.  abs_leaf as in shap_restatement.terms"""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    half = num(0.5)
    out_ = []
    with np.errstate(all="ignore"):
        for t, wt, cov in zip(trees, weights, covers):
            W = num(np.float64(np.float32(wt)))
            mine, mag = [], 0.0
            for leaf, els in SR.leaf_elements(t, cov, num):
                out = num(np.float64(t["output"][leaf]))
                mag += abs(float(W) * float(out))
                d = len(els)
                if d < 2:                                            # a leaf with one element, and a single leaf, add nothing
                    continue
                o_bool = [SR.agrees(rows, f, conds) for f, _, conds in els]
                z = [e[1] for e in els]
                for c in range(d):
                    zc = z[c]
                    oc = np.where(o_bool[c], SR._arr(num, n, 1), SR._arr(num, n, 0))
                    skip_c = np.where(o_bool[c], zc == num(1), zc == num(0))
                    hc = (oc - zc) * half
                    keep = [e for e in range(d) if e != c]           # the reduced list, in order, of length d - 1
                    red = SR.leaf_terms([o_bool[e] for e in keep], [z[e] for e in keep], num)
                    for e, (x, skipped) in zip(keep, red):
                        x = x * out
                        x = x * hc
                        x = x * W
                        mine.append((els[c][0], els[e][0], x, skipped | skip_c))
            out_.append(mine)
            if abs_leaf is not None:
                abs_leaf.append(mag)
    return out_


def assemble(pairs, phi, n, columns, num=f64):
    """[n][C + 2][C + 2] from the pair terms and the SHAP values phi [n][C + 2] of the same columns: every off-diagonal cell one serial
    chain from +0.0 (pairs whose two features share a slot are not walked), the diagonal r = phi_i, then r = r - out[i][j] for j = 0 .. C
    ascending, j != i; the bias cell phi's bias slot; the rest of row and column C + 1 is +0.0"""
    columns = [int(c) for c in columns]
    C = len(columns)
    S = C + 2
    slot_of = {f: s for s, f in enumerate(columns)}
    cell = [[SR._arr(num, n, 0) for _ in range(S)] for _ in range(S)]
    with np.errstate(all="ignore"):
        for mine in pairs:
            for fc, fe, x, skipped in mine:
                i, j = slot_of.get(fc, C), slot_of.get(fe, C)
                if i == j:
                    continue
                cell[i][j] = np.where(skipped, cell[i][j], cell[i][j] + x)
        for i in range(C + 1):
            r = phi[:, i] if n else SR._arr(num, 0, 0)
            for j in range(C + 1):
                if j != i:
                    r = r - cell[i][j]
            cell[i][i] = r
        if n:
            cell[C + 1][C + 1] = phi[:, C + 1]
    if not n:
        return np.zeros((0, S, S), np.float64 if num is f64 else object)
    return np.stack([np.stack(r, axis=1) for r in cell], axis=1)


def interactions(trees, weights, covers, rows, columns, num=f64, abs_leaf=None):
    rows = np.asarray(rows, np.float32)
    phi = SR.shap(trees, weights, covers, rows, columns, num)
    return assemble(pair_terms(trees, weights, covers, rows, num, abs_leaf), phi, len(rows), columns, num)


# ---- the definition: the Shapley interaction index of S -> v_S(root) by enumeration, exact ------------------------------------------------
def brute(trees, weights, covers, rows, columns):
    """off-diagonal: sum over S in N \\ {p, q} of |S|! (k - |S| - 2)! / (2 (k - 1)!) (v_{S+p+q} - v_{S+p} - v_{S+q} + v_S), added into
    [slot_p][slot_q] unless the two share a slot; the diagonal is shap_restatement.brute's value less the row's other cells (in exact
    arithmetic the order does not matter); the bias cell its bias slot"""
    rows = np.asarray(rows, np.float32)
    columns = [int(c) for c in columns]
    C = len(columns)
    S_ = C + 2
    slot_of = {f: s for s, f in enumerate(columns)}
    out = np.empty((len(rows), S_, S_), object)
    out[:] = Fraction(0)
    with np.errstate(invalid="ignore"):
        for t, wt, cov in zip(trees, weights, covers):
            W = frac(np.float64(np.float32(wt)))
            players = sorted({int(f) for f in t["feature"] if f != -1})
            k = len(players)
            for r, row in enumerate(rows):
                v = {S: SR.value_of_set(t, cov, row, S) for m in range(k + 1) for S in map(frozenset, itertools.combinations(players, m))}
                for p in players:
                    for q in players:
                        i, j = slot_of.get(p, C), slot_of.get(q, C)
                        if p == q or i == j:
                            continue
                        tot = Fraction(0)
                        for S, vs in v.items():
                            if p in S or q in S:
                                continue
                            tot += Fraction(math.factorial(len(S)) * math.factorial(k - len(S) - 2), 2 * math.factorial(k - 1)) * (
                                v[S | {p, q}] - v[S | {p}] - v[S | {q}] + vs)
                        out[r, i, j] += W * tot
    phi = SR.brute(trees, weights, covers, rows, columns)
    for r in range(len(rows)):
        for i in range(C + 1):
            out[r, i, i] = phi[r, i] - sum((out[r, i, j] for j in range(C + 1) if j != i), Fraction(0))
        out[r, C + 1, C + 1] = phi[r, C + 1]
    return out


def as_float(a):
    return np.array([float(x) for x in np.ravel(a)], np.float64).reshape(np.shape(a))


# ---- the LDS plan of k_model_interact and the row-chunk rule (rl_interact_host.h) ---------------------------------------------------------
def slot_limit(wr, docs=64):
    """interact_slot_limit: the accumulators [attributed slots][docs + 1] f64 a block holds beside w[wr][docs] f64, wr = the model's
    longest path (one row less than k_model_shap's), at least 1"""
    return max(0, SR.LDS_BUDGET - wr * docs * 8) // ((docs + 1) * 8)


def chunk_rows(n_docs, row_stride, C, scratch_bytes=0):
    """interact_chunk_rows: per row the row itself, 8 (C + 2)^2 bytes of result and 8 (C + 2) bytes of SHAP values within scratch_bytes
    (0: 256 MiB); at least one row"""
    budget = scratch_bytes if scratch_bytes > 0 else 256 << 20
    return max(1, min(n_docs, budget // (4 * row_stride + 8 * (C + 2) ** 2 + 8 * (C + 2))))
