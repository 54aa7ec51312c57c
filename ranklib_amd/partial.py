"""python -m ranklib_amd.partial: partial dependence and ICE curves of a model on a file -- how the score moves as one
feature moves: set the feature to a grid value in every document, score the file again, average.  The mean over the documents is the
partial-dependence (PD) value of the cell, the per-document scores behind it are its ICE curves ("individual conditional expectation").
A LambdaMART / MART model takes every (feature, grid value) cell in one GPU pass over the file (LambdaMART.partialDependence,
rl_model_predict_partial); every other model scores one substituted copy per cell (Ranker.partialDependence).  Both give the same bits.

  -load model            the model (one)
  -test file             the file to evaluate on (one)
  -feature file          the features to vary, one id per line as RankLib's -feature files (default: the model's own, ascending)
  -grid n|thresholds     n: n order statistics of the feature's distinct values in the file (default 20); thresholds: the model's own
                         thresholds of the feature and one value beyond the last -- the whole curve of a tree model, which is piecewise
                         constant (tree models only)
  -norm, -qrel, -gmax, -missingZero, -hr, -device   as in ranklib_amd.importance: the file is prepared by Evaluator.readTestFile
  -out tsv               one line per cell: feature <TAB> value <TAB> mean <TAB> centred mean <TAB> rms shift
  -ice file              one line per cell: feature <TAB> value <TAB> the score of every document in file order
  -pairs file            two-feature partial dependence as well: one pair of feature ids "a b" per line.  The surface over
                         both grids at once, for a LambdaMART / MART model in one GPU pass (rl_model_predict_partial2)
  -grid2 n|thresholds    the grid of either axis of a pair, as -grid (default 10)
  -out2 tsv              one line per cell: a <TAB> b <TAB> value_a <TAB> value_b <TAB> mean <TAB> centred mean <TAB> rms shift, sorted by
                         ascending pair and values, and one further line per pair: a <TAB> b <TAB> h2 <TAB> its value
  -ice2 file             one line per cell: a <TAB> b <TAB> value_a <TAB> value_b <TAB> the score of every document in file order
  -ale tsv               accumulated local effects: one line per edge: feature <TAB> edge <TAB> ale <TAB> local effect of
                         the interval ending there <TAB> count.  For a LambdaMART / MART model in one GPU pass (rl_model_predict_ale).
                         It may stand without -out: then only the accumulated local effects are computed
  -intervals n           the intervals of a feature, 1 .. 255: n + 1 order statistics of its distinct values in the file are the edges
                         (default 20); a feature with fewer than two distinct values has no interval and is left out
  -local file            one line per feature and document: feature <TAB> document <TAB> interval <TAB> lo <TAB> hi
  -ale2 tsv              second-order accumulated local effects of the pairs of -pairs: one line per pair of edges:
                         a <TAB> b <TAB> edge_a <TAB> edge_b <TAB> ale <TAB> local effect of the cell ending there <TAB> count.  A count
                         of 0 away from the first edges is an empty cell: the surface there is an extrapolation.  For a LambdaMART /
                         MART model in one GPU pass (rl_model_predict_ale2).  It may stand without -out and -out2
  -intervals2 n          the intervals of either axis of a pair, 1 .. 64 (default 10), edges as -intervals; a pair with a feature of
                         fewer than two distinct values is left out
  -local2 file           one line per pair and document: a <TAB> b <TAB> document <TAB> cell <TAB> s00 <TAB> s01 <TAB> s10 <TAB> s11

Accumulated local effects answer the same question as partial dependence without leaving the data: a document is moved only between
the two edges of the interval its own value lies in (0: it lies outside the edges and is not moved), lo and hi are its scores at the
lower and the upper edge, the local effect of an interval is the mean of hi - lo over its documents, the curve is the running sum of the
local effects from 0 at the first edge, centred as ALEPlot does it: minus sum n_k (ale(z_{k-1}) + ale(z_k)) / 2 / sum n_k.  Where the
features are correlated -- LETOR's are -- partial dependence averages the model over rows that cannot occur; this does not.

The second-order effect of a pair is what the two features do together beyond what either does alone.  A document is moved between the
four corners of the cell its own two values lie in (cell -1: it lies outside the edges of either axis and is not moved); s00 .. s11
are its scores there (first digit a, second b; 0 the lower edge), d = (s11 - s01) - (s10 - s00), the local effect of a cell is the mean
of d over its documents (0 in an empty cell).  The surface is ALEPlot's: the double running sum of the local effects over both axes
from a zero first row and column; minus its own two main effects -- per interval of a the count-weighted mean over the cells of that
row of the surface's step across the interval, averaged over the cell's two b edges, accumulated along a; b alike --; minus the
count-weighted mean over all cells of the mean of the cell's four corners.

Lines are sorted by ascending feature, then ascending value; the numbers are printed as Double.toString.  The sums behind a mean take
one fixed order (include/rlhip.h): partial p is the serial f64 chain over the documents [256 p, 256 p + 256), the total the serial chain
over the partials.  centred mean = mean - the base mean (the same sum over the unsubstituted scores); rms shift = sqrt of the mean
squared move of a document away from its own score: its spread over a feature's cells shows how much the feature matters at all.

h2 of a pair is Friedman and Popescu's interaction strength on the grid: with F_ab the pair's mean surface, F_a and F_b the one-feature
curves on the same grids, each centred by its unweighted mean over its cells, h2 = sum (F_ab - F_a - F_b)^2 / sum F_ab^2 over the cells
(0 where the denominator is 0).  The original weights every term by the data: it evaluates the functions at the documents' own values.
Here uniform weights over the grid cells stand in for the data distribution.  That is reasonable because the grids are order statistics
of the file's distinct values: the cells are spread the way the data is rather than evenly over its range.  With -grid2 thresholds the
cells follow the model, not the data, and h2 says only how far the surface is from additive on those cells.
"""
import collections
import logging
import re
import sys

import numpy as np

from ._native import ALE2_MAX_CELLS, ALE2_SUM_SUPER, ALE_MAX_INTERVALS, PARTIAL_SUM_BLOCK, RankLibError

logger = logging.getLogger("ranklib_amd")

Partial = collections.namedtuple("Partial", "features grids mean centred rms base_mean base ice")
Partial.__doc__ = """features [F], ascending; per feature c: grids[c] f32 [G_c], mean[c] f64 [G_c] (the PD values), centred[c] = mean[c] -
base_mean, rms[c] = sqrt(shift2); base_mean; base f64 [n_docs], the unsubstituted scores; ice: None, or per feature f64 [G_c][n_docs]"""

Partial2 = collections.namedtuple("Partial2", "pairs grids mean centred rms h2 base_mean base ice")
Partial2.__doc__ = """pairs [(a, b)] as asked; per pair p: grids[p] = (f32 [ga], f32 [gb]), mean[p] f64 [ga][gb] (the PD surface), centred[p] =
mean[p] - base_mean, rms[p] = sqrt(shift2), h2[p] the interaction strength on the grid (the module's text); base_mean; base f64 [n_docs];
ice: None, or per pair f64 [ga][gb][n_docs]"""


def fixed_order_sums(scores, base):
    """(S1, S2) of one cell in the fixed order: scores and base f64 [n_docs].  A NumPy statement of it: cumsum is a serial chain, a row
    of the padded matrix one partial; the leading +0.0 is the chain's start and the +0.0 padding changes no sum that started there."""
    x = np.asarray(scores, np.float64)
    with np.errstate(all="ignore"):
        d = x - np.asarray(base, np.float64)
        q = d * d
        out = []
        for v in (x, q):
            parts = -(-len(v) // PARTIAL_SUM_BLOCK)
            pad = np.zeros(parts * PARTIAL_SUM_BLOCK, np.float64)
            pad[:len(v)] = v
            m = np.zeros((parts, PARTIAL_SUM_BLOCK + 1), np.float64)
            m[:, 1:] = pad.reshape(parts, PARTIAL_SUM_BLOCK)
            p = np.cumsum(m, axis=1)[:, -1]
            out.append(float(np.cumsum(np.concatenate([[0.0], p]))[-1]))
    return out[0], out[1]


Ale = collections.namedtuple("Ale", "features edges ale effect count centre lo hi interval")
Ale.__doc__ = """features [F], ascending (a feature without two distinct values in the file is left out); per feature c: edges[c] f32
[K_c + 1], ale[c] f64 [K_c + 1] the centred curve at the edges, effect[c] f64 [K_c + 1] the local effect of the interval ending at the
edge (0 at the first), count[c] int64 [K_c + 1] its documents (0 at the first), centre[c] what was subtracted; lo, hi, interval: None, or
per feature f64 [n_docs], f64 [n_docs] and int32 [n_docs] (0: the document is outside the edges)"""


def ale_intervals(values, edges):
    """int32 [n]: the interval of every own value (f32) under the strictly ascending edges z_0 < ... < z_K -- 1 + #{j in 1 .. K-1 :
    z_j < v} where z_0 <= v <= z_K, else 0 (below, above, NaN)"""
    v, z = np.asarray(values, np.float32), np.asarray(edges, np.float32)
    with np.errstate(invalid="ignore"):
        inside = (z[0] <= v) & (v <= z[-1])
    return np.where(inside, 1 + np.searchsorted(z[1:-1], np.where(inside, v, z[0]), side="left"), 0).astype(np.int32)


def ale_cell_sums(lo, hi, interval, K):
    """(int64 count [K], f64 S [K]) of one column in the fixed order of include/rlhip.h: lo and hi f64 [n_docs], interval int32 [n_docs].
    A NumPy statement of it: a document of another cell stands as +0.0, which changes no chain that started from +0.0 (such a chain
    is never -0.0); cumsum is a serial chain, a row of the padded matrix one partial."""
    iv = np.asarray(interval)
    with np.errstate(all="ignore"):
        d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    parts = -(-len(d) // PARTIAL_SUM_BLOCK)
    count, total = np.zeros(K, np.int64), np.zeros(K, np.float64)
    for k in range(1, K + 1):
        member = iv == k
        count[k - 1] = int(member.sum())
        pad = np.zeros(parts * PARTIAL_SUM_BLOCK, np.float64)
        pad[:len(d)] = np.where(member, d, 0.0)
        m = np.zeros((parts, PARTIAL_SUM_BLOCK + 1), np.float64)
        m[:, 1:] = pad.reshape(parts, PARTIAL_SUM_BLOCK)
        with np.errstate(all="ignore"):
            total[k - 1] = _serial(np.cumsum(m, axis=1)[:, -1])
    return count, total


def ale_curve(count, total):
    """(ale f64 [K + 1] centred, effect f64 [K + 1], centre) of one column's cells: effect_k = S_k / n_k (0 where n_k == 0, and at the
    first edge), the curve their serial chain from 0 at z_0, centred as ALEPlot does it: minus the serial chain of n_k (ale(z_{k-1}) +
    ale(z_k)) / 2 over k, divided by the sum of the n_k (0 where no document is inside)"""
    n = np.asarray(count, np.int64)
    with np.errstate(all="ignore"):
        effect = np.concatenate([[0.0], np.where(n > 0, np.asarray(total, np.float64) / np.maximum(n, 1), 0.0)])
        curve = np.cumsum(effect)
        inside = int(n.sum())
        centre = _serial(n.astype(np.float64) * ((curve[:-1] + curve[1:]) / 2.0)) / float(inside) if inside else 0.0
        return curve - centre, effect, centre


def summarize_ale(features, edges, counts, totals, lo=None, hi=None, interval=None):
    """Ale of per-cell results: per feature count int64 [K_c] and total f64 [K_c]"""
    curves = [ale_curve(n, s) for n, s in zip(counts, totals)]
    return Ale([int(f) for f in features], [np.asarray(e, np.float32) for e in edges], [c[0] for c in curves], [c[1] for c in curves],
               [np.concatenate([[0], np.asarray(n, np.int64)]) for n in counts], [c[2] for c in curves], lo, hi, interval)


def ale_edges(samples, features, intervals):
    """(the features that have an interval, their edges): order_statistics(values, intervals + 1) of the feature's values in samples; a
    feature with fewer than two distinct values there has no interval, is logged and left out"""
    n = int(intervals)
    if not 1 <= n <= ALE_MAX_INTERVALS:
        raise RankLibError("rlhip: -intervals must be 1 .. %d (got %d)" % (ALE_MAX_INTERVALS, n))
    kept, edges = [], []
    for f in features:
        z = order_statistics([dp.fVals[f] if f < len(dp.fVals) else np.nan for rl in samples for dp in rl.rl], n + 1)
        if len(z) < 2:
            logger.info("Feature %d has fewer than two distinct values in the file: no interval, left out", f)
            continue
        kept.append(f)
        edges.append(z)
    return kept, edges


Ale2 = collections.namedtuple("Ale2", "pairs edges ale effect count centre corner cell")
Ale2.__doc__ = """pairs [(a, b)] as asked (a pair with a feature of fewer than two distinct values in the file is left out); per pair p:
edges[p] = (f32 [Ka + 1], f32 [Kb + 1]), ale[p] f64 [Ka + 1][Kb + 1] the centred second-order surface at the edges, effect[p] f64
[Ka][Kb] the local effect of every cell (0 where it is empty), count[p] int64 [Ka][Kb], centre[p] what was subtracted last; corner,
cell: None, or per pair f64 [4][n_docs] (slot 2 ua + ub) and int32 [n_docs] ((k - 1) Kb + l - 1; -1: outside)"""
ALE2_MAX_INTERVALS = int(ALE2_MAX_CELLS ** 0.5)               # of either axis, where both take the same count


def ale2_cell_sums(d, cell, cells):
    """(int64 count [cells], f64 S [cells]) of one pair in the three-level fixed order of include/rlhip.h: d f64 [n_docs], cell int32
    [n_docs] (-1: outside).  A NumPy statement of it, as ale_cell_sums: a row of the padded matrix is one partial, a row of the padded
    partials one super-partial, every chain starts from +0.0 and a +0.0 term changes none."""
    d, cell = np.asarray(d, np.float64), np.asarray(cell)
    parts = -(-len(d) // PARTIAL_SUM_BLOCK)
    supers = -(-parts // ALE2_SUM_SUPER)
    count, total = np.zeros(cells, np.int64), np.zeros(cells, np.float64)
    for c in np.unique(cell[cell >= 0]):
        member = cell == c
        count[c] = int(member.sum())
        pad = np.zeros(supers * ALE2_SUM_SUPER * PARTIAL_SUM_BLOCK, np.float64)
        pad[:len(d)] = np.where(member, d, 0.0)
        with np.errstate(all="ignore"):
            for width in (PARTIAL_SUM_BLOCK, ALE2_SUM_SUPER):
                m = np.zeros((len(pad) // width, width + 1), np.float64)
                m[:, 1:] = pad.reshape(-1, width)
                pad = np.cumsum(m, axis=1)[:, -1]
            total[c] = _serial(pad)
    return count, total


def ale2_surface(count, total):
    """(ale f64 [Ka + 1][Kb + 1] centred, effect f64 [Ka][Kb], centre) of one pair's cells, count and total [Ka][Kb]: ALEPlot's rule, the
    module's text.  cumsum along a, then along b; the sums over a row, a column and all cells are NumPy's."""
    n = np.asarray(count, np.int64)
    b = n.astype(np.float64)
    with np.errstate(all="ignore"):
        effect = np.where(n > 0, np.asarray(total, np.float64) / np.maximum(n, 1), 0.0)
        acc = np.zeros((n.shape[0] + 1, n.shape[1] + 1), np.float64)
        acc[1:, 1:] = np.cumsum(np.cumsum(effect, axis=0), axis=1)
        da, db = acc[1:, :] - acc[:-1, :], acc[:, 1:] - acc[:, :-1]
        rows, cols = b.sum(axis=1), b.sum(axis=0)
        ma = np.where(rows > 0, (b * ((da[:, :-1] + da[:, 1:]) / 2.0)).sum(axis=1) / np.maximum(rows, 1.0), 0.0)
        mb = np.where(cols > 0, (b * ((db[:-1, :] + db[1:, :]) / 2.0)).sum(axis=0) / np.maximum(cols, 1.0), 0.0)
        surf = acc - np.concatenate([[0.0], np.cumsum(ma)])[:, None] - np.concatenate([[0.0], np.cumsum(mb)])[None, :]
        inside = float(b.sum())
        four = (surf[:-1, :-1] + surf[:-1, 1:] + surf[1:, :-1] + surf[1:, 1:]) / 4.0
        centre = float((b * four).sum()) / inside if inside else 0.0
        return surf - centre, effect, centre


def summarize_ale2(pairs, edges, counts, totals, corner=None, cell=None):
    """Ale2 of per-cell results: per pair count int64 [Ka * Kb] and total f64 [Ka * Kb], row-major"""
    edges = [(np.asarray(za, np.float32), np.asarray(zb, np.float32)) for za, zb in edges]
    shape = [(len(za) - 1, len(zb) - 1) for za, zb in edges]
    counts = [np.asarray(n, np.int64).reshape(sh) for n, sh in zip(counts, shape)]
    surfs = [ale2_surface(n, np.asarray(s, np.float64).reshape(sh)) for n, s, sh in zip(counts, totals, shape)]
    return Ale2([(int(a), int(b)) for a, b in pairs], edges, [s[0] for s in surfs], [s[1] for s in surfs], counts, [s[2] for s in surfs], corner, cell)


def ale2_edges(samples, pairs, intervals):
    """(the pairs both of whose features have an interval, their (edges_a, edges_b)): ale_edges per feature; the other pairs are left out"""
    n = int(intervals)
    if not 1 <= n <= ALE2_MAX_INTERVALS:
        raise RankLibError("rlhip: -intervals2 must be 1 .. %d (got %d)" % (ALE2_MAX_INTERVALS, n))
    feats, zs = ale_edges(samples, sorted({f for pr in pairs for f in pr}), n)
    z = dict(zip(feats, zs))
    kept = [(a, b) for a, b in pairs if a in z and b in z]
    return kept, [(z[a], z[b]) for a, b in kept]


def ale2_lines(result):
    """the -ale2 lines: ascending pair, then ascending edges; a pair asked twice is written once"""
    from .learning import java_double_str
    d = lambda x: java_double_str(float(x))      # noqa: E731
    first = {pr: p for p, pr in reversed(list(enumerate(result.pairs)))}
    out = []
    for (a, b), p in sorted(first.items()):
        za, zb = result.edges[p]
        out += ["%d\t%d\t%s\t%s\t%s\t%s\t%d" % (a, b, d(za[k]), d(zb[l]), d(result.ale[p][k, l]), d(result.effect[p][k - 1, l - 1] if k and l else 0.0),
                                                int(result.count[p][k - 1, l - 1]) if k and l else 0) for k in range(len(za)) for l in range(len(zb))]
    return out


def local2_lines(result):
    """the -local2 lines: a <TAB> b <TAB> document (from 0, file order) <TAB> cell <TAB> s00 <TAB> s01 <TAB> s10 <TAB> s11"""
    from .learning import java_double_str
    d = lambda x: java_double_str(float(x))      # noqa: E731
    return ["%d\t%d\t%d\t%d\t%s" % (a, b, i, int(result.cell[p][i]), "\t".join(d(result.corner[p][c][i]) for c in range(4)))
            for p, (a, b) in enumerate(result.pairs) for i in range(len(result.cell[p]))]


def ale_lines(result):
    """the -ale lines: ascending feature, then ascending edge"""
    from .learning import java_double_str
    d = lambda x: java_double_str(float(x))      # noqa: E731
    return ["%d\t%s\t%s\t%s\t%d" % (f, d(z), d(result.ale[c][k]), d(result.effect[c][k]), int(result.count[c][k]))
            for c, f in enumerate(result.features) for k, z in enumerate(result.edges[c])]


def local_lines(result):
    """the -local lines: feature <TAB> document (from 0, file order) <TAB> interval <TAB> lo <TAB> hi"""
    from .learning import java_double_str
    d = lambda x: java_double_str(float(x))      # noqa: E731
    return ["%d\t%d\t%d\t%s\t%s" % (f, i, int(result.interval[c][i]), d(result.lo[c][i]), d(result.hi[c][i]))
            for c, f in enumerate(result.features) for i in range(len(result.interval[c]))]


def model_thresholds(ranker, feature):
    """the distinct f32 thresholds of feature in a tree model's text, ascending, -0.0 folded into 0.0"""
    from .learning import LambdaMART, RFRanker
    if not isinstance(ranker, (LambdaMART, RFRanker)):
        raise RankLibError("rlhip: -grid thresholds needs a tree model: a %s model has no thresholds" % ranker.name())
    found = re.findall(r"<feature>\s*(\d+)\s*</feature>\s*<threshold>\s*([^<\s]+)\s*</threshold>", ranker.model())
    v = np.array([float(t) for f, t in found if int(f) == int(feature)], np.float64).astype(np.float32)
    return np.unique(v[~np.isnan(v)] + np.float32(0))


def grid_for(model, samples, feature, grid):
    """the f32 grid of one feature, strictly ascending.  grid == "thresholds" (tree models only): the model's distinct thresholds of
    the feature plus nextafter(last, +inf) where that is finite and greater -- every value the PD can take appears, since v <= thr goes
    left.  An integer n: n order statistics of the feature's distinct non-NaN values in samples, at the indices (j (m - 1)) // (n - 1) of
    the m sorted values, duplicates dropped; all m when m <= n.  -0.0 is folded into 0.0 before de-duplicating."""
    feature = int(feature)
    if isinstance(grid, str):
        if grid.lower() != "thresholds":
            raise RankLibError("rlhip: -grid takes a count or 'thresholds' (got %s)" % grid)
        v = model_thresholds(model, feature)
        if v.size:
            with np.errstate(over="ignore"):
                nxt = np.nextafter(v[-1], np.float32(np.inf), dtype=np.float32)
            if np.isfinite(nxt) and nxt > v[-1]:
                v = np.concatenate([v, [nxt]]).astype(np.float32)
        if not v.size:
            raise RankLibError("rlhip: the model has no threshold on feature %d: -grid thresholds has no value for it" % feature)
        return v
    n = int(grid)
    if n < 1:
        raise RankLibError("rlhip: -grid must be at least 1 (got %d)" % n)
    v = order_statistics([dp.fVals[feature] if feature < len(dp.fVals) else np.nan for rl in samples for dp in rl.rl], n)
    if not v.size:
        raise RankLibError("rlhip: feature %d has no value in the file: no grid for it" % feature)
    return v


def order_statistics(values, n):
    """n order statistics of the distinct non-NaN values, f32 ascending (-0.0 folded into 0.0): the indices (j (m - 1)) // (n - 1) of the m
    sorted values, duplicates dropped; all m when m <= n; the middle one for n == 1"""
    col = np.asarray(values, np.float32)
    v = np.unique(col[~np.isnan(col)] + np.float32(0))
    m = len(v)
    if m <= n:
        return v
    if n == 1:
        return v[(m - 1) // 2:(m - 1) // 2 + 1]
    return v[np.unique([(j * (m - 1)) // (n - 1) for j in range(n)])]


def summarize(features, grids, base, mean, shift2, ice=None):
    """Partial of per-cell results: per feature mean and shift2 f64 [G_c]"""
    base = np.asarray(base, np.float64)
    base_mean = fixed_order_sums(base, base)[0] / len(base)
    mean = [np.asarray(m, np.float64) for m in mean]
    with np.errstate(all="ignore"):
        centred = [m - base_mean for m in mean]
        rms = [np.sqrt(np.asarray(s, np.float64)) for s in shift2]
    return Partial([int(f) for f in features], [np.asarray(g, np.float32) for g in grids], mean, centred, rms, base_mean, base, ice)


def _serial(v):
    """the serial f64 chain over v in row-major order, from +0.0"""
    return float(np.cumsum(np.concatenate([[0.0], np.asarray(v, np.float64).ravel()]))[-1])


def h2_on_grid(surface, curve_a, curve_b):
    """Friedman and Popescu's h2 with uniform weights over the cells: surface f64 [ga][gb], curve_a [ga], curve_b [gb], each centred here
    by its unweighted mean; every sum a serial f64 chain in row-major order; 0.0 where the surface is flat"""
    with np.errstate(all="ignore"):
        fab = surface - _serial(surface) / surface.size
        fa = curve_a - _serial(curve_a) / curve_a.size
        fb = curve_b - _serial(curve_b) / curve_b.size
        r = fab - fa[:, None] - fb[None, :]
        den = _serial(fab * fab)
        return _serial(r * r) / den if den != 0.0 else 0.0


def summarize2(pairs, grids, base, mean, shift2, one, ice=None):
    """Partial2 of per-cell results: per pair mean and shift2 f64 [ga * gb] row-major; one: the Partial of the pairs' features on the
    same grids (the curves h2 needs)"""
    base = np.asarray(base, np.float64)
    base_mean = fixed_order_sums(base, base)[0] / len(base)
    grids = [(np.asarray(ga, np.float32), np.asarray(gb, np.float32)) for ga, gb in grids]
    shape = [(len(ga), len(gb)) for ga, gb in grids]
    mean = [np.asarray(m, np.float64).reshape(sh) for m, sh in zip(mean, shape)]
    with np.errstate(all="ignore"):
        centred = [m - base_mean for m in mean]
        rms = [np.sqrt(np.asarray(s, np.float64)).reshape(sh) for s, sh in zip(shift2, shape)]
    curve = lambda f: one.mean[one.features.index(f)]      # noqa: E731
    h2 = [h2_on_grid(m, curve(a), curve(b)) for (a, b), m in zip(pairs, mean)]
    if ice is not None:
        ice = [np.asarray(s, np.float64).reshape(sh + (len(base),)) for s, sh in zip(ice, shape)]
    return Partial2([(int(a), int(b)) for a, b in pairs], grids, mean, centred, rms, h2, base_mean, base, ice)


def _cells2(result):
    """(pair index, a, b, u, v) of the -out2 / -ice2 lines: ascending pair, then ascending values; a pair asked twice is written once"""
    first = {pr: p for p, pr in reversed(list(enumerate(result.pairs)))}
    return [(p, a, b, u, v) for (a, b), p in sorted(first.items()) for u in range(len(result.grids[p][0])) for v in range(len(result.grids[p][1]))]


def table2_lines(result):
    """the -out2 lines: the cells, then one h2 line per pair"""
    from .learning import java_double_str
    d = lambda x: java_double_str(float(x))      # noqa: E731
    cells = _cells2(result)
    out = ["%d\t%d\t%s\t%s\t%s\t%s\t%s" % (a, b, d(result.grids[p][0][u]), d(result.grids[p][1][v]), d(result.mean[p][u, v]),
                                          d(result.centred[p][u, v]), d(result.rms[p][u, v])) for p, a, b, u, v in cells]
    return out + ["%d\t%d\th2\t%s" % (a, b, d(result.h2[p])) for p, a, b in sorted({(p, a, b) for p, a, b, _, _ in cells}, key=lambda t: t[1:])]


def ice2_lines(result):
    from .learning import java_double_str
    d = lambda x: java_double_str(float(x))      # noqa: E731
    return ["%d\t%d\t%s\t%s\t%s" % (a, b, d(result.grids[p][0][u]), d(result.grids[p][1][v]), "\t".join(d(s) for s in result.ice[p][u, v]))
            for p, a, b, u, v in _cells2(result)]


def read_pairs(path):
    """the -pairs file: one "a b" per line; empty lines and lines that start with # are skipped"""
    out = []
    with open(path, encoding="ascii") as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#"):
                continue
            if len(t) != 2 or not all(x.isdigit() for x in t):
                raise RankLibError("-pairs takes one pair of feature ids 'a b' per line (got %s)" % ln.strip())
            out.append((int(t[0]), int(t[1])))
    return out


def _grid_arg(flag, grid):
    if grid.lower() == "thresholds":
        return grid
    try:
        return int(grid)
    except ValueError:
        raise RankLibError("%s takes a count or 'thresholds' (got %s)" % (flag, grid)) from None


def table_lines(result):
    """the -out lines: ascending feature, then ascending value"""
    from .learning import java_double_str
    return ["%d\t%s\t%s\t%s\t%s" % (f, java_double_str(float(v)), java_double_str(float(result.mean[c][g])),
                                    java_double_str(float(result.centred[c][g])), java_double_str(float(result.rms[c][g])))
            for c, f in enumerate(result.features) for g, v in enumerate(result.grids[c])]


def ice_lines(result):
    from .learning import java_double_str
    return ["%d\t%s\t%s" % (f, java_double_str(float(v)), "\t".join(java_double_str(float(s)) for s in result.ice[c][g]))
            for c, f in enumerate(result.features) for g, v in enumerate(result.grids[c])]


def main(argv=None):
    from .evaluator import ArgCursor, Evaluator, common_flag
    from .features import FeatureManager
    from .learning import RankerFactory, RankerType
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args:
        print("Usage: -load model -test file [-feature file] [-grid n|thresholds] [-norm sum|zscore|linear] [-qrel f] [-gmax g] [-missingZero] "
              "[-hr] [-device d] [-out tsv] [-ice file] [-pairs file [-grid2 n|thresholds] [-out2 tsv] [-ice2 file]]")
        print("       accumulated local effects: [-ale tsv [-intervals n] [-local file]]")
        print("       second-order accumulated local effects of the pairs: [-ale2 tsv [-intervals2 n] [-local2 file]]")
        return 0
    models, testFiles = [], []
    grid, featureFile, outFile, iceFile = "20", "", "", ""
    grid2, pairsFile, out2File, ice2File = "10", "", "", ""
    aleFile, intervals, localFile = "", "", ""
    ale2File, intervals2, local2File = "", "", ""
    Evaluator.mustHaveRelDoc = False
    Evaluator.normalize = False
    Evaluator.qrelFile = ""
    cur = ArgCursor(args)
    nxt = cur.nxt
    for a in cur:
        if a == "-load": models.append(nxt())
        elif a == "-test": testFiles.append(nxt())
        elif a == "-grid": grid = nxt()
        elif a == "-feature": featureFile = nxt()
        elif a == "-out": outFile = nxt()
        elif a == "-ice": iceFile = nxt()
        elif a == "-pairs": pairsFile = nxt()
        elif a == "-grid2": grid2 = nxt()
        elif a == "-out2": out2File = nxt()
        elif a == "-ice2": ice2File = nxt()
        elif a == "-ale": aleFile = nxt()
        elif a == "-intervals": intervals = nxt()
        elif a == "-local": localFile = nxt()
        elif a == "-ale2": ale2File = nxt()
        elif a == "-intervals2": intervals2 = nxt()
        elif a == "-local2": local2File = nxt()
        elif not common_flag(a, nxt):
            cur.unknown()
    if len(models) != 1:
        raise RankLibError("ranklib_amd.partial takes exactly one -load model (got %d)" % len(models))
    if len(testFiles) != 1:
        raise RankLibError("ranklib_amd.partial takes exactly one -test file (got %d)" % len(testFiles))
    if (out2File or ice2File) and not pairsFile:
        raise RankLibError("-out2 and -ice2 need -pairs file")
    if (intervals or localFile) and not aleFile:
        raise RankLibError("-intervals and -local need -ale tsv")
    if intervals and not (intervals.isdigit() and 1 <= int(intervals) <= ALE_MAX_INTERVALS):
        raise RankLibError("-intervals takes a count 1 .. %d (got %s)" % (ALE_MAX_INTERVALS, intervals))
    if (intervals2 or local2File) and not ale2File:
        raise RankLibError("-intervals2 and -local2 need -ale2 tsv")
    if ale2File and not pairsFile:
        raise RankLibError("-ale2 needs -pairs file")
    if intervals2 and not (intervals2.isdigit() and 1 <= int(intervals2) <= ALE2_MAX_INTERVALS):
        raise RankLibError("-intervals2 takes a count 1 .. %d (got %s)" % (ALE2_MAX_INTERVALS, intervals2))
    grid = _grid_arg("-grid", grid)
    pairs = read_pairs(pairsFile) if pairsFile else None
    ranker = RankerFactory().loadRankerFromFile(models[0])
    features = [int(f) for f in FeatureManager.readFeature(featureFile)] if featureFile else None
    e = Evaluator(RankerType.LAMBDAMART, "ERR@10", "ERR@10")
    test = e.readTestFile(ranker, testFiles[0])
    if aleFile:
        ale = ranker.accumulatedEffects(test, features=features, intervals=int(intervals or 20), local=bool(localFile))
        lines = ale_lines(ale)
        logger.info("feature\tedge\tale\tlocal effect\tcount\t(%s)", testFiles[0])
        for ln in lines:
            logger.info(ln)
        with open(aleFile, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in lines))
        logger.info("Accumulated local effects saved to: %s", aleFile)
        if localFile:
            with open(localFile, "w", encoding="ascii") as out:
                out.write("".join(ln + "\n" for ln in local_lines(ale)))
            logger.info("Local effects saved to: %s", localFile)
        if not (outFile or iceFile or pairsFile):
            return 0
    if ale2File:
        ale2 = ranker.accumulatedEffects2(test, pairs, intervals=int(intervals2 or 10), local=bool(local2File))
        lines = ale2_lines(ale2)
        logger.info("a\tb\tedge a\tedge b\tale\tlocal effect\tcount\t(%s)", testFiles[0])
        for ln in lines:
            logger.info(ln)
        with open(ale2File, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in lines))
        logger.info("Second-order accumulated local effects saved to: %s", ale2File)
        if local2File:
            with open(local2File, "w", encoding="ascii") as out:
                out.write("".join(ln + "\n" for ln in local2_lines(ale2)))
            logger.info("Local second-order effects saved to: %s", local2File)
        if not (outFile or iceFile or out2File or ice2File):
            return 0
    res = ranker.partialDependence(test, features=features, grid=grid, ice=bool(iceFile))
    lines = table_lines(res)
    logger.info("feature\tvalue\tmean\tcentred mean\trms shift\t(%s, base mean %s)", testFiles[0], res.base_mean)
    for ln in lines:
        logger.info(ln)
    if outFile:
        with open(outFile, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in lines))
        logger.info("Partial dependence saved to: %s", outFile)
    if iceFile:
        with open(iceFile, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in ice_lines(res)))
        logger.info("ICE curves saved to: %s", iceFile)
    if pairs is not None:
        res2 = ranker.partialDependence2(test, pairs, grid=_grid_arg("-grid2", grid2), ice=bool(ice2File))
        lines = table2_lines(res2)
        logger.info("a\tb\tvalue a\tvalue b\tmean\tcentred mean\trms shift")
        for ln in lines:
            logger.info(ln)
        if out2File:
            with open(out2File, "w", encoding="ascii") as out:
                out.write("".join(ln + "\n" for ln in lines))
            logger.info("Two-feature partial dependence saved to: %s", out2File)
        if ice2File:
            with open(ice2File, "w", encoding="ascii") as out:
                out.write("".join(ln + "\n" for ln in ice2_lines(res2)))
            logger.info("Two-feature ICE surfaces saved to: %s", ice2File)
    return 0


if __name__ == "__main__":
    sys.exit(main())
