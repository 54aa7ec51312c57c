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

Lines are sorted by ascending feature, then ascending value; the numbers are printed as Double.toString.  The sums behind a mean take
one fixed order (include/rlhip.h): partial p is the serial f64 chain over the documents [256 p, 256 p + 256), the total the serial chain
over the partials.  centred mean = mean - the base mean (the same sum over the unsubstituted scores); rms shift = sqrt of the mean
squared move of a document away from its own score: its spread over a feature's cells shows how much the feature matters at all.
"""
import collections
import logging
import re
import sys

import numpy as np

from ._native import PARTIAL_SUM_BLOCK, RankLibError

logger = logging.getLogger("ranklib_amd")

Partial = collections.namedtuple("Partial", "features grids mean centred rms base_mean base ice")
Partial.__doc__ = """features [F], ascending; per feature c: grids[c] f32 [G_c], mean[c] f64 [G_c] (the PD values), centred[c] = mean[c] -
base_mean, rms[c] = sqrt(shift2); base_mean; base f64 [n_docs], the unsubstituted scores; ice: None, or per feature f64 [G_c][n_docs]"""


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
              "[-hr] [-device d] [-out tsv] [-ice file]")
        return 0
    models, testFiles = [], []
    grid, featureFile, outFile, iceFile = "20", "", "", ""
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
        elif not common_flag(a, nxt):
            cur.unknown()
    if len(models) != 1:
        raise RankLibError("ranklib_amd.partial takes exactly one -load model (got %d)" % len(models))
    if len(testFiles) != 1:
        raise RankLibError("ranklib_amd.partial takes exactly one -test file (got %d)" % len(testFiles))
    if grid.lower() != "thresholds":
        try:
            grid = int(grid)
        except ValueError:
            raise RankLibError("-grid takes a count or 'thresholds' (got %s)" % grid) from None
    ranker = RankerFactory().loadRankerFromFile(models[0])
    features = [int(f) for f in FeatureManager.readFeature(featureFile)] if featureFile else None
    e = Evaluator(RankerType.LAMBDAMART, "ERR@10", "ERR@10")
    test = e.readTestFile(ranker, testFiles[0])
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
