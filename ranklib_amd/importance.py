"""python -m ranklib_amd.importance: permutation feature importance of a model on a file it was not trained on -- what a
feature is worth under the metric: shuffle its column, score and rank the file again, see how far the metric falls.  RankLib has only
-feature_stats, how often a feature appears in a split (features/FeatureStats.java).  A LambdaMART / MART model takes every (feature,
repeat) cell in one GPU pass per file (LambdaMART.permutationImportance, rl_model_eval_permuted); every other model scores one permuted
copy per cell (Ranker.permutationImportance).  Both give the same bits.

  -load model            the model (one)
  -test file             the file to evaluate on (one)
  -metric2T M            the metric (the evaluator's default, ERR@10)
  -repeat R              permutations per feature (default 5)
  -seed s                repeat r draws its permutation from numpy.random.RandomState(s + r) (default 1)
  -within                permute inside every list instead of over the whole file
  -feature file          the features to measure, one id per line as RankLib's -feature files (default: the model's own, ascending)
  -norm, -qrel, -gmax, -missingZero, -hr, -device   as in ranklib_amd.stages: the file is prepared by Evaluator.readTestFile
  -out tsv               one line per feature: id <TAB> importance <TAB> std over repeats <TAB> base mean <TAB> mean of repeat 1 ...

Lines are sorted by descending importance, ties by ascending feature id; the numbers are printed as Double.toString.  A mean is the
serial f64 sum of a file's list values in list order divided by the list count, as Evaluator.test has it; importance = base mean - the
serial mean of the repeat means; std is the population standard deviation of the repeat means.
"""
import collections
import logging
import math
import sys

import numpy as np

from ._native import RankLibError

logger = logging.getLogger("ranklib_amd")

Importance = collections.namedtuple("Importance", "features base_mean repeat_means importance std base values")
Importance.__doc__ = """features [F]; base_mean; repeat_means f64 [F][R]; importance f64 [F]; std f64 [F]; base f64 [lists], the unpermuted
per-list values; values f64 [F][R][lists], the per-list values of every cell"""


def donor_maps(sizes, repeats, seed=1, within=False):
    """int32 [repeats][n_docs]: donor[r][i] is the document whose value document i receives in repeat r.  sizes: the lists' lengths in
    file order.  Repeat r is numpy.random.RandomState(seed + r).permutation(n_docs) -- a stream NumPy's compatibility policy freezes --
    or, within, the same generator applied list by list in file order, every donor staying in its own list."""
    if repeats < 1:
        raise RankLibError("-repeat must be at least 1 (got %d)" % repeats)
    sizes = [int(s) for s in sizes]
    n = sum(sizes)
    out = np.zeros((repeats, n), np.int32)
    for r in range(repeats):
        rs = np.random.RandomState(seed + r)
        if not within:
            out[r] = rs.permutation(n)
            continue
        a = 0
        for s in sizes:
            out[r, a:a + s] = a + rs.permutation(s)
            a += s
    return out


def serial_mean(values):
    s = 0.0
    for v in values:
        s += float(v)
    return s / len(values)


def summarize(features, base, values):
    """Importance of per-list values: base [lists], values [F][R][lists]"""
    values = np.asarray(values, np.float64)
    F, R = values.shape[0], values.shape[1]
    base_mean = serial_mean(base)
    means = np.array([[serial_mean(values[c, r]) for r in range(R)] for c in range(F)], np.float64).reshape(F, R)
    imp, std = np.zeros(F), np.zeros(F)
    for c in range(F):
        mu = serial_mean(means[c])
        imp[c] = base_mean - mu
        std[c] = math.sqrt(serial_mean([(float(v) - mu) * (float(v) - mu) for v in means[c]]))
    return Importance([int(f) for f in features], base_mean, means, imp, std, np.asarray(base, np.float64), values)


def table_lines(result):
    """the -out lines: descending importance, ties (and only ties) by ascending feature id"""
    from .learning import java_double_str
    order = sorted(range(len(result.features)), key=lambda c: (-result.importance[c], result.features[c]))
    return ["%d\t%s\t%s\t%s\t%s" % (result.features[c], java_double_str(float(result.importance[c])), java_double_str(float(result.std[c])),
                                    java_double_str(float(result.base_mean)),
                                    "\t".join(java_double_str(float(v)) for v in result.repeat_means[c])) for c in order]


def main(argv=None):
    from .evaluator import ArgCursor, Evaluator, common_flag
    from .features import FeatureManager
    from .learning import RankerFactory, RankerType
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args:
        print("Usage: -load model -test file [-metric2T M] [-repeat R] [-seed s] [-within] [-feature file] [-norm sum|zscore|linear] [-qrel f] "
              "[-gmax g] [-missingZero] [-hr] [-device d] [-out tsv]")
        return 0
    models, testFiles = [], []
    metric, repeats, seed, within, featureFile, outFile = "ERR@10", 5, 1, False, "", ""
    Evaluator.mustHaveRelDoc = False
    Evaluator.normalize = False
    Evaluator.qrelFile = ""
    cur = ArgCursor(args)
    nxt = cur.nxt
    for a in cur:
        if a == "-load": models.append(nxt())
        elif a == "-test": testFiles.append(nxt())
        elif a == "-metric2t": metric = nxt()
        elif a == "-repeat": repeats = int(nxt())
        elif a == "-seed": seed = int(nxt())
        elif a == "-within": within = True
        elif a == "-feature": featureFile = nxt()
        elif a == "-out": outFile = nxt()
        elif not common_flag(a, nxt):
            cur.unknown()
    if len(models) != 1:
        raise RankLibError("ranklib_amd.importance takes exactly one -load model (got %d)" % len(models))
    if len(testFiles) != 1:
        raise RankLibError("ranklib_amd.importance takes exactly one -test file (got %d)" % len(testFiles))
    if repeats < 1:
        raise RankLibError("-repeat must be at least 1 (got %d)" % repeats)
    ranker = RankerFactory().loadRankerFromFile(models[0])
    features = [int(f) for f in FeatureManager.readFeature(featureFile)] if featureFile else None
    e = Evaluator(RankerType.LAMBDAMART, metric, metric)
    test = e.readTestFile(ranker, testFiles[0])
    res = ranker.permutationImportance(test, e.testScorer, features=features, repeats=repeats, seed=seed, within=within)
    lines = table_lines(res)
    logger.info("feature\timportance\tstd\t%s on %s\trepeats", e.testScorer.name(), testFiles[0])
    for ln in lines:
        logger.info(ln)
    if outFile:
        with open(outFile, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in lines))
        logger.info("Importance saved to: %s", outFile)
    return 0


if __name__ == "__main__":
    sys.exit(main())
