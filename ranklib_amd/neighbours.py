"""python -m ranklib_amd.neighbours: for every document of a file the k documents of a reference file that a LambdaMART / MART model treats
most like it -- those that reach the same leaf in the most trees, the proximity of random-forest practice.  One GPU pass
(LambdaMART.neighbours, rl_model_predict_neighbours): both files are walked on the device and matched there.

  -load model            the model (one): LambdaMART or MART
  -reference file        the documents neighbours are taken from (one), usually the training file
  -test file             the documents whose neighbours are asked for (one)
  -self                  the test file is the reference: no -reference, and no document is its own neighbour
  -k n                   neighbours per document (default 10, at most 64)
  -feature file          the features -norm normalises over, one id per line as RankLib's -feature files (default: the model's own)
  -norm, -missingZero, -device   as in ranklib_amd.leaves: the files are prepared by Evaluator.readTestFile
  -from t                the first tree of the window (default 0)
  -count n               the trees of the window (default: through the last tree)
  -out tsv               one line per (document, neighbour), documents in file order, neighbours by shared trees descending and then by
                         their place in the reference file: the document's qid <TAB> its description <TAB> the neighbour's rank from 1
                         <TAB> its qid <TAB> its description <TAB> its label <TAB> the trees they share <TAB> the trees of the window.
                         A description a line does not have is an empty field.
"""
import logging
import sys

from ._native import NEAR_MAX_K, RankLibError

logger = logging.getLogger("ranklib_amd")


def out_line(dp, rank, ndp, shared, trees):
    """the -out line of one (document, neighbour)"""
    from .learning import java_float_to_int
    return "%s\t%s\t%d\t%s\t%s\t%d\t%d\t%d" % (dp.id, dp.description or "", rank, ndp.id, ndp.description or "", java_float_to_int(ndp.label),
                                               shared, trees)


def main(argv=None):
    from .evaluator import ArgCursor, Evaluator, common_flag
    from .features import FeatureManager
    from .learning import LambdaMART, RankerFactory, RankerType
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args:
        print("Usage: -load model (-reference file -test file | -self -test file) [-k n] [-feature file] [-norm sum|zscore|linear] "
              "[-missingZero] [-device d] [-from t] [-count n] -out tsv")
        return 0
    models, refFiles, testFiles = [], [], []
    featureFile, outFile = "", ""
    first, count, k, own = 0, None, 10, False
    Evaluator.mustHaveRelDoc = False
    Evaluator.normalize = False
    Evaluator.qrelFile = ""
    cur = ArgCursor(args)
    nxt = cur.nxt

    def number(flag, what):
        v = nxt()
        try:
            return int(v)
        except ValueError:
            raise RankLibError("%s takes a number of %s (got %s)" % (flag, what, v)) from None
    for a in cur:
        if a == "-load": models.append(nxt())
        elif a == "-reference": refFiles.append(nxt())
        elif a == "-test": testFiles.append(nxt())
        elif a == "-self": own = True
        elif a == "-k": k = number("-k", "neighbours")
        elif a == "-feature": featureFile = nxt()
        elif a == "-from": first = number("-from", "trees")
        elif a == "-count": count = number("-count", "trees")
        elif a == "-out": outFile = nxt()
        elif not common_flag(a, nxt, reader_only=True):
            cur.unknown()
    if len(models) != 1:
        raise RankLibError("ranklib_amd.neighbours takes exactly one -load model (got %d)" % len(models))
    if len(testFiles) != 1:
        raise RankLibError("ranklib_amd.neighbours takes exactly one -test file (got %d)" % len(testFiles))
    if len(refFiles) != (0 if own else 1):
        raise RankLibError("ranklib_amd.neighbours takes -self or exactly one -reference file (got %s%d)" % ("-self and " if own else "", len(refFiles)))
    if not outFile:
        raise RankLibError("ranklib_amd.neighbours needs -out tsv")
    if not 1 <= k <= NEAR_MAX_K:
        raise RankLibError("-k must be in 1 .. %d (got %d)" % (NEAR_MAX_K, k))
    if first < 0:
        raise RankLibError("-from must be at least 0 (got %d)" % first)
    if count is not None and count < 1:
        raise RankLibError("-count must be at least 1 (got %d)" % count)
    ranker = RankerFactory().loadRankerFromFile(models[0])
    if not isinstance(ranker, LambdaMART):
        ranker.neighbours([], [])                           # the refusal, naming the model type
    if featureFile:
        ranker.setFeatures([int(f) for f in FeatureManager.readFeature(featureFile)])
    total = len(ranker.leafCounts())
    if first >= total or (count is not None and first + count > total):
        raise RankLibError("-from %d%s leaves the model's %d trees" % (first, "" if count is None else " -count %d" % count, total))
    trees = total - first if count is None else count
    e = Evaluator(RankerType.LAMBDAMART, "ERR@10", "ERR@10")
    test = e.readTestFile(ranker, testFiles[0])
    ref = test if own else e.readTestFile(ranker, refFiles[0])
    dps, rdps = [dp for rl in test for dp in rl.rl], [dp for rl in ref for dp in rl.rl]
    if not dps or not rdps:
        raise RankLibError("ranklib_amd.neighbours needs at least one document in either file")
    index, shared = ranker.neighbours(test, ref, k, first, count, own)
    with open(outFile, "w", encoding="ascii") as out:
        for dp, ids, cnt in zip(dps, index, shared):
            out.write("".join(out_line(dp, j + 1, rdps[i], s, trees) + "\n" for j, (i, s) in enumerate(zip(ids, cnt)) if i >= 0))
    logger.info("Up to %d neighbours of %d documents among %d, by shared leaves in %d trees, saved to: %s", k, len(dps), len(rdps), trees, outFile)
    return 0


if __name__ == "__main__":
    sys.exit(main())
