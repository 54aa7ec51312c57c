"""python -m ranklib_amd.leaves: the leaf every document of a file reaches in every tree of a LambdaMART / MART model --
pred_leaf of XGBoost and LightGBM, apply() of scikit-learn.  One GPU pass per chunk of the file (LambdaMART.leaves,
rl_model_predict_leaves); the leaves of a tree are numbered from 0 in the order of its leaves in the model text, left first.

  -load model            the model (one): LambdaMART or MART
  -test file             the file (one)
  -feature file          the features -norm normalises over, one id per line as RankLib's -feature files (default: the model's own)
  -norm, -missingZero, -device   as in ranklib_amd.contribs: the file is prepared by Evaluator.readTestFile
  -from t                the first tree of the window (default 0)
  -count n               the trees of the window (default: through the last tree)
  -out tsv               one line per document in file order: qid <TAB> the document's description, where the line has one <TAB> the leaf
                         number in every tree of the window, tab-separated
  -npy file              the same numbers as a NumPy file, uint16 [documents][trees]
  -letor file            the one-hot leaf embedding as sparse LETOR lines for a downstream learner: label qid:id c:1 c:1 ..., one c per
                         tree of the window, ascending: c = 1 + the leaves of the window's trees before the tree + the leaf number

The file goes through the device in chunks of whole lists (learning.list_chunks), and the lines are written chunk by chunk.
"""
import logging
import sys

import numpy as np

from ._native import RankLibError

logger = logging.getLogger("ranklib_amd")


def out_line(dp, leaves):
    """the -out line of one document: leaves uint16 [trees]"""
    return "\t".join([dp.id] + ([dp.description] if dp.description else []) + [str(int(v)) for v in leaves])


def letor_line(dp, leaves, base):
    """the -letor line of one document: base int64 [trees], 1 + the leaves of the window's trees before each tree"""
    from .learning import java_float_to_int
    return "%d qid:%s %s" % (java_float_to_int(dp.label), dp.id, " ".join("%d:1" % c for c in base + leaves.astype(np.int64)))


def column_bases(counts):
    """1 + the leaves before every tree of a window whose trees have counts leaves: the first LETOR feature id of every tree"""
    return 1 + np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))[:-1]]).astype(np.int64)


def main(argv=None):
    from .evaluator import ArgCursor, Evaluator, common_flag
    from .features import FeatureManager
    from .learning import LambdaMART, Ranker, RankerFactory, RankerType, list_chunks
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args:
        print("Usage: -load model -test file [-feature file] [-norm sum|zscore|linear] [-missingZero] [-device d] [-from t] [-count n] "
              "-out tsv [-npy file] [-letor file]")
        return 0
    models, testFiles = [], []
    featureFile, outFile, npyFile, letorFile = "", "", "", ""
    first, count = 0, None
    Evaluator.mustHaveRelDoc = False
    Evaluator.normalize = False
    Evaluator.qrelFile = ""
    cur = ArgCursor(args)
    nxt = cur.nxt

    def number(flag):
        v = nxt()
        try:
            return int(v)
        except ValueError:
            raise RankLibError("%s takes a number of trees (got %s)" % (flag, v)) from None
    for a in cur:
        if a == "-load": models.append(nxt())
        elif a == "-test": testFiles.append(nxt())
        elif a == "-feature": featureFile = nxt()
        elif a == "-from": first = number("-from")
        elif a == "-count": count = number("-count")
        elif a == "-out": outFile = nxt()
        elif a == "-npy": npyFile = nxt()
        elif a == "-letor": letorFile = nxt()
        elif not common_flag(a, nxt, reader_only=True):     # no -gmax, -qrel, -hr here, and -device is LambdaMART's alone
            cur.unknown()
    if len(models) != 1:
        raise RankLibError("ranklib_amd.leaves takes exactly one -load model (got %d)" % len(models))
    if len(testFiles) != 1:
        raise RankLibError("ranklib_amd.leaves takes exactly one -test file (got %d)" % len(testFiles))
    if not outFile:
        raise RankLibError("ranklib_amd.leaves needs -out tsv")
    if first < 0:
        raise RankLibError("-from must be at least 0 (got %d)" % first)
    if count is not None and count < 1:
        raise RankLibError("-count must be at least 1 (got %d)" % count)
    ranker = RankerFactory().loadRankerFromFile(models[0])
    if not isinstance(ranker, LambdaMART):
        ranker.leaves([])                                   # the refusal, naming the model type
    if featureFile:
        ranker.setFeatures([int(f) for f in FeatureManager.readFeature(featureFile)])
    counts = ranker.leafCounts()
    if first >= len(counts) or (count is not None and first + count > len(counts)):
        raise RankLibError("-from %d%s leaves the model's %d trees" % (first, "" if count is None else " -count %d" % count, len(counts)))
    counts = counts[first:] if count is None else counts[first:first + count]
    base = column_bases(counts)
    e = Evaluator(RankerType.LAMBDAMART, "ERR@10", "ERR@10")
    test = e.readTestFile(ranker, testFiles[0])
    parts, docs = [], 0
    out = open(outFile, "w", encoding="ascii")
    letor = open(letorFile, "w", encoding="ascii") if letorFile else None
    try:
        for a, b in list_chunks(test, Ranker.EVAL_ROW_BYTES):
            dps = [dp for rl in test[a:b] for dp in rl.rl]
            if not dps:
                continue
            got = ranker.leaves(ranker._rows(dps), first, count)
            out.write("".join(out_line(dp, row) + "\n" for dp, row in zip(dps, got)))
            if letor:
                letor.write("".join(letor_line(dp, row, base) + "\n" for dp, row in zip(dps, got)))
            if npyFile:
                parts.append(got)
            docs += len(dps)
    finally:
        out.close()
        if letor:
            letor.close()
    logger.info("Leaves of %d documents in %d trees (%d leaves in all) saved to: %s", docs, len(counts), int(np.sum(counts)), outFile)
    if letorFile:
        logger.info("One-hot leaf features 1 .. %d saved to: %s", int(np.sum(counts)), letorFile)
    if npyFile:
        np.save(npyFile, np.concatenate(parts) if parts else np.zeros((0, len(counts)), np.uint16))
        logger.info("Leaf numbers saved to: %s", npyFile)
    return 0


if __name__ == "__main__":
    sys.exit(main())
