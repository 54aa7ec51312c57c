"""python -m ranklib_amd.contribs: which features put a document where it is -- per-document feature contributions of a LambdaMART /
MART model (Saabas path attribution, XGBoost's pred_contribs with approx_contribs) in one GPU pass per file (LambdaMART.contributions,
DESIGN.md 26).  RankLib's model text holds no node counts, so every node's cover is counted on a background file first, usually the
training file.  A document's contributions sum to the f64 sum of its weighted leaf outputs, which is the model's score up to the float
rounding of Ensemble.eval's chain -- not its bits.

  -load model            the model (one)
  -background file       the file the nodes' covers are counted on (repeatable: the counts add up)
  -test file             the file whose documents are explained (one)
  -feature file          the features to report, one id per line as for the evaluator; what the others contribute goes to `rest`
                         (default: every feature the model splits on)
  -exact                 exact Shapley values (path-dependent TreeSHAP, XGBoost's pred_contribs without approx_contribs)
                         in place of Saabas' path attribution: the same files and the same local-accuracy line, from about two orders
                         of magnitude more work on the device
  -interactions tsv      SHAP interaction values (XGBoost's pred_interactions) summed over the file; implies -exact, and
                         -out / -summary still work beside it.  One line per unordered pair i < j of the reported features:
                         fi <TAB> fj <TAB> mean |out[i][j] + out[j][i]| <TAB> mean (out[i][j] + out[j][i]), and one line
                         fi <TAB> fi <TAB> mean |out[i][i]| <TAB> mean out[i][i] per feature, sorted by the first number descending, then
                         by the ids (pairs with `rest` are printed, not written).  Every sum over the documents is one serial f64 chain
                         in file order, carried from chunk to chunk, so it does not depend on the chunking; each is divided once.
                         Per-document matrices: LambdaMART.interactions.
  -norm, -missingZero, -device   as in ranklib_amd.evaluator: the files are prepared by the code its -load -test uses
  -out tsv               one line per document: qid <TAB> index in its list <TAB> the model's score (Float.toString) and then
                         fid:value ... rest:value bias:value, the values as Double.toString
  -summary tsv           one line per feature: id <TAB> mean |contribution| over the file <TAB> mean contribution, sorted by the first
                         descending, then by id (`rest` and `bias` are printed, not written).  The sums are math.fsum over the documents,
                         divided once: exactly rounded, so the order of the documents does not matter.

It also prints the largest |sum of a document's slots - f64 sum of its weighted leaf outputs| over the file, the right-hand side from a
walk of its own on the device (rl_model_predict_leaf_sums), chunk by chunk as the contributions go.
"""
import logging
import math
import sys

import numpy as np

from ._native import RankLibError

logger = logging.getLogger("ranklib_amd")


def _means(col):
    col = [float(v) for v in col]
    return math.fsum(abs(v) for v in col) / len(col), math.fsum(col) / len(col)


def summary_lines(ids, matrix):
    """the -summary lines of contributions [docs][len(ids) + 2]: one per feature"""
    from .learning import java_double_str
    rows = sorted(((f,) + _means(matrix[:, c]) for c, f in enumerate(ids)), key=lambda r: (-r[1], r[0]))
    return ["%d\t%s\t%s" % (f, java_double_str(a), java_double_str(m)) for f, a, m in rows]


def chain_sums(carry, values):
    """carry [cells] + the serial f64 chain over values [docs][cells] in document order: cumsum is a serial chain (partial.fixed_order_sums'
    device), and its first element is the carry, so a file summed chunk after chunk gives the bits of one chain over the file"""
    with np.errstate(all="ignore"):
        return np.cumsum(np.concatenate([np.asarray(carry, np.float64)[None], np.asarray(values, np.float64)]), axis=0)[-1]


def pair_values(matrix):
    """[docs][C + 1][C + 1] of interaction values [docs][C + 2][C + 2]: cell [i][j], i != j, holds out[i][j] + out[j][i] (one rounded
    sum; the two orders give the same bits), cell [i][i] holds out[i][i]; the bias row and column are left out"""
    m = np.asarray(matrix, np.float64)[:, :-1, :-1]
    with np.errstate(all="ignore"):
        v = m + m.transpose(0, 2, 1)
    k = np.arange(m.shape[1])
    v[:, k, k] = m[:, k, k]
    return v


def pair_lines(ids, abs_sums, sums, n_docs):
    """(the -interactions lines, the lines of the pairs with rest): abs_sums and sums [C + 1][C + 1] are the chains of |pair_values| and
    pair_values over n_docs documents"""
    from .learning import java_double_str
    C = len(ids)
    names = [int(f) for f in ids] + ["rest"]
    rows = [(float(abs_sums[i, j]) / n_docs, float(sums[i, j]) / n_docs, i, j) for i in range(C + 1) for j in range(i, C + 1)]
    keep = sorted((r for r in rows if r[3] < C), key=lambda r: (-r[0], names[r[2]], names[r[3]]))
    rest = sorted((r for r in rows if r[3] == C), key=lambda r: (-r[0], r[2]))
    fmt = lambda r: "%s\t%s\t%s\t%s" % (names[r[2]], names[r[3]], java_double_str(r[0]), java_double_str(r[1]))      # noqa: E731
    return [fmt(r) for r in keep], [fmt(r) for r in rest]


def main(argv=None):
    from .evaluator import ArgCursor, Evaluator, common_flag
    from .features import FeatureManager
    from .learning import LambdaMART, RankerFactory, RankerType, java_double_str, java_float_str, result_steps
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args:
        print("Usage: -load model -background file [-background file ...] -test file [-feature file] [-norm sum|zscore|linear] [-missingZero] "
              "[-device d] [-out tsv] [-summary tsv] [-exact] [-interactions tsv]")
        return 0
    models, backgrounds, testFiles = [], [], []
    featureFile, outFile, summaryFile, pairFile = "", "", "", ""
    exact = False
    Evaluator.mustHaveRelDoc = False
    Evaluator.normalize = False
    Evaluator.qrelFile = ""
    cur = ArgCursor(args)
    nxt = cur.nxt
    for a in cur:
        if a == "-load": models.append(nxt())
        elif a == "-background": backgrounds.append(nxt())
        elif a == "-test": testFiles.append(nxt())
        elif a == "-feature": featureFile = nxt()
        elif a == "-out": outFile = nxt()
        elif a == "-summary": summaryFile = nxt()
        elif a == "-exact": exact = True
        elif a == "-interactions":
            pairFile = nxt()
            exact = True
        elif not common_flag(a, nxt, reader_only=True):     # no -gmax, -qrel, -hr here, and -device is LambdaMART's alone
            cur.unknown()
    if len(models) != 1:
        raise RankLibError("ranklib_amd.contribs takes exactly one -load model (got %d)" % len(models))
    if not backgrounds:
        raise RankLibError("ranklib_amd.contribs needs a -background file: the model text holds no node counts")
    if len(testFiles) != 1:
        raise RankLibError("ranklib_amd.contribs needs a -test file, exactly one (got %d)" % len(testFiles))
    ranker = RankerFactory().loadRankerFromFile(models[0])
    if not isinstance(ranker, LambdaMART):
        ranker.contributions([], None)                      # the refusal, naming the model type
    features = [int(f) for f in FeatureManager.readFeature(featureFile)] if featureFile else None
    e = Evaluator(RankerType.LAMBDAMART, "ERR@10", "ERR@10")
    for k, f in enumerate(backgrounds):
        ranker.countCover(e.readTestFile(ranker, f), accumulate=k > 0)
    test = e.readTestFile(ranker, testFiles[0])
    cols = None if features is None else features
    ids = [int(f) for f in ranker._model.features()] if cols is None else cols
    parts, scores, worst = [], [], 0.0
    predict = ranker._model.predict_shap if exact else ranker._model.predict_contribs
    S = len(ids) + 2
    pair_abs, pair_sum = np.zeros((S - 1, S - 1)), np.zeros((S - 1, S - 1))
    gap_row = gap_sym = gap_all = 0.0
    for rows in ranker._rowChunks(test):                    # whole lists, the rows of a chunk under EVAL_ROW_BYTES
        part = predict(rows, cols)[0]
        for a0, b0 in result_steps(len(rows) if pairFile else 0, 8 * S * S):      # pieces whose matrices stay under EVAL_ROW_BYTES
            sub = rows[a0:b0]
            inter = ranker._model.predict_interactions(sub, cols)[0]
            vals = pair_values(inter)
            pair_abs, pair_sum = chain_sums(pair_abs, np.abs(vals)), chain_sums(pair_sum, vals)
            with np.errstate(all="ignore"):
                rs = np.zeros(inter.shape[:2], np.float64)
                for c in range(S):                          # cell after cell: a serial f64 sum per document and row of its matrix
                    rs = rs + inter[:, :, c]
                cs = np.zeros(len(sub), np.float64)
                for c in range(S):
                    cs = cs + rs[:, c]
                gaps = [np.abs(rs - part[a0:a0 + len(sub)]), np.abs(inter - inter.transpose(0, 2, 1)), np.abs(cs - ranker._model.leaf_sums(sub))]
            gaps = [float(g[np.isfinite(g)].max()) if np.isfinite(g).any() else 0.0 for g in gaps]
            gap_row, gap_sym, gap_all = max(gap_row, gaps[0]), max(gap_sym, gaps[1]), max(gap_all, gaps[2])
        parts.append(part)
        scores.append(ranker._model.predict_rows(rows))
        with np.errstate(all="ignore"):
            total = np.zeros(len(rows), np.float64)
            for c in range(part.shape[1]):                  # slot after slot: a serial f64 sum per document
                total = total + part[:, c]
            gap = np.abs(total - ranker._model.leaf_sums(rows))
        gap = gap[np.isfinite(gap)]
        if gap.size:
            worst = max(worst, float(gap.max()))
    if not parts:
        parts, scores = [predict(np.zeros((0, 1), np.float32), cols)[0]], [np.zeros(0, np.float32)]
    matrix, scores = np.concatenate(parts), np.concatenate(scores)
    n_docs = matrix.shape[0]
    logger.info("%d documents, %d features, background of %d rows", n_docs, len(ids), ranker._model.cover_rows())
    if exact:
        logger.info("Exact Shapley values (path-dependent TreeSHAP)")
    logger.info("Largest |sum of contributions - f64 sum of weighted leaf outputs|: %s", java_double_str(worst))
    names = [str(f) for f in ids] + ["rest", "bias"]
    if outFile:
        with open(outFile, "w", encoding="ascii") as out:
            d = 0
            for rl in test:
                for k in range(rl.size()):
                    out.write("%s\t%d\t%s\t%s\n" % (rl.getID(), k, java_float_str(scores[d]),
                                                    "\t".join("%s:%s" % (nm, java_double_str(float(v))) for nm, v in zip(names, matrix[d]))))
                    d += 1
        logger.info("Contributions saved to: %s", outFile)
    lines = summary_lines(ids, matrix) if n_docs else []
    logger.info("feature\tmean |contribution|\tmean contribution")
    for ln in lines:
        logger.info(ln)
    for nm, c in (("rest", len(ids)), ("bias", len(ids) + 1)):
        if n_docs:
            logger.info("%s\t%s\t%s", nm, *[java_double_str(v) for v in _means(matrix[:, c])])
    if summaryFile:
        with open(summaryFile, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in lines))
        logger.info("Summary saved to: %s", summaryFile)
    if pairFile:
        kept, rest = pair_lines(ids, pair_abs, pair_sum, n_docs) if n_docs else ([], [])
        logger.info("feature\tfeature\tmean |interaction|\tmean interaction")
        for ln in kept + rest:
            logger.info(ln)
        logger.info("Largest |sum of a row of interaction values - its exact contribution|: %s", java_double_str(gap_row))
        logger.info("Largest |out[i][j] - out[j][i]|: %s", java_double_str(gap_sym))
        logger.info("Largest |sum of interaction values - f64 sum of weighted leaf outputs|: %s", java_double_str(gap_all))
        with open(pairFile, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in kept))
        logger.info("Interaction values saved to: %s", pairFile)
    return 0


if __name__ == "__main__":
    sys.exit(main())
