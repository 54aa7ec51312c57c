"""python -m ranklib_amd.stages: a LambdaMART / MART model evaluated after every n-th tree on files it was not trained on, in one GPU
pass per file (LambdaMART.stagedScores) -- the learning curve on a test set, under any of the seven metrics, and the
model cut at its best point.  RankLib has this only as the validation roll-back during training (learning/tree/LambdaMART.java:169-272).

  -load model            the model (one)
  -test file             a file to evaluate on (repeatable)
  -metric2T M            the metric (the evaluator's default, ERR@10)
  -step n                stages n, 2n, ... and always the whole model (default 1)
  -norm, -qrel, -gmax, -missingZero, -hr, -device   as in ranklib_amd.evaluator: the files are prepared by the code its -load -test uses
  -curve out             one line per stage: trees <TAB> mean on file 1 [<TAB> mean on file 2 ...], the means as Double.toString
  -save out [-pick i]    the model truncated at the earliest stage with the highest mean on the i-th -test file (default the first)

A file's mean at a stage is the serial f64 sum of its lists' values in list order divided by the list count, as Evaluator.test has it.
"""
import logging
import sys

from ._native import RankLibError
from .evaluator import ArgCursor, Evaluator, common_flag
from .learning import LambdaMART, RankerFactory, RankerType, java_double_str

logger = logging.getLogger("ranklib_amd")


def stage_list(n_trees, step):
    """the tree counts step, 2 step, ... up to n_trees, and always n_trees"""
    if step < 1:
        raise RankLibError("-step must be at least 1 (got %d)" % step)
    if n_trees < 1:
        raise RankLibError("the model has no trees")
    st = list(range(step, n_trees + 1, step))
    if not st or st[-1] != n_trees:
        st.append(n_trees)
    return st


def file_means(values):
    """per stage, the mean of a file's lists: a serial f64 sum in list order, one division (values: [stages][lists])"""
    out = []
    for row in values:
        s = 0.0
        for v in row:
            s += float(v)
        out.append(s / len(row))
    return out


def pick_stage(means):
    """the index of the earliest stage with the highest mean: a later stage replaces an earlier one only when strictly greater"""
    best = 0
    for i in range(1, len(means)):
        if means[i] > means[best]:
            best = i
    return best


def main(argv=None):
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args:
        print("Usage: -load model -test file [-test file ...] [-metric2T M] [-step n] [-norm sum|zscore|linear] [-qrel f] [-gmax g] "
              "[-missingZero] [-hr] [-device d] [-curve out] [-save out [-pick i]]")
        return 0
    models, testFiles = [], []
    metric, step, curveFile, saveFile, pick = "ERR@10", 1, "", "", 1
    Evaluator.mustHaveRelDoc = False
    Evaluator.normalize = False
    Evaluator.qrelFile = ""
    cur = ArgCursor(args)
    nxt = cur.nxt
    for a in cur:
        if a == "-load": models.append(nxt())
        elif a == "-test": testFiles.append(nxt())
        elif a == "-metric2t": metric = nxt()
        elif a == "-step": step = int(nxt())
        elif a == "-curve": curveFile = nxt()
        elif a == "-save": saveFile = nxt()
        elif a == "-pick": pick = int(nxt())
        elif not common_flag(a, nxt):
            cur.unknown()
    if len(models) != 1:
        raise RankLibError("ranklib_amd.stages takes exactly one -load model (got %d)" % len(models))
    if not testFiles:
        raise RankLibError("ranklib_amd.stages needs at least one -test file")
    if not 1 <= pick <= len(testFiles):
        raise RankLibError("-pick %d: there are %d -test files" % (pick, len(testFiles)))
    ranker = RankerFactory().loadRankerFromFile(models[0])
    if not isinstance(ranker, LambdaMART):
        ranker.stagedScores([], None)                       # the refusal, naming the model type
    stages = stage_list(ranker._model.num_trees(), step)
    means, name = [], metric
    for f in testFiles:
        e = Evaluator(RankerType.LAMBDAMART, metric, metric)     # its own scorer per file, as one `-load model -test file` run has
        name = e.testScorer.name()
        test = e.readTestFile(ranker, f)
        means.append(file_means(ranker.stagedScores(test, e.testScorer, stages)))
    lines = ["%d\t%s" % (t, "\t".join(java_double_str(m[s]) for m in means)) for s, t in enumerate(stages)]
    logger.info("trees\t%s", "\t".join("%s on %s" % (name, f) for f in testFiles))
    for ln in lines:
        logger.info(ln)
    if curveFile:
        with open(curveFile, "w", encoding="ascii") as out:
            out.write("".join(ln + "\n" for ln in lines))
        logger.info("Curve saved to: %s", curveFile)
    if saveFile:
        best = pick_stage(means[pick - 1])
        logger.info("Best stage on %s: %d trees (%s = %s)", testFiles[pick - 1], stages[best], name, java_double_str(means[pick - 1][best]))
        ranker.truncated(stages[best]).save(saveFile)
        logger.info("Model saved to: %s", saveFile)
    return 0


if __name__ == "__main__":
    sys.exit(main())
