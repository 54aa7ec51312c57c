"""Host-side mirror of RankLib's plugin surface for the `-ranker 6` path.

Same class and method names, argument meaning and error behaviour as the Java, so code and tests written against
RankLib's API read the same here:

    DataPoint / DenseDataPoint   learning/DataPoint.java:22-200, learning/DenseDataPoint.java:10-51
    RankList                     learning/RankList.java:21-114
    Ranker (abstract)            learning/Ranker.java:36-186
    LambdaMART                   learning/tree/LambdaMART.java:33-329   (init/learn run on the GPU through librlhip.so)
    CoorAscent                   learning/CoorAscent.java:33-396        (learn and eval run on the GPU through librlhip.so)
    AdaRank                      learning/boosting/AdaRank.java:33-346  (learn and eval run on the GPU through librlhip.so)
    LinearRegRank                learning/LinearRegRank.java:23-240     (learn and eval run on the GPU through librlhip.so)
    RankNet / LambdaRank / ListNet   learning/neuralnet/RankNet.java:33-490, LambdaRank.java, ListNet.java:24-236
                                 (model text in and out, eval on the GPU through librlhip.so; all three also train there, each
                                 behind a seed of its own)
    RankerType / RankerFactory   learning/RankerType.java, learning/RankerFactory.java:36-118
    RankerTrainer                learning/RankerTrainer.java:23-56

There is no JVM in this environment; the Java drop-in class that does the same over JNI is in integration/.
All numeric work happens behind the C ABI (ranklib_amd/_native.py); nothing here computes a histogram, a
lambda or a tree on the CPU.
"""
import enum
import random
import logging
import math
import os
import time

import numpy as np

from . import _native as N
from ._native import RankLibError
from .metric import TREE_TRAINABLE, ERRScorer, held_judgments, id_keys, keep_ideals, metric_name

logger = logging.getLogger("ranklib_amd")


# ---------------------------------------------------------------------------------------------------------
class DataPoint:
    """learning/DataPoint.java + DenseDataPoint: `label qid:ID fid:val ... # description`"""
    missingZero = False               # DataPoint.missingZero (static)  learning/DataPoint.java:23
    __slots__ = ("label", "id", "description", "fVals", "cached")

    def __init__(self, text=None):
        self.label = 0.0
        self.id = ""
        self.description = ""
        self.fVals = None
        self.cached = -1.0
        if text is not None:
            self._parse(text)

    def _parse(self, text):           # learning/DataPoint.java:58-110
        try:
            idx = text.find("#")
            if idx != -1:
                self.description = text[idx:]
                text = text[:idx].strip()
            fs = text.split()
            self.label = float(np.float32(fs[0]))
            if self.label < 0:
                raise RankLibError("Relevance label cannot be negative. System will now exit.")
            self.id = fs[1][fs[1].rfind(":") + 1:]
            last = 0
            pairs = []
            for tok in fs[2:]:
                f = int(tok[:tok.index(":")])
                if f <= 0:
                    raise RankLibError("Cannot use feature numbering less than or equal to zero. Start your features at 1.")
                pairs.append((f, np.float32(tok[tok.rfind(":") + 1:])))
                last = max(last, f)
            fv = np.full(last + 1, np.nan, dtype=np.float32)      # fVals[0] is unused, UNKNOWN = NaN
            for f, v in pairs:
                fv[f] = v
            self.fVals = fv
        except RankLibError:
            raise
        except Exception as ex:       # noqa: BLE001 -- the reference wraps everything
            raise RankLibError("Error in DataPoint::parse() %s" % ex)

    @classmethod
    def from_parsed(cls, label, qid, description, fvals):
        """a DataPoint from already parsed fields (features.FeatureManager.readInput's native path)"""
        dp = cls.__new__(cls)
        dp.label = label
        dp.id = qid
        dp.description = description
        dp.fVals = fvals
        dp.cached = -1.0
        return dp

    def getFeatureValue(self, fid):   # learning/DenseDataPoint.java:21-32
        if fid <= 0 or fid >= len(self.fVals):
            if DataPoint.missingZero:
                return np.float32(0)
            raise RankLibError("Error in DenseDataPoint::getFeatureValue(): requesting unspecified feature, fid=%d" % fid)
        v = self.fVals[fid]
        return np.float32(0) if np.isnan(v) else v

    def getFeatureCount(self):
        return len(self.fVals) - 1

    def getLabel(self):
        return self.label

    def getID(self):
        return self.id

    def getDescription(self):
        return self.description

    def toString(self):               # learning/DataPoint.java:188-199, kept as written: the label is cast to int, a cell that is NaN loses
        fv = self.fVals               # its separator too, and the description follows one more space whether it is empty or not
        last = len(fv) - 1
        out = ["%d qid:%s " % (java_float_to_int(self.label), self.id)]
        for i in range(1, last + 1):
            v = fv[i]
            if v == v:
                out.append("%d:%s%s" % (i, java_float_str(v), "" if i == last else " "))
        out.append(" " + self.description)
        return "".join(out)


def java_float_to_int(v):             # (int) of a Java float: NaN is 0, the cast truncates and saturates
    if v != v:
        return 0
    return int(max(-2147483648.0, min(2147483647.0, v)))


DenseDataPoint = DataPoint


class RankList:
    """learning/RankList.java: an ordered list of DataPoints of one query"""

    def __init__(self, rl, idx=None, offset=0):
        pts = rl.rl if isinstance(rl, RankList) else list(rl)
        self.rl = [pts[i - offset] for i in idx] if idx is not None else list(pts)
        self.featureCount = max((dp.getFeatureCount() for dp in self.rl), default=0)

    def getID(self):
        return self.rl[0].getID()

    def size(self):
        return len(self.rl)

    def __len__(self):
        return len(self.rl)

    def get(self, k):
        return self.rl[k]

    def getFeatureCount(self):
        return self.featureCount


def flatten(samples, features):
    """List[RankList] -> (X [n, len(features)] via getFeatureValue, labels, qoff, qkey): what LambdaMART.init()
    walks (learning/tree/LambdaMART.java:71-91); equal qid strings get equal keys (NDCGScorer cache quirk)."""
    n = sum(rl.size() for rl in samples)
    F = len(features)
    X = np.zeros((n, F), np.float32)
    labels = np.zeros(n, np.float32)
    qoff = np.zeros(len(samples) + 1, np.int32)
    qkey = id_keys(rl.getID() for rl in samples)
    fa = np.asarray(features, np.int64)
    k = 0
    for q, rl in enumerate(samples):
        for dp in rl.rl:
            fv = dp.fVals
            if fa.size and (fa.min() <= 0 or fa.max() >= len(fv)):
                X[k] = [dp.getFeatureValue(int(f)) for f in features]
            else:
                row = fv[fa]
                X[k] = np.where(np.isnan(row), np.float32(0), row)
            labels[k] = dp.label
            k += 1
        qoff[q + 1] = k
    return X, labels, qoff, qkey


def dense_rows(dps, need=None, checked=None):
    """The documents dps as f32 rows for the scoring kernels: column f holds feature id f, an unknown cell (NaN) reads 0, and the rows are
    as wide as the longest document and as id need asks.  Unless -missingZero is set a document too short for an id a model reads is
    refused with DenseDataPoint.getFeatureValue's message, by the rule of the model's family.  The tree rankers (checked None) look at
    need alone, the model's largest feature id, name it, and never refuse id 0: a model without features has need == 0.  The linear and
    neural rankers (checked: their feature ids; need: the largest of them) look at every id in order, document by document, refuse
    f <= 0 too and name the first id that fails."""
    if need is None:
        need = max([int(f) for f in checked] + [0])
    width = max([need + 1] + [len(dp.fVals) for dp in dps])
    rows = np.zeros((len(dps), width), np.float32)
    for i, dp in enumerate(dps):
        fv = dp.fVals
        rows[i, :len(fv)] = np.where(np.isnan(fv), np.float32(0), fv)
    if not DataPoint.missingZero:
        for dp in dps:
            n = len(dp.fVals)
            for f in ([need] if checked is None else checked):
                if f >= n or (f <= 0 and checked is not None):
                    raise RankLibError("Error in DenseDataPoint::getFeatureValue(): requesting unspecified feature, fid=%d" % f)
    return rows


def list_chunks(samples, limit):
    """(a, b) index pairs that cut samples into chunks of whole lists samples[a:b] whose f32 rows stay within limit bytes; None: one
    chunk for the whole file.  The rows of a chunk are as wide as its widest list (getFeatureCount() + 1 columns, at least one), a chunk
    always takes its first list, however large, and a further list joins unless that makes (docs + size) * width * 4 > limit: with
    the callers' limit the test reads `> Ranker.EVAL_ROW_BYTES`, not `>=`, so rows that fill the limit exactly stay together."""
    a = 0
    while a < len(samples):
        b, docs, width = a, 0, 1
        while b < len(samples):
            w = max(width, samples[b].getFeatureCount() + 1)
            if limit is not None and b > a and (docs + samples[b].size()) * w * 4 > limit:
                break
            docs, width, b = docs + samples[b].size(), w, b + 1
        yield a, b
        a = b


def result_steps(n_rows, bytes_per_row):
    """(a, b) index pairs that cut n_rows rows into pieces whose results, bytes_per_row each, stay within Ranker.EVAL_ROW_BYTES; a piece
    holds at least one row"""
    step = max(1, Ranker.EVAL_ROW_BYTES // bytes_per_row)
    for a in range(0, n_rows, step):
        yield a, min(a + step, n_rows)


# ---------------------------------------------------------------------------------------------------------
def stable_desc_order(scores):
    """MergeSorter.sort(double[], false): stable, descending (utilities/MergeSorter.java:134-189)"""
    return np.argsort(-np.asarray(scores, np.float64), kind="stable")


class Ranker:
    """learning/Ranker.java:36-186"""

    def __init__(self, samples=None, features=None, scorer=None):
        self.samples = samples if samples is not None else []
        self.features = features
        self.scorer = scorer
        self.scoreOnTrainingData = 0.0
        self.bestScoreOnValidationData = 0.0
        self.validationSamples = None
        self._logbuf = ""

    def setTrainingSet(self, samples):
        self.samples = samples

    def setFeatures(self, features):
        self.features = features

    def setValidationSet(self, samples):
        self.validationSamples = samples

    def setMetricScorer(self, scorer):
        self.scorer = scorer

    def getScoreOnTrainingData(self):
        return self.scoreOnTrainingData

    def getScoreOnValidationData(self):
        return self.bestScoreOnValidationData

    def getFeatures(self):
        return self.features

    def rank(self, rl):               # Ranker.rank(RankList) / rank(List<RankList>)  :88-103
        if isinstance(rl, RankList):
            return RankList(rl, list(stable_desc_order(self.evalList(rl))))
        return [self.rank(x) for x in rl]

    def evalList(self, rl):
        return [self.eval(dp) for dp in rl.rl]

    EVAL_ROW_BYTES = 1 << 30          # evalLists: bytes of f32 rows one scoring call is given at most (whole lists; one list may exceed it)

    def evalLists(self, samples):
        """The scores of every document of every list, list after list: (f64 [n_docs], int64 qoff [len(samples) + 1]).  The documents
        go through _evalDocs in chunks of whole lists whose rows stay under EVAL_ROW_BYTES."""
        qoff = np.zeros(len(samples) + 1, np.int64)
        np.cumsum([rl.size() for rl in samples], out=qoff[1:])
        out = np.zeros(int(qoff[-1]), np.float64)
        for a, b in list_chunks(samples, Ranker.EVAL_ROW_BYTES):
            if qoff[b] > qoff[a]:
                out[int(qoff[a]):int(qoff[b])] = self._evalDocs([dp for rl in samples[a:b] for dp in rl.rl])
        return out, qoff

    def _evalDocs(self, dps):
        """f64 scores of the documents dps; a ranker family overrides it with one call of its scoring kernel"""
        return np.array([self.eval(dp) for dp in dps], np.float64)

    # rlhip: a model after its first t trees.  LambdaMART and MART have stages; bags are not stages, and a linear or
    # neural model has none
    def stagedScores(self, samples, scorer, stages=None):
        raise RankLibError("rlhip: stagedScores needs a LambdaMART or MART model: a %s model has no stages" % self.name())

    def truncated(self, t):
        raise RankLibError("rlhip: truncated needs a LambdaMART or MART model: a %s model has no stages" % self.name())

    # rlhip: per-document feature contributions walk the paths of one ensemble of trees
    def countCover(self, background, accumulate=False):
        raise RankLibError("rlhip: contributions needs a LambdaMART or MART model: a %s model has no trees%s" % (
            self.name(), " of one ensemble: a forest is several ensembles averaged" if self.name() == "Random Forests" else ""))

    def contributions(self, samples, background, features=None, exact=False):
        self.countCover(background)

    def interactions(self, samples, background, features=None):
        self.countCover(background)

    def _askedFeatures(self, features, who, to_do):
        """the feature ids a per-feature method works on, ascending and distinct (None: the model's own); who and to_do word the refusals"""
        feats = sorted({int(f) for f in (self.features if features is None else features)})
        if not feats:
            raise RankLibError("rlhip: %s has no feature to %s" % (who, to_do))
        if feats[0] < 1:
            raise RankLibError("rlhip: %s takes feature ids >= 1 (got %d)" % (who, feats[0]))
        return feats

    # rlhip: permutation feature importance: what a feature is worth under the scorer on these lists
    def permutationImportance(self, samples, scorer, features=None, repeats=5, seed=1, within=False):
        """importance.Importance of features (None: the model's own, ascending) on samples under scorer: per feature and repeat the
        documents receive that feature's value from the document importance.donor_maps names (a permutation of the whole file, or with
        within one inside every list; the same map serves every feature of a repeat), the file is scored and ranked again, and the
        importance is the base mean minus the mean over repeats.  This is the generic path, for every ranker: per cell a permuted copy
        of the documents goes through evalLists and metric.score_lists."""
        from . import importance as I
        from .metric import score_lists
        feats = self._askedFeatures(features, "permutationImportance", "measure")
        donors = I.donor_maps([rl.size() for rl in samples], repeats, seed, within)
        flat, _ = self.evalLists(samples)
        base, _ = score_lists(scorer, samples, flat)
        dps = [dp for rl in samples for dp in rl.rl]
        values = np.zeros((len(feats), repeats, len(samples)), np.float64)
        for c, f in enumerate(feats):
            for r in range(repeats):
                perm = permuted_lists(samples, dps, f, donors[r])
                flat, _ = self.evalLists(perm)
                values[c, r], _ = score_lists(scorer, perm, flat)
        return I.summarize(feats, base, values)

    # rlhip: partial dependence and ICE curves: how the score moves as one feature moves
    def partialDependence(self, samples, features=None, grid=20, ice=False):
        """partial.Partial of features (None: the model's own, ascending) on samples: per feature the grid partial.grid_for gives (grid:
        a count of order statistics, or "thresholds" for a tree model) and per grid value the mean score of the documents with the
        feature set to it, its difference from the base mean and the rms move of a document away from its own score; with ice the
        per-document scores of every cell too.  This is the generic path, for every ranker: per cell a substituted copy of the
        documents goes through evalLists, and the sums take the fixed order of include/rlhip.h (partial.fixed_order_sums)."""
        from . import partial as P
        feats = self._askedFeatures(features, "partialDependence", "vary")
        if not sum(rl.size() for rl in samples):
            raise RankLibError("rlhip: partialDependence needs at least one document")
        grids = [P.grid_for(self, samples, f, grid) for f in feats]
        base, _ = self.evalLists(samples)
        mean, shift2, curves = [], [], []
        for f, g in zip(feats, grids):
            sc = np.stack([self.evalLists(substituted_lists(samples, f, v))[0] for v in g])
            sums = [P.fixed_order_sums(s, base) for s in sc]
            mean.append(np.array([s1 for s1, _ in sums], np.float64) / float(len(base)))
            shift2.append(np.array([s2 for _, s2 in sums], np.float64) / float(len(base)))
            curves.append(sc)
        return P.summarize(feats, grids, base, mean, shift2, curves if ice else None)

    def save(self, modelFile):        # :106-122
        d = modelFile.rsplit("/", 1)[0] if "/" in modelFile else None
        if d:
            import os
            os.makedirs(d, exist_ok=True)
        with open(modelFile, "w", encoding="ascii") as f:
            f.write(self.model())

    # fixed-width log table  learning/Ranker.java:124-155
    def printLog(self, lens, msgs):
        for ln, msg in zip(lens, msgs):
            self._logbuf += (msg[:ln] if len(msg) > ln else msg + " " * (ln - len(msg))) + " | "

    def printLogLn(self, lens, msgs):
        self.printLog(lens, msgs)
        self.flushLog()

    def flushLog(self):
        if self._logbuf:
            logger.info(self._logbuf)
            self._logbuf = ""

    def init(self):
        raise NotImplementedError

    def learn(self):
        raise NotImplementedError

    def eval(self, p):                # noqa: A003 -- RankLib's name
        return -1.0

    def createNew(self):
        raise NotImplementedError

    def model(self):
        raise NotImplementedError

    def loadFromString(self, fullText):
        raise NotImplementedError

    def name(self):
        raise NotImplementedError

    def printParameters(self):
        raise NotImplementedError


def permuted_lists(samples, dps, fid, donor):
    """samples with feature fid of document i (dps[i], the documents in file order) taken from document donor[i]: new lists of new
    DataPoints, everything else shared.  A document without the feature donates the unknown value (NaN, which reads as 0)."""
    out, i = [], 0
    for rl in samples:
        pts = []
        for dp in rl.rl:
            src = dps[int(donor[i])].fVals
            fv = np.full(max(len(dp.fVals), fid + 1), np.nan, np.float32)
            fv[:len(dp.fVals)] = dp.fVals
            fv[fid] = src[fid] if fid < len(src) else np.nan
            pts.append(DataPoint.from_parsed(dp.label, dp.id, dp.description, fv))
            i += 1
        out.append(RankList(pts))
    return out


def substituted_lists(samples, fid, value):
    """samples with feature fid of every document set to value: new lists of new DataPoints, everything else shared.  A document too
    short for the feature is widened with the unknown value (NaN, which reads as 0)."""
    out = []
    for rl in samples:
        pts = []
        for dp in rl.rl:
            fv = np.full(max(len(dp.fVals), fid + 1), np.nan, np.float32)
            fv[:len(dp.fVals)] = dp.fVals
            fv[fid] = value
            pts.append(DataPoint.from_parsed(dp.label, dp.id, dp.description, fv))
        out.append(RankList(pts))
    return out


def java_round(val, n):               # utilities/SimpleMath.java:54-60
    p = 10 ** n
    return math.floor(val * p + .5) / p


class FeatureHistogram:
    """Only the process-global knob of learning/tree/FeatureHistogram.java:34 lives on the host: the fraction of the features
    every split attempt looks at (set by RFRanker.init, never restored -- like the Java static)."""
    samplingRate = 1.0
    seed = 0          # not in the Java (it draws from an unseeded Random): makes the draw reproducible, see rlhip.h rl_params.seed


RESUME_NOT_BAGS = ("rlhip: -resume / -checkpoint continue one LambdaMART (-ranker 6) or MART (-ranker 0) run; the bags of Random Forests "
                   "(-ranker 8) are trainers of their own and are not built for it")
REFIT_NOT_BAGS = ("rlhip: -refit recomputes the leaf values of one LambdaMART (-ranker 6) or MART (-ranker 0) model; the bags of Random Forests "
                  "(-ranker 8) are trainers of their own and are not built for it")


class LambdaMART(Ranker):
    """learning/tree/LambdaMART.java with init()/learn() executed on an MI355X (librlhip.so)."""
    # process-global parameters, like the Java statics (:37-42)
    nTrees = 1000
    learningRate = 0.1
    nThreshold = 256
    nRoundToStopEarly = 100
    nTreeLeaves = 10
    minLeafSupport = 1
    device = 0
    fastLeaf = False          # not in the Java (-fastleaf): leaf sums as the fixed f64 reduction of RL_FLAG_FAST_LEAF instead of the float running
                              # sums of :401-408; inherited by MART and, through these classes, by the bags of Random Forests
    # not in the Java either (-resume / -checkpoint): the text of a saved model whose trees become this run's first rounds (nTrees stays
    # the TOTAL number of trees); a file that receives model() of all trees so far -- not rolled back -- after every checkpointEvery-th round.  A run
    # resumed from such a checkpoint is the uninterrupted run bit for bit; resumed from a FINAL model, which was rolled back to its best validation
    # prefix, it restarts early stopping from that prefix -- a legitimate "train further", not the uninterrupted run
    resumeFrom = None
    checkpointFile = None
    checkpointEvery = 100
    # -refit / -decay: the text of a saved model whose trees keep their structure and get new leaf values from this run's training data
    # -- stored output = refitDecay * old + (1 - refitDecay) * new, in [0, 1); 0: the new values alone -- as this run's first rounds; nTrees stays the
    # TOTAL: equal to the model's tree count the run only refits, larger it trains further behind the refit trees
    refitFrom = None
    refitDecay = 0.0
    _RANKER = "LAMBDAMART"

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self.ensemble = None          # list of FlatTree (pre-order) after learn(); scoring model after loadFromString
        self.impacts = None
        self._trainer = None
        self._model = None
        self._model_text = None

    def init(self):                   # :68-166
        logger.info("Initializing... ")
        metric = metric_name(self.scorer) if self.scorer is not None else None
        if metric not in TREE_TRAINABLE:
            raise RankLibError("rlhip: the train metric must be one of NDCG, DCG, MAP, ERR, P, RR (got %s)" % (self.scorer.name() if self.scorer else None))
        cls = type(self)
        self.impacts = np.zeros(len(self.features))
        train = flatten(self.samples, self.features)          # before the trainer exists, as ever: a row that cannot be read is refused first
        N.set_err_max(ERRScorer.MAX)              # the reference's static ERRScorer.MAX (-gmax) reaches the kernels through the library's static
        t = N.Trainer(n_trees=cls.nTrees, n_leaves=cls.nTreeLeaves, learning_rate=cls.learningRate, n_threshold=cls.nThreshold,
                      min_leaf_support=cls.minLeafSupport, early_stop_rounds=cls.nRoundToStopEarly, metric_k=self.scorer.getK(),
                      device=cls.device, metric=metric, ranker=self._RANKER, flags=N.RL_FLAG_FAST_LEAF if cls.fastLeaf else 0,
                      feature_sampling_rate=FeatureHistogram.samplingRate, seed=FeatureHistogram.seed)
        feed_trainer(self, t, metric, lambda lists: train if lists is self.samples else flatten(lists, self.features), feature_ids=self.features)
        t.init()
        self._resumed, self._resume_stop = 0, False
        if cls.resumeFrom is not None:
            self._resume_stop = t.adopt_model_text(cls.resumeFrom)
            self._resumed = t.num_trees()
        if cls.refitFrom is not None:      # the refit rounds are printed and continued like adopted ones (learn)
            if cls.resumeFrom is not None:
                raise RankLibError("rlhip: refitFrom together with resumeFrom: a model is either adopted as it is or refitted")
            self._resume_stop = t.refit_model_text(cls.refitFrom, cls.refitDecay)
            self._resumed = t.num_trees()
        self._trainer = t

    def _logRound(self, m, tm, vm):
        self.printLog([7], [str(m + 1)])
        self.printLog([9], [java_double_str(java_round(float(tm), 4))])
        if vm is not None:
            self.printLog([9], [java_double_str(java_round(float(vm), 4))])
        self.flushLog()

    def _writeCheckpoint(self, t):
        """all trees so far, complete or not at all: the text goes to a file beside the checkpoint and is moved over it in one step"""
        cls = type(self)
        tmp = cls.checkpointFile + ".tmp"
        with open(tmp, "w", encoding="ascii") as f:
            f.write(t.model_text())
        os.replace(tmp, cls.checkpointFile)

    def learn(self):                  # :169-272
        cls = type(self)
        t = self._trainer
        logger.info("Training starts...")
        nm = self.scorer.name()
        if self.validationSamples is not None:
            self.printLogLn([7, 9, 9], ["#iter", nm + "-T", nm + "-V"])
        else:
            self.printLogLn([7, 9], ["#iter", nm + "-T"])
        resumed = getattr(self, "_resumed", 0)
        for m in range(resumed):      # the adopted rounds' lines, as the run that grew them printed them (refit rounds: from rl_get_round_metrics too)
            self._logRound(m, *t.round_metrics(m))
        for m in range(resumed, 0 if getattr(self, "_resume_stop", False) else cls.nTrees):
            _, tm, vm, stop = t.boost_round(want_tree=False)
            self._logRound(m, tm, vm)
            if cls.checkpointFile and (m + 1) % cls.checkpointEvery == 0:
                self._writeCheckpoint(t)
            if stop:
                break
        ts, vs = t.finish()           # rollback to the best validation model + scorer.score(rank(samples))
        self.scoreOnTrainingData = ts
        logger.info("Finished sucessfully.")
        logger.info("%s on training data: %s", nm, java_round(ts, 4))
        if vs is not None:
            self.bestScoreOnValidationData = vs
            logger.info("%s on validation data: %s", nm, java_round(vs, 4))
        self.ensemble = [t.get_tree(i) for i in range(t.num_trees())]
        self._model_text = t.model_text()
        self._model = N.Model(self._model_text, cls.device)
        logger.info("-- FEATURE IMPACTS")          # impacts[] is never written in the reference either (:58,80,267-271)
        for i, f in enumerate(self.features):
            logger.info(" Feature %d reduced error %s", f, self.impacts[i])

    # --- scoring: Ensemble.eval (float accumulation) on the GPU -------------------------------------------
    def _rows(self, dps):
        return dense_rows(dps, int(max(self._model.features(), default=0)))

    def eval(self, dp):               # noqa: A003  :275-277
        return float(self._model.predict_rows(self._rows([dp]))[0])

    def evalList(self, rl):
        return [float(v) for v in self._model.predict_rows(self._rows(rl.rl))]

    def _evalDocs(self, dps):
        return self._model.predict_rows(self._rows(dps)).astype(np.float64)

    # --- stages: the model after its first t trees (rlhip) ---------------------------------------
    def stagedScores(self, samples, scorer, stages=None):
        """scorer's value of every list of samples under the model's first t trees, for every t of stages (tree counts, strictly
        increasing; None: every tree): f64 [len(stages)][len(samples)], row i what metric.score_lists gives for truncated(stages[i]),
        bit for bit.  One _native.Model.eval_stages call per chunk of whole lists whose rows stay under EVAL_ROW_BYTES; what the scorer
        holds is resolved per list id exactly as score_lists does it, and the ideal DCGs the calls computed are written back into
        idealGains.  A (stage, list) cell whose scores hold a NaN is filled on the host: predict_stages on that list's rows, then the
        per-list path of score_lists.  Lists longer than metric.EVAL_HOST_LEN stay on the device (both paths give the same bits; the
        host's would cost one sort per stage)."""
        st = np.arange(1, self._model.num_trees() + 1, dtype=np.int32) if stages is None else np.ascontiguousarray(stages, dtype=np.int32)
        name = metric_name(scorer)
        out = np.zeros((st.size, len(samples)), np.float64)
        for a, b in list_chunks(samples, Ranker.EVAL_ROW_BYTES):
            empty, dev, rows, dq, labels, ids = self._devChunk(samples, a, b)
            for q in empty:                                  # the scorer's own answer, whatever the stage
                out[:, q] = scorer.score(samples[q])
            if not dev:
                continue
            qkey, ideal, rdc = held_judgments(scorer, name, ids)
            vals, nan, used = self._model.eval_stages(rows, labels, dq, name, scorer.k, st, err_max=ERRScorer.MAX, qkey=qkey,
                                                      ideal_dcg=ideal, rel_doc_count=rdc)
            out[:, dev] = vals
            keep_ideals(scorer, name, ids, used)
            for j in np.flatnonzero(nan.any(axis=0)):
                which = np.flatnonzero(nan[:, j])
                sc = self._model.predict_stages(rows[int(dq[j]):int(dq[j + 1])], st[which])
                for r, s in enumerate(which):
                    order = stable_desc_order(sc[r].astype(np.float64))
                    out[s, dev[j]] = scorer.score(RankList(samples[dev[j]], list(order)))
        return out

    def _devChunk(self, samples, a, b):
        """What one device call over the lists samples[a:b] takes: (empty, the indices of the lists without a document, which the kernels
        do not take; dev, the indices of the others; rows, their documents; dq, the int64 offsets of the lists of dev into rows; the
        documents' labels; ids, the id of every list of dev).  Without a list for the device everything after dev is None."""
        empty = [q for q in range(a, b) if not samples[q].size()]
        dev = [q for q in range(a, b) if samples[q].size()]
        if not dev:
            return empty, dev, None, None, None, None
        rows = self._rows([dp for q in dev for dp in samples[q].rl])
        dq = np.concatenate([[0], np.cumsum([samples[q].size() for q in dev])]).astype(np.int64)
        labels = np.fromiter((dp.label for q in dev for dp in samples[q].rl), np.float32, count=int(dq[-1]))
        return empty, dev, rows, dq, labels, [samples[q].getID() for q in dev]

    # --- permutation importance in one pass (rlhip) ----------------------------------------------
    def permutationImportance(self, samples, scorer, features=None, repeats=5, seed=1, within=False):
        """Ranker.permutationImportance, bit for bit, without a permuted copy per cell: every (feature, repeat) cell and the base are
        walked, ranked and scored by _native.Model.eval_permuted.  Without within a document's donor may be any document of the file,
        so every list's donor rows have to be in the call: ONE call takes the whole file, whatever EVAL_ROW_BYTES says.  With within
        the donors stay in their lists and the file goes in chunks of whole lists whose rows stay under EVAL_ROW_BYTES.  What the scorer
        holds is resolved per list id as score_lists does it.  A cell whose scores hold a NaN is filled on the host, as stagedScores
        fills a stage: that list's permuted rows through predict_rows, then the per-list path of score_lists."""
        from . import importance as I
        feats = self._askedFeatures(features, "permutationImportance", "measure")
        cols = np.array(feats, np.int32)
        sizes = [rl.size() for rl in samples]
        donors = I.donor_maps(sizes, repeats, seed, within)
        doc0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        name = metric_name(scorer)
        base = np.zeros(len(samples), np.float64)
        values = np.zeros((len(feats), repeats, len(samples)), np.float64)
        for a, b in list_chunks(samples, Ranker.EVAL_ROW_BYTES if within else None):
            empty, dev, rows, dq, labels, ids = self._devChunk(samples, a, b)
            for q in empty:                                  # the scorer's own answer, whatever the cell
                base[q] = values[:, :, q] = scorer.score(samples[q])
            if not dev:
                continue
            don = donors[:, int(doc0[a]):int(doc0[b])] - np.int32(doc0[a])      # (empty lists hold no document: the chunk's rows are contiguous)
            qkey, ideal, rdc = held_judgments(scorer, name, ids)
            bv, bnan, vals, nan, used = self._model.eval_permuted(rows, labels, dq, name, scorer.k, cols, don, err_max=ERRScorer.MAX,
                                                                  qkey=qkey, ideal_dcg=ideal, rel_doc_count=rdc)
            base[dev] = bv
            values[:, :, dev] = vals
            keep_ideals(scorer, name, ids, used)

            def on_host(j, c, r):
                lo, hi = int(dq[j]), int(dq[j + 1])
                part = rows[lo:hi].copy()
                if c is not None and feats[c] < rows.shape[1]:
                    part[:, feats[c]] = rows[don[r, lo:hi], feats[c]]
                order = stable_desc_order(self._model.predict_rows(part).astype(np.float64))
                return scorer.score(RankList(samples[dev[j]], list(order)))
            for j in np.flatnonzero(bnan):
                base[dev[j]] = on_host(j, None, 0)
            for c, r, j in np.argwhere(nan):
                values[c, r, dev[j]] = on_host(j, c, r)
        return I.summarize(feats, base, values)

    # --- partial dependence in one pass (rlhip) --------------------------------------------------
    def partialDependence(self, samples, features=None, grid=20, ice=False):
        """Ranker.partialDependence, bit for bit, without a substituted copy per cell: every (feature, grid value) cell and the base are
        walked and summed by _native.Model.predict_partial.  A mean does not split over calls, so ONE call takes the whole file,
        whatever EVAL_ROW_BYTES says, as permutationImportance does without within."""
        from . import partial as P
        feats = self._askedFeatures(features, "partialDependence", "vary")
        dps = [dp for rl in samples for dp in rl.rl]
        if not dps:
            raise RankLibError("rlhip: partialDependence needs at least one document")
        grids = [P.grid_for(self, samples, f, grid) for f in feats]
        base, mean, shift2, sc = self._model.predict_partial(self._rows(dps), feats, grids, ice=ice)
        off = np.concatenate([[0], np.cumsum([len(g) for g in grids])]).astype(np.int64)
        cut = lambda a: [a[int(off[c]):int(off[c + 1])] for c in range(len(feats))]      # noqa: E731
        return P.summarize(feats, grids, base.astype(np.float64), cut(mean), cut(shift2), cut(sc.astype(np.float64)) if ice else None)

    # --- per-document feature contributions (rlhip) ----------------------------------------------
    def _rowChunks(self, samples):
        """the documents of samples as rows, in chunks of whole lists whose rows stay under EVAL_ROW_BYTES"""
        for a, b in list_chunks(samples, Ranker.EVAL_ROW_BYTES):
            dps = [dp for q in range(a, b) for dp in samples[q].rl]
            if dps:
                yield self._rows(dps)

    def countCover(self, background, accumulate=False):
        """count, per node, the documents of `background` whose walk visits it (_native.Model.cover): RankLib's model text holds no node
        counts, so the node values contributions() works with come from a background file, usually the training file.  accumulate: add
        to the counts of earlier calls."""
        if not accumulate:
            self._model.cover(np.zeros((0, 1), np.float32))
        for rows in self._rowChunks(background):
            self._model.cover(rows, accumulate=True)

    def contributions(self, samples, background, features=None, exact=False):
        """Which features put a document where it is: (f64 [documents of samples in file order][C + 2], the C feature ids).  Column c
        holds what feature ids[c] contributes to every document's score, column C what the features not asked for contribute, column
        C + 1 the bias -- Saabas path attribution over node values averaged with the covers of `background` (None: the counts of earlier
        countCover calls).  features None: every feature the model splits on.  A row sums to the f64 sum of the document's weighted leaf
        outputs: the model's score up to the float rounding of Ensemble.eval's chain, not its bits.  One _native.Model.predict_contribs
        call per chunk of whole lists whose rows stay under EVAL_ROW_BYTES.  exact: the Shapley values themselves, path-dependent
        TreeSHAP (_native.Model.predict_shap), in the same layout: consistent where Saabas' attribution depends on which
        feature sits higher in a tree, at about two orders of magnitude more work."""
        if background is not None:
            self.countCover(background)
        cols = None if features is None else [int(f) for f in features]
        ids = [int(f) for f in self._model.features()] if cols is None else cols
        predict = self._model.predict_shap if exact else self._model.predict_contribs
        parts = [predict(rows, cols)[0] for rows in self._rowChunks(samples)]
        if not parts:                                        # no document: the library still checks the columns and that covers exist
            parts = [predict(np.zeros((0, 1), np.float32), cols)[0]]
        return np.concatenate(parts), ids

    def _interactionChunks(self, samples, n_slots):
        """the row chunks of _rowChunks cut again so that a chunk's result [rows][n_slots][n_slots] f64 stays under EVAL_ROW_BYTES
        (a chunk holds at least one row)"""
        for rows in self._rowChunks(samples):
            for a, b in result_steps(len(rows), 8 * n_slots * n_slots):
                yield rows[a:b]

    def interactions(self, samples, background, features=None):
        """Which features work together: (f64 [documents of samples in file order][C + 2][C + 2], the C feature ids) -- SHAP
        interaction values, XGBoost's pred_interactions (_native.Model.predict_interactions), over the covers of
        `background` (None: the counts of earlier countCover calls).  features None: every feature the model splits on.  Cell [i][j],
        i != j, is the joint effect of features ids[i] and ids[j], [i][i] what is left of feature i's exact contribution
        (contributions(exact=True)) when its row's other cells are taken away, row and column C what the features not asked for do,
        [C + 1][C + 1] the bias.  The rows go in chunks whose result stays under EVAL_ROW_BYTES."""
        if background is not None:
            self.countCover(background)
        cols = None if features is None else [int(f) for f in features]
        ids = [int(f) for f in self._model.features()] if cols is None else cols
        parts = [self._model.predict_interactions(rows, cols)[0] for rows in self._interactionChunks(samples, len(ids) + 2)]
        if not parts:                                        # no document: the library still checks the columns and that covers exist
            parts = [self._model.predict_interactions(np.zeros((0, 1), np.float32), cols)[0]]
        return np.concatenate(parts), ids

    def truncated(self, t):
        """a ranker of this class holding the first t trees: its model text is truncate_model_text(model(), t)"""
        r = self.createNew()
        r.loadFromString(truncate_model_text(self._model_text, t))
        return r

    def createNew(self):
        return LambdaMART()

    def toString(self):
        return self.model().split("\n\n", 1)[1]

    def model(self):                  # :290-301
        return self._model_text

    def loadFromString(self, fullText):   # :304-310
        self._model_text = fullText
        self._model = N.Model(fullText, type(self).device)
        self.features = [int(f) for f in self._model.features()]

    def name(self):
        return "LambdaMART"

    def getEnsemble(self):
        return self.ensemble

    def printParameters(self):        # :313-320
        cls = type(self)
        logger.info("No. of trees: %d", cls.nTrees)
        logger.info("No. of leaves: %d", cls.nTreeLeaves)
        logger.info("No. of threshold candidates: %d", cls.nThreshold)
        logger.info("Min leaf support: %d", cls.minLeafSupport)
        logger.info("Learning rate: %s", cls.learningRate)
        logger.info("Stop early: %d rounds without performance gain on validation data", cls.nRoundToStopEarly)


class MART(LambdaMART):
    """learning/tree/MART.java: LambdaMART with residual pseudo-responses and mean leaf outputs ("Inherits *ALL*
    parameters from LambdaMART": the class attributes above are shared, like the Java statics)."""
    _RANKER = "MART"

    def createNew(self):              # :36-39
        return MART()

    def name(self):                   # :41-44
        return "MART"


def truncate_model_text(text, t):
    """The text of a LambdaMART / MART model cut after its first t trees: everything before the first <tree> element as it stands (every
    `##` line verbatim) with one comment line `## rlhip: first t of T trees` behind the last `##` line of that header, the first t <tree>
    elements byte for byte, then </ensemble>.  t outside [1, T] is refused."""
    import re
    starts = [m.start() for m in re.finditer(r"^[ \t]*<tree\b", text, re.M)]
    ends = [m.end() for m in re.finditer(r"</tree>[ \t]*\r?\n?", text)]
    T = len(starts)
    if T == 0 or len(ends) != T:
        raise RankLibError("rlhip: truncated needs the text of a tree ensemble (found %d <tree> and %d </tree>)" % (T, len(ends)))
    if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 1 or t > T:
        raise RankLibError("rlhip: truncated(t) takes 1 <= t <= %d, the model's trees (got %r)" % (T, t))
    head = text[:starts[0]].splitlines(keepends=True)
    at = max([i + 1 for i, ln in enumerate(head) if ln.startswith("##")], default=0)
    head.insert(at, "## rlhip: first %d of %d trees\n" % (t, T))
    return "".join(head) + text[starts[0]:ends[int(t) - 1]] + "</ensemble>\n"


def java_double_str(v):
    """Double.toString of a Java double (score files, indri files, the per-round log table): shortest digits that round-trip (JDK >= 19),
    decimal notation for 1e-3 <= |v| < 1e7, computerised scientific notation ("1.0E-5") otherwise; repr() switches at 1e-4 / 1e16."""
    d = float(v)
    if d != d:
        return "NaN"
    if d in (float("inf"), float("-inf")):
        return "Infinity" if d > 0 else "-Infinity"
    if d == 0:
        return "-0.0" if math.copysign(1.0, d) < 0 else "0.0"
    a = abs(d)
    if 1e-3 <= a < 1e7:
        r = np.format_float_positional(np.float64(d), unique=True, trim="0")
        return r if "." in r else r + ".0"
    m, e = np.format_float_scientific(np.float64(d), unique=True, trim="0").split("e")
    return (m if "." in m else m + ".0") + "E" + str(int(e))


def java_float_str(v):
    """Float.toString of a Java float (header lines of the model files): shortest digits that round-trip, decimal notation for
    1e-3 <= |v| < 1e7, computerised scientific notation otherwise."""
    f = np.float32(v)
    if f == 0:
        return "-0.0" if np.signbit(f) else "0.0"
    a = abs(float(f))
    if a == math.inf:                 # (a feature value may be one: DataPoint.toString)
        return "Infinity" if f > 0 else "-Infinity"
    if 1e-3 <= a < 1e7:
        r = np.format_float_positional(f, unique=True, trim="0")
        return r if "." in r else r + ".0"
    m, e = np.format_float_scientific(f, unique=True, trim="0").split("e")
    return (m if "." in m else m + ".0") + "E" + str(int(e))


class Sampler:
    """learning/Sampler.java:25-68.  The Java draws from an unseeded java.util.Random; `seed` makes the bags reproducible."""

    def __init__(self, seed=None):
        self.rng = random.Random(seed)
        self.samples = None
        self.remains = None

    def doSampling(self, samplingPool, samplingRate, withReplacement):
        n = len(samplingPool)
        size = int(np.float32(samplingRate) * np.float32(n))          # (int) (samplingRate * samplingPool.size()), float arithmetic
        self.samples = []
        if withReplacement:
            used = [False] * n
            for _ in range(size):
                sel = self.rng.randrange(n)
                self.samples.append(samplingPool[sel])
                used[sel] = True
            self.remains = [samplingPool[i] for i in range(n) if not used[i]]
        else:
            pool = list(range(n))
            for _ in range(size):
                sel = self.rng.randrange(len(pool))
                self.samples.append(samplingPool[pool[sel]])
                del pool[sel]
            self.remains = [samplingPool[i] for i in pool]
        return self.samples

    def getSamples(self):
        return self.samples

    def getRemains(self):
        return self.remains


class RFRanker(Ranker):
    """learning/tree/RFRanker.java: bagging over MART / LambdaMART trained on the GPU.  Every bag is a sample of the training
    lists WITH replacement (Sampler), trained with feature sampling at every split attempt (FeatureHistogram.samplingRate);
    eval = mean over the bags of Ensemble.eval (:109-115)."""
    nBag = 300
    subSamplingRate = 1.0
    featureSamplingRate = 0.3
    rType = None                      # RankerType.MART, set below (the enum is defined after this class)
    nTrees = 1
    nTreeLeaves = 100
    learningRate = 0.1
    nThreshold = 256
    minLeafSupport = 1
    seed = 0                          # not in the Java: bag i samples with Random(mix(seed, i)) and draws features with the same seed

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self.ensembles = None         # per bag: the "<ensemble>...</ensemble>\n" text (Ensemble.toString)
        self._models = None           # per bag: N.Model for scoring

    @staticmethod
    def bag_seed(seed, i):
        return (int(seed) * 0x9E3779B97F4A7C15 + (i + 1) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF

    def init(self):                   # :57-69 -- overwrites LambdaMART's statics and never restores them, like the Java
        logger.info("Initializing... ")
        cls = type(self)
        if LambdaMART.resumeFrom is not None or LambdaMART.checkpointFile:
            raise RankLibError(RESUME_NOT_BAGS)
        if LambdaMART.refitFrom is not None:
            raise RankLibError(REFIT_NOT_BAGS)
        self.ensembles = [None] * cls.nBag
        LambdaMART.nTrees = cls.nTrees
        LambdaMART.nTreeLeaves = cls.nTreeLeaves
        LambdaMART.learningRate = cls.learningRate
        LambdaMART.nThreshold = cls.nThreshold
        LambdaMART.minLeafSupport = cls.minLeafSupport
        LambdaMART.nRoundToStopEarly = -1          # no early stopping inside a bag
        FeatureHistogram.samplingRate = cls.featureSamplingRate

    def learn(self):                  # :72-107
        cls = type(self)
        rf = RankerFactory()
        logger.info("Training starts...")
        nm = self.scorer.name()
        self.printLogLn([9, 9, 11], ["bag", nm + "-B", nm + "-OOB"])
        impacts = None
        self._models = []
        for i in range(cls.nBag):
            bs = self.bag_seed(cls.seed, i)
            sp = Sampler(bs)
            bag = sp.doSampling(self.samples, cls.subSamplingRate, True)
            FeatureHistogram.seed = bs
            r = rf.createRanker(cls.rType, bag, self.features, self.scorer)
            r.init()
            r.learn()
            impacts = r.impacts if impacts is None else impacts + r.impacts
            self.printLogLn([9, 9], ["b[%d]" % (i + 1), java_double_str(java_round(r.getScoreOnTrainingData(), 4))])
            self.ensembles[i] = r.toString()
            self._models.append(r._model)
        self.scoreOnTrainingData = self.scorer.score(self.rank(self.samples))
        logger.info("Finished sucessfully.")
        logger.info("%s on training data: %s", nm, java_round(self.scoreOnTrainingData, 4))
        if self.validationSamples is not None:
            self.bestScoreOnValidationData = self.scorer.score(self.rank(self.validationSamples))
            logger.info("%s on validation data: %s", nm, java_round(self.bestScoreOnValidationData, 4))
        logger.info("-- FEATURE IMPACTS")
        for i, f in enumerate(self.features):
            logger.info(" Feature %d reduced error %s", f, impacts[i])

    def evalList(self, rl):
        return [float(v) for v in self._evalDocs(rl.rl)]

    def _evalDocs(self, dps):         # :109-115 for every document at once: double s += (float) ensemble.eval; s / nBag
        rows = dense_rows(dps, max(int(max(m.features(), default=0)) for m in self._models))
        s = np.zeros(len(rows), np.float64)
        for m in self._models:
            s += m.predict_rows(rows).astype(np.float64)
        return s / len(self._models)

    def eval(self, dp):               # noqa: A003
        return self.evalList(RankList([dp]))[0]

    def createNew(self):
        return RFRanker()

    def toString(self):               # :122-128
        return "".join(e + "\n" for e in self.ensembles)

    def model(self):                  # :131-143
        cls = type(self)
        out = "## " + self.name() + "\n"
        out += "## No. of bags = %d\n" % cls.nBag
        out += "## Sub-sampling = %s\n" % java_float_str(cls.subSamplingRate)
        out += "## Feature-sampling = %s\n" % java_float_str(cls.featureSamplingRate)
        out += "## No. of trees = %d\n" % cls.nTrees
        out += "## No. of leaves = %d\n" % cls.nTreeLeaves
        out += "## No. of threshold candidates = %d\n" % cls.nThreshold
        out += "## Learning rate = %s\n" % java_float_str(cls.learningRate)
        out += "\n"
        return out + self.toString()

    @staticmethod
    def ensembleBlocks(fullText):
        """the "<ensemble> ... </ensemble>" blocks of a Random Forests model text, one per bag, in file order (no device is needed: what
        loadFromString reads, and all the Combiner needs)"""
        text = "\n".join(ln for ln in fullText.split("\n") if not ln.startswith("##"))       # parsing/ModelLineProducer.java:43-78
        blocks = []
        pos = 0
        while True:
            a = text.find("<ensemble>", pos)
            if a < 0:
                break
            b = text.find("</ensemble>", a)
            if b < 0:
                raise RankLibError("Error in RFRanker::load(): unterminated <ensemble>")
            blocks.append(text[a:b + len("</ensemble>")])
            pos = b + len("</ensemble>")
        if not blocks:
            raise RankLibError("Error in RFRanker::load(): no <ensemble> in the model")
        return blocks

    def loadFromString(self, fullText):   # :146-178: every "<ensemble> ... </ensemble>" block is one bag
        blocks = self.ensembleBlocks(fullText)
        self.ensembles = [blk + "\n" for blk in blocks]
        self._models = [N.Model("## LambdaMART\n\n" + blk + "\n", LambdaMART.device) for blk in blocks]
        feats = []
        for m in self._models:                  # insertion-ordered set (the Java uses a HashSet: iteration order unspecified)
            for f in m.features():
                if int(f) not in feats:
                    feats.append(int(f))
        self.features = feats

    def name(self):
        return "Random Forests"

    def getEnsembles(self):
        return self.ensembles

    def printParameters(self):        # :181-189
        cls = type(self)
        logger.info("No. of bags: %d", cls.nBag)
        logger.info("Sub-sampling: %s", java_float_str(cls.subSamplingRate))
        logger.info("Feature-sampling: %s", java_float_str(cls.featureSamplingRate))
        logger.info("No. of trees: %d", cls.nTrees)
        logger.info("No. of leaves: %d", cls.nTreeLeaves)
        logger.info("No. of threshold candidates: %d", cls.nThreshold)
        logger.info("Learning rate: %s", java_float_str(cls.learningRate))


def feed_trainer(ranker, t, metric, flat=None, **train_args):
    """The training / validation lists of a ranker into its trainer t (the tree trainer, or one of the linear and neural ones), with the
    NDCG ideal-DCG keys shared across the two sets: a validation list whose id the training set holds takes that id's key, the others
    continue after the training keys.  Then what the scorer object already holds reaches the trainer list by list: idealGains entries
    (-qrel, NDCGScorer.java:50-96 -- or any earlier use of the same scorer object: a cached entry is a cached entry), sent only when
    there is one, and relDocCount (-qrel, APScorer.java:45-66).  flat: the ranker's own flatten(samples) where the columns are not the
    feature list's (LinearRegRank); train_args: further arguments of t.set_train (the tree trainer's feature_ids)."""
    if flat is None:
        flat = lambda lists: flatten(lists, ranker.features)      # noqa: E731
    X, lab, qoff, qkey = flat(ranker.samples)
    nk = int(qkey.max()) + 1 if len(qkey) else 0
    t.set_train(X, lab, qoff, qkey=qkey, **train_args)
    if ranker.validationSamples is not None:
        Xv, lv, qv, _ = flat(ranker.validationSamples)
        ids = {}
        for q, rl in enumerate(ranker.samples):
            ids.setdefault(rl.getID(), int(qkey[q]))
        vkey = np.array([ids.setdefault(rl.getID(), nk + i) for i, rl in enumerate(ranker.validationSamples)], np.int32)
        t.set_validation(Xv, lv, qv, qkey=vkey)
    for validation, lists in ((False, ranker.samples), (True, ranker.validationSamples)):
        if lists is None:
            continue
        _, ideal, rdc = held_judgments(ranker.scorer, metric, [rl.getID() for rl in lists])
        if not getattr(ranker.scorer, "idealGains", None):       # where a scoring call sends an array of NaN, a trainer is sent nothing
            ideal = None
        if ideal is not None or rdc is not None:
            t.set_external_judgments(validation, ideal, rdc)


def _key_value_line(fullText):
    """The first non-empty line that is not "##", split by utilities/KeyValuePair.java into (keys, values)"""
    line = None
    for content in fullText.splitlines():
        content = content.strip()
        if not content or content.startswith("##"):
            continue
        line = content
        break
    idx = line.rfind("#")
    if idx != -1:
        line = line[:idx].strip()
    keys, values = [], []
    for tok in line.split(" "):
        tok = tok.strip()
        if not tok:
            continue
        keys.append(tok[:tok.index(":")])
        values.append(tok[tok.rfind(":") + 1:])
    return keys, values


class _LinearRanker(Ranker):
    """What CoorAscent, AdaRank, RankBoost and LinearRegRank share: each trains through a _native trainer of its own (self._trainer, made
    by init()) and scores rows with one of the library's predict functions (_predict)."""

    def _train_metric(self):
        """the scorer's metric as the trainers name it; the linear rankers train on all six"""
        metric = metric_name(self.scorer) if self.scorer is not None else None
        if metric not in N.RL_CA_METRIC:
            raise RankLibError("rlhip: the %s train metric must be one of NDCG, DCG, MAP, ERR, P, RR (got %s)"
                               % (self.name(), self.scorer.name() if self.scorer else None))
        return metric

    def _finish_learn(self):
        """the end of every learn(): the final scores, their log lines, and the trainer closed"""
        t, nm = self._trainer, self.scorer.name()
        ts, vs = t.scores()
        self.scoreOnTrainingData = java_round(ts, 4)
        logger.info("Finished sucessfully.")
        logger.info("%s on training data: %s", nm, java_double_str(self.scoreOnTrainingData))
        if vs is not None:
            self.bestScoreOnValidationData = vs
            logger.info("%s on validation data: %s", nm, java_double_str(java_round(vs, 4)))
        t.close()
        self._trainer = None

    def evalList(self, rl):
        if rl.size() == 0:
            return []
        return [float(v) for v in self._predict(rl.rl)]

    def _evalDocs(self, dps):
        return np.asarray(self._predict(dps), np.float64)

    def eval(self, dp):               # noqa: A003  the Java's eval(DataPoint): the same f64 sum, one row
        return self.evalList(RankList([dp]))[0]


class CoorAscent(_LinearRanker):
    """learning/CoorAscent.java: the linear ranker, learn() executed on an MI355X (librlhip.so rl_ca_*, every trial of a search direction
    in one pass), eval() as the GPU's f64 dot product in feature order."""
    # process-global parameters, like the Java statics (:37-43)
    nRestart = 5
    nMaxIteration = 25
    stepBase = 0.05
    stepScale = 2.0
    tolerance = 0.001
    regularized = False
    slack = 0.001
    seed = 0                          # not in the Java (Collections.shuffle on an unseeded Random): one java.util.Random(seed) per learn()
    device = 0

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self.weight = None
        self.trace = None             # structured array of the last learn() (_native.CA_TRACE_DTYPE)
        self._trainer = None

    def init(self):                   # :60-64
        logger.info("Initializing... ")
        self.weight = [1.0 / len(self.features)] * len(self.features)
        metric = self._train_metric()
        cls = type(self)
        t = N.CoorAscentTrainer(n_restart=cls.nRestart, n_max_iteration=cls.nMaxIteration, step_base=cls.stepBase, step_scale=cls.stepScale,
                                tolerance=cls.tolerance, regularized=cls.regularized, slack=cls.slack, metric=metric,
                                metric_k=self.scorer.getK(), device=cls.device, seed=cls.seed, err_max=ERRScorer.MAX)
        feed_trainer(self, t, metric)
        self._trainer = t

    def learn(self):                  # :67-202
        cls = type(self)
        t = self._trainer
        logger.info("Training starts...")
        t.learn()
        nm = self.scorer.name()
        self.trace = tr = t.trace()
        best = None
        for rec in tr:                # the Java's log, replayed from the trace
            kind = int(rec["kind"])
            if kind == N.CA_RESTART:
                logger.info("[+] Random restart #%d/%d...", int(rec["restart"]) + 1, cls.nRestart)
                best = float(rec["score"])
            elif kind == N.CA_PASS:
                logger.info("Shuffling features' order...")
                logger.info("Optimizing weight vector... ")
                self.printLogLn([7, 8, 7], ["Feature", "weight", nm])
            elif kind == N.CA_TRIAL and rec["improved"]:
                best = float(rec["score"])
                w = float(rec["weight"])
                bw = ("+" if w > 0 else "") + java_double_str(java_round(w, 4))
                self.printLogLn([7, 8, 7], [str(self.features[int(rec["feature"])]), bw, java_double_str(java_round(best, 4))])
        self.weight = [float(v) for v in t.weights()]
        self._finish_learn()

    # --- scoring: 0.0 + w[0] x[f0] + w[1] x[f1] + ... in f64 on the GPU (rl_ca_predict) -----------------
    def _predict(self, dps):          # eval :229-235
        return N.ca_predict(self.features, self.weight, dense_rows(dps, checked=self.features), type(self).device)

    def createNew(self):
        return CoorAscent()

    def toString(self):               # :243-249
        return " ".join("%d:%s" % (f, java_double_str(w)) for f, w in zip(self.features, self.weight))

    def model(self):                  # :252-264
        cls = type(self)
        out = "## " + self.name() + "\n"
        out += "## Restart = %d\n" % cls.nRestart
        out += "## MaxIteration = %d\n" % cls.nMaxIteration
        out += "## StepBase = %s\n" % java_double_str(cls.stepBase)
        out += "## StepScale = %s\n" % java_double_str(cls.stepScale)
        out += "## Tolerance = %s\n" % java_double_str(cls.tolerance)
        out += "## Regularized = %s\n" % ("true" if cls.regularized else "false")
        out += "## Slack = %s\n" % java_double_str(cls.slack)
        return out + self.toString()

    def loadFromString(self, fullText):   # :267-296: the first non-empty line that is not "##", read by utilities/KeyValuePair.java
        try:
            keys, values = _key_value_line(fullText)
            self.features = [int(k) for k in keys]
            self.weight = [float(v) for v in values]
        except Exception as ex:       # noqa: BLE001 -- the reference wraps everything
            raise RankLibError("Error in CoorAscent::load(): %s" % ex)

    def printParameters(self):        # :298-308
        cls = type(self)
        logger.info("No. of random restarts: %d", cls.nRestart)
        logger.info("No. of iterations to search in each direction: %d", cls.nMaxIteration)
        logger.info("Tolerance: %s", java_double_str(cls.tolerance))
        if cls.regularized:
            logger.info("Reg. param: %s", java_double_str(cls.slack))
        else:
            logger.info("Regularization: No")

    def name(self):
        return "Coordinate Ascent"

    @staticmethod
    def getDistance(w1, w2):          # :350-364
        s1 = s2 = 0.0
        for a, b in zip(w1, w2):
            s1 += abs(a)
            s2 += abs(b)
        dist = 0.0
        for a, b in zip(w1, w2):
            t = a / s1 - b / s2
            dist += t * t
        return math.sqrt(dist)

    def copyModel(self, ranker):      # :384-391
        if len(ranker.weight) != len(self.features):
            raise RankLibError("These two models use different feature set!!")
        self.weight = list(ranker.weight)
        logger.info("Model loaded.")

    def distance(self, ca):           # :393-395
        return self.getDistance(self.weight, ca.weight)


class AdaRank(_LinearRanker):
    """learning/boosting/AdaRank.java: a linear ensemble of single-feature weak rankers, learn() executed on an MI355X (librlhip.so
    rl_ada_*: the weak rankers' metric table once, then a candidate pass and one ranking of the ensemble per round), eval() as the GPU's
    f64 sum in ensemble order."""
    # process-global parameters, like the Java statics (:37-40)
    nIteration = 500
    tolerance = 0.002
    trainWithEnqueue = True
    maxSelCount = 5
    device = 0

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self.rankers = []             # the weak rankers' feature IDs (WeakRanker.getFID), in ensemble order; may repeat
        self.rweight = []
        self.trace = None             # structured array of the last learn() (_native.ADA_TRACE_DTYPE)
        self._trainer = None

    def init(self):                   # :205-227
        logger.info("Initializing... ")
        metric = self._train_metric()
        cls = type(self)
        t = N.AdaRankTrainer(n_iteration=cls.nIteration, tolerance=cls.tolerance, train_with_enqueue=cls.trainWithEnqueue,
                             max_sel_count=cls.maxSelCount, metric=metric, metric_k=self.scorer.getK(), device=cls.device,
                             err_max=ERRScorer.MAX)
        feed_trainer(self, t, metric)
        self.rankers, self.rweight = [], []
        self._trainer = t

    def learn(self):                  # :230-262
        t = self._trainer
        logger.info("Training starts...")
        nm = self.scorer.name()
        self.printLogLn([7, 8, 9, 9, 9], ["#iter", "Sel. F.", nm + "-T", nm + "-V", "Status"])
        try:
            t.learn()
        finally:
            self.trace = tr = t.trace()
            for rec in tr:            # the Java's log, replayed from the trace
                kind, fid = int(rec["kind"]), (self.features[int(rec["feature"])] if rec["feature"] >= 0 else -1)
                if kind == N.ADA_ROLLBACK:
                    self.printLog([7], [str(int(rec["iteration"]))])
                    self.printLogLn([8, 9, 9, 9], [str(fid), "", "", "ROLLBACK"])
                elif kind == N.ADA_ROUND:
                    self.printLog([7], [str(int(rec["iteration"]))])
                    self.printLog([8, 9], [str(fid), java_double_str(java_round(float(rec["train_score"]), 4))])
                    vs = java_double_str(java_round(float(rec["valid_score"]), 4)) if t.has_valid else ""
                    self.printLogLn([9, 9], [vs, N.ADA_STATUS[int(rec["status"])]])
        cols, w = t.model()
        self.rankers = [int(self.features[int(c)]) for c in cols]
        self.rweight = [float(v) for v in w]
        self._finish_learn()

    # --- scoring: 0.0 + w[0] x[f0] + w[1] x[f1] + ... in f64 on the GPU (rl_ca_predict, repeated fids) -----------------
    def _predict(self, dps):          # eval :265-271
        return N.ca_predict(self.rankers, self.rweight, dense_rows(dps, checked=self.rankers), type(self).device)

    def createNew(self):
        return AdaRank()

    def toString(self):               # :279-285
        return " ".join("%d:%s" % (f, java_double_str(w)) for f, w in zip(self.rankers, self.rweight))

    def model(self):                  # :288-297
        cls = type(self)
        out = "## " + self.name() + "\n"
        out += "## Iteration = %d\n" % cls.nIteration
        out += "## Train with enqueue: %s\n" % ("Yes" if cls.trainWithEnqueue else "No")
        out += "## Tolerance = %s\n" % java_double_str(cls.tolerance)
        out += "## Max consecutive selection count = %d\n" % cls.maxSelCount
        return out + self.toString()

    def loadFromString(self, fullText):   # :300-332
        try:
            keys, values = _key_value_line(fullText)
            self.features = [int(k) for k in keys]
            self.rankers = list(self.features)
            self.rweight = [float(v) for v in values]
        except Exception as ex:       # noqa: BLE001 -- the reference wraps everything
            raise RankLibError("Error in AdaRank::load(): %s" % ex)

    def printParameters(self):        # :335-340
        cls = type(self)
        logger.info("No. of rounds: %d", cls.nIteration)
        logger.info("Train with 'enequeue': %s", "Yes" if cls.trainWithEnqueue else "No")
        logger.info("Tolerance: %s", java_double_str(cls.tolerance))
        logger.info("Max Sel. Count: %d", cls.maxSelCount)

    def name(self):
        return "AdaRank"


class RankBoost(_LinearRanker):
    """learning/boosting/RankBoost.java: an ensemble of threshold weak rankers (RBWeakRanker: 1 if x[fid] > threshold else 0), init() and
    learn() executed on an MI355X (librlhip.so rl_rb_*: the crucial pairs' weights, the potentials, the candidate chains, the Z_t chain
    and the metrics of every round), eval() as the GPU's f64 sum in ensemble order."""
    # process-global parameters, like the Java statics (:38-39)
    nIteration = 300
    nThreshold = 10
    device = 0

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self.wRankers = []            # (fid, threshold) of the weak rankers, in ensemble order; a fid may repeat
        self.rWeight = []
        self.trace = None             # structured array of the last learn() (_native.RB_TRACE_DTYPE)
        self._trainer = None

    def init(self):                   # :143-263
        logger.info("Initializing... ")
        metric = self._train_metric()
        cls = type(self)
        t = N.RankBoostTrainer(n_iteration=cls.nIteration, n_threshold=cls.nThreshold, metric=metric, metric_k=self.scorer.getK(),
                               device=cls.device, err_max=ERRScorer.MAX)
        feed_trainer(self, t, metric)
        self.wRankers, self.rWeight = [], []
        self._trainer = t

    def learn(self):                  # :265-346
        t = self._trainer
        logger.info("Training starts...")
        nm = self.scorer.name()
        self.printLogLn([7, 8, 9, 9, 9, 9], ["#iter", "Sel. F.", "Threshold", "Error", nm + "-T", nm + "-V"])
        try:
            t.learn()
        finally:
            self.trace = tr = t.trace()
            for rec in tr:            # the Java's log, replayed from the trace
                self.printLog([7, 8, 9, 9], [str(int(rec["iteration"])), str(self.features[int(rec["feature"])]),
                                             java_double_str(java_round(float(rec["threshold"]), 4)),
                                             java_double_str(java_round(float(rec["r_t"]), 4))])
                self.printLog([9], [java_double_str(java_round(float(rec["train_score"]), 4))])
                if t.has_valid:
                    self.printLog([9], [java_double_str(java_round(float(rec["valid_score"]), 4))])
                self.flushLog()
        cols, thr, w = t.model()
        self.wRankers = [(int(self.features[int(c)]), float(v)) for c, v in zip(cols, thr)]
        self.rWeight = [float(v) for v in w]
        self._finish_learn()

    # --- scoring: 0.0 + w[0] h_0(x) + w[1] h_1(x) + ... in f64 on the GPU (rl_rb_predict, repeated fids) ---------------
    def _predict(self, dps):          # eval :348-355
        fids = [f for f, _ in self.wRankers]
        return N.rb_predict(fids, [t for _, t in self.wRankers], self.rWeight, dense_rows(dps, checked=fids), type(self).device)

    def createNew(self):
        return RankBoost()

    def toString(self):               # :362-369
        return " ".join("%d:%s:%s" % (f, java_double_str(t), java_double_str(w)) for (f, t), w in zip(self.wRankers, self.rWeight))

    def model(self):                  # :371-379
        cls = type(self)
        out = "## " + self.name() + "\n"
        out += "## Iteration = %d\n" % cls.nIteration
        out += "## No. of threshold candidates = %d\n" % cls.nThreshold
        return out + self.toString()

    def loadFromString(self, fullText):   # :381-427
        try:
            content = None
            for line in fullText.split("\n"):
                line = line.strip()
                if not line or line.startswith("##"):
                    continue
                content = line
                break
            if content is None:
                raise RankLibError("Model name is not found.")
            idx = content.rfind("#")
            if idx != -1:
                content = content[:idx].strip()       # the comment at the end of the line
            self.wRankers, self.rWeight = [], []
            for tok in content.split(" "):
                tok = tok.strip()
                if not tok:
                    continue
                strs = tok.split(":")
                self.wRankers.append((int(strs[0]), float(strs[1])))
                self.rWeight.append(float(strs[2]))
            self.features = [f for f, _ in self.wRankers]
        except Exception as ex:       # noqa: BLE001 -- the reference wraps everything
            raise RankLibError("Error in RankBoost::load(): %s" % ex)

    def printParameters(self):        # :430-433
        cls = type(self)
        logger.info("No. of rounds: %d", cls.nIteration)
        logger.info("No. of threshold candidates: %d", cls.nThreshold)

    def name(self):
        return "RankBoost"


class LinearRegRank(_LinearRanker):
    """learning/LinearRegRank.java: the least-squares ranker.  learn() runs on an MI355X (librlhip.so rl_lr_*: xTx and xTy accumulated cell
    by cell in the Java's document order, then the Java's elimination without pivoting on the host), eval() as the GPU's f64 sum that
    starts from weight[last].  nVar is the largest feature id of the training lists: features 1 .. nVar - 1 and a constant are fitted,
    feature nVar is not, and eval() pairs weight[i] with features[i] whatever was fitted there."""
    lambda_ = 1E-10                   # LinearRegRank.lambda (:26), -L2
    device = 0

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self.weight = None
        self.gram = None              # (xTx, xTy) of the last learn(), before the ridge term
        self.times = None
        self._trainer = None

    def init(self):                   # :39-41
        logger.info("Initializing...")
        metric = self._train_metric()
        cls = type(self)
        nVar = max((rl.getFeatureCount() for rl in self.samples), default=0)      # :50-56
        if nVar < 1:
            raise RankLibError("Error: some of the input arrays is empty.")       # solve() :189-191
        feats = [int(f) for f in self.features]
        if len(feats) > nVar:
            raise RankLibError("rlhip: Linear Regression has %d features to score with but only nVar = %d weights (the largest feature id "
                               "of the training lists); the Java ends in an ArrayIndexOutOfBoundsException in eval" % (len(feats), nVar))
        # the columns: feature ids 1 .. W.  The fit reads 1 .. nVar - 1 and eval reads the feature list; nothing else is asked of a row
        width = max([nVar] + feats)
        need = sorted(set(range(1, nVar)) | set(feats))

        def flat(lists):
            Xn, lab, qoff, qkey = flatten(lists, need)
            X = np.zeros((Xn.shape[0], width), np.float32)
            for j, f in enumerate(need):
                if 1 <= f <= width:
                    X[:, f - 1] = Xn[:, j]
            return X, lab, qoff, qkey

        t = N.LinearRegTrainer(lambda_=cls.lambda_, metric=metric, metric_k=self.scorer.getK(), device=cls.device, err_max=ERRScorer.MAX)
        feed_trainer(self, t, metric, flat)
        t.set_features(nVar, [f - 1 if 1 <= f <= width else -1 for f in feats])
        self._trainer = t

    def learn(self):                  # :44-100
        t = self._trainer
        logger.info("Training starts...")
        logger.info("Learning the least square model... ")
        try:
            t.learn()
        finally:
            try:
                self.gram, self.times = t.gram(), t.times()
            except RankLibError:
                self.gram = self.times = None
        self.weight = [float(v) for v in t.weights()]
        self._finish_learn()

    # --- scoring: weight[last] + w[0] x[f0] + w[1] x[f1] + ... in f64 on the GPU (rl_lr_predict) -------------------------
    def _predict(self, dps):          # eval :103-109
        if len(self.features) > len(self.weight):
            raise RankLibError("rlhip: Linear Regression has %d features to score with but only %d weights; the Java ends in an "
                               "ArrayIndexOutOfBoundsException in eval" % (len(self.features), len(self.weight)))
        return N.lr_predict(self.features, self.weight, dense_rows(dps, checked=self.features), type(self).device)

    def createNew(self):
        return LinearRegRank()

    def toString(self):               # :117-123: the "0:" entry carries weight[0], and every pair ends in a space: `i == weight.length - 1`
        out = "0:" + java_double_str(self.weight[0]) + " "      # never holds inside a loop that runs to features.length <= weight.length
        for i, f in enumerate(self.features):
            out += "%d:%s" % (f, java_double_str(self.weight[i])) + ("" if i == len(self.weight) - 1 else " ")
        return out

    def model(self):                  # :126-131
        return "## " + self.name() + "\n## Lambda = " + java_double_str(type(self).lambda_) + "\n" + self.toString()

    def loadFromString(self, fullText):   # :134-170: keys > 0 fill features / weight in order, the key 0 value goes to weight[last]
        try:
            keys, values = _key_value_line(fullText)
            weight = [0.0] * len(keys)
            features = [0] * (len(keys) - 1)
            idx = 0
            for k, v in zip(keys, values):
                fid = int(k)
                if fid > 0:
                    features[idx] = fid
                    weight[idx] = float(v)
                    idx += 1
                else:
                    weight[len(weight) - 1] = float(v)
            self.features, self.weight = features, weight
        except Exception as ex:       # noqa: BLE001 -- the reference wraps everything
            raise RankLibError("Error in LinearRegRank::load(): %s" % ex)

    def printParameters(self):        # :173-175
        logger.info("L2-norm regularization: lambda = %s", java_double_str(type(self).lambda_))

    def name(self):
        return "Linear Regression"


def _neural_refusal(type_name):
    """what createRanker, init() and learn() say about RANKNET, LAMBDARANK and LISTNET without their seed: they load and score, they do
    not train"""
    return ("rlhip builds -ranker 6 (LambdaMART), 0 (MART), 8 (Random Forests), 4 (Coordinate Ascent), 3 (AdaRank), 2 (RankBoost) and "
            "9 (Linear Regression); %s, one of the neural-net rankers, is out of scope (SURVEY.md 8)%s"
            % (type_name, "; ListNet trains only with a seed for its initial weights (-netseed n / ListNet.seed)" if type_name == "LISTNET" else
               "; RankNet trains only with a seed for its initial weights (-rnseed n / RankNet.seed)" if type_name == "RANKNET" else
               "; LambdaRank trains only with a seed for its initial weights (-lamseed n / LambdaRank.lamseed)" if type_name == "LAMBDARANK"
               else ""))


class JavaRandom:
    """java.util.Random as its javadoc specifies it: the 48-bit LCG, nextInt(bound) with its rejection loop and nextFloat()"""
    _MASK = (1 << 48) - 1

    def __init__(self, seed):
        self.seed = (int(seed) ^ 0x5DEECE66D) & self._MASK

    def next(self, bits):
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & self._MASK
        v = (self.seed >> (48 - bits)) & 0xFFFFFFFF
        return v - (1 << 32) if v >= (1 << 31) else v

    def nextInt(self, bound=None):
        if bound is None:
            return self.next(32)
        if bound <= 0:
            raise ValueError("bound must be positive")
        r = self.next(31)
        m = bound - 1
        if (bound & m) == 0:
            return (bound * r) >> 31
        u = r
        while u - (u % bound) + m >= (1 << 31):       # the Java's int overflow test
            u = self.next(31)
        return u % bound

    def nextFloat(self):
        return np.float32(self.next(24)) / np.float32(1 << 24)


class Neuron:
    """the one static of learning/neuralnet/Neuron.java that reaches training: ListNet.init() and RankNet.init() copy their learningRate
    into it, and `-lr x` copies it (0.001 unless an earlier init() changed it) into ListNet.learningRate (eval/Evaluator.java:294-296)"""
    learningRate = 0.001              # Neuron.java:22


def _java_int(tok):
    """Integer.parseInt: an optional sign and decimal digits, nothing else, within 32 bits"""
    body = tok[1:] if tok[:1] in ("+", "-") else tok
    if not body or not body.isascii() or not body.isdigit():
        raise ValueError('For input string: "%s"' % tok)
    v = int(tok)
    if not -(1 << 31) <= v < (1 << 31):
        raise ValueError('For input string: "%s"' % tok)
    return v


class RankNet(Ranker):
    """learning/neuralnet/RankNet.java as a scoring-only ranker: loadFromString (:400-448), eval (:336-349) on an MI355X (librlhip.so
    rl_net_*) and model() / toString() (:356-398).  The network is the one wire() (:87-110) makes: layer 0 = the inputs and a bias neuron,
    then the hidden layers, then one output neuron.  self.weights[l - 1] is layer l's matrix [n_l][n_{l-1} + 1]: row j = the weights of
    neuron j's inLinks (the previous layer's neurons in order, the bias last), the order eval() sums in.  A model file lists the weights by
    outLinks instead: input and hidden neurons feed the next layer's neurons in order, the bias neuron (line "0 F") every neuron of layer
    1, then of layer 2, ..., then the output neuron.

    init() and learn() (:257-334) run on an MI355X (librlhip.so rl_rn_*: per epoch every list's forward pass, then one weight update per
    document from its pairs, bit for bit the Java's doubles: DESIGN.md 16) -- but only with RankNet.seed set (-rnseed n, an rlhip
    extension): the Java draws the initial weights from an unseeded static Random (Synapse.java:18,29).  Here every init() draws them from
    a fresh java.util.Random(seed), two draws per synapse in wire()'s creation order.  With seed = None both stay refused.  LambdaRank, a
    subclass, looks at LambdaRank.lamseed only; ListNet, another, at its own seed only."""
    # process-global parameters, like the Java statics (:37-40)
    nIteration = 100
    nHiddenLayer = 1
    nHiddenNodePerLayer = 10
    learningRate = 0.00005
    device = 0
    seed = None                       # rlhip extension (-rnseed): None = training refused
    _TYPE = "RANKNET"
    _LOAD = "RankNet"                 # the class whose loadFromString runs: LambdaRank inherits RankNet's, ListNet has its own copy
    _LAMBDARANK = False               # the trainer's form: rl_rn_set_lambdarank
    _METRICS = ("NDCG", "DCG", "MAP", "ERR", "P", "RR")

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self.hidden = []              # sizes of the hidden layers
        self.weights = []             # per layer past the input: np.float64 [n_l][n_{l-1} + 1]
        self._net = None
        self._trainer = None

    @staticmethod
    def draw_synapse(rnd):
        """Synapse.java:29: (nextInt(2) == 0 ? 1 : -1) * nextFloat() / 10 -- an int times a float, a FLOAT division by 10, widened"""
        sign = np.float32(1 if rnd.nextInt(2) == 0 else -1)
        return float(np.float32(np.float32(sign * rnd.nextFloat()) / np.float32(10)))

    @staticmethod
    def initial_weights(seed, n):
        """the matrices of a network of sizes n = [F, hidden ..., 1], drawn from java.util.Random(seed) in the order wire() (:87-110)
        creates the synapses: input i to every neuron of layer 1 (i outer), then layer to layer (the source neuron outer), then the bias
        to every neuron of layers 1, 2, ..."""
        rnd = JavaRandom(seed)
        w = [np.zeros((n[l], n[l - 1] + 1), np.float64) for l in range(1, len(n))]
        for i in range(n[0]):
            for j in range(n[1]):
                w[0][j, i] = RankNet.draw_synapse(rnd)
        for l in range(1, len(n) - 1):
            for j in range(n[l]):
                for k in range(n[l + 1]):
                    w[l][k, j] = RankNet.draw_synapse(rnd)
        for l in range(1, len(n)):
            for j in range(n[l]):
                w[l - 1][j, n[l - 1]] = RankNet.draw_synapse(rnd)
        return w

    def _trains(self):
        """RankNet itself, and only behind RankNet.seed: LambdaRank inherits the attribute and does not look at it"""
        return self._TYPE == "RANKNET" and RankNet.seed is not None

    def _seed(self):
        return RankNet.seed

    def init(self):                   # :257-287
        if not self._trains():
            raise RankLibError(_neural_refusal(self._TYPE))
        logger.info("Initializing... ")
        metric = metric_name(self.scorer) if self.scorer is not None else None
        if metric not in N.RL_CA_METRIC or metric not in self._METRICS:
            raise RankLibError("rlhip: the %s train metric must be one of %s (got %s)"
                               % (self.name(), ", ".join(self._METRICS), self.scorer.name() if self.scorer else None))
        hidden = [int(RankNet.nHiddenNodePerLayer)] * int(RankNet.nHiddenLayer)
        start = self.initial_weights(self._seed(), [len(self.features)] + hidden + [1])
        Neuron.learningRate = RankNet.learningRate          # :286
        t = N.RankNetTrainer(n_epochs=RankNet.nIteration, learning_rate=Neuron.learningRate, hidden_sizes=hidden, metric=metric,
                             metric_k=self.scorer.getK(), device=RankNet.device, err_max=ERRScorer.MAX, lambdarank=self._LAMBDARANK)
        feed_trainer(self, t, metric)
        t.set_weights(np.concatenate([m.ravel() for m in start]))
        self.hidden, self.weights, self._net = hidden, start, None
        self._trainer = t

    def learn(self):                  # :290-334
        t = self._trainer
        if not self._trains() or t is None:
            raise RankLibError(_neural_refusal(self._TYPE))
        nm, valid = self.scorer.name(), self.validationSamples is not None
        logger.info("Training starts...")
        self.printLogLn([7, 14, 9, 9], ["#epoch", "% mis-ordered", nm + "-T", nm + "-V"])
        self.printLogLn([7, 14, 9, 9], [" ", "  pairs", " ", " "])
        try:
            try:
                t.learn()
            except N.NoBestModelError:
                # bestModelOnValidation still holds its empty lists: l.get(0) throws (:206-223)
                raise RankLibError("Error in NeuralNetwork.restoreBestModelOnValidation(): java.lang.IndexOutOfBoundsException: "
                                   "Index 0 out of bounds for length 0") from None
            for r in t.trace():           # :306: round(misorderedPairs / totalPairs, 4); the cross-entropy `error` is never printed
                total = int(r["total_pairs"])
                ratio = java_double_str(java_round(int(r["misordered"]) / total, 4)) if total else "NaN"
                self.printLog([7, 14], [str(int(r["epoch"])), ratio])
                self.printLog([9], [java_double_str(java_round(float(r["train"]), 4))])
                if valid:
                    self.printLog([9], [java_double_str(java_round(float(r["valid"]), 4))])
                self.flushLog()
            n = self._sizes()
            flat, self.weights, at = np.array(t.weights(), np.float64), [], 0
            for l in range(1, len(n)):
                self.weights.append(flat[at:at + n[l] * (n[l - 1] + 1)].reshape(n[l], n[l - 1] + 1).copy())
                at += n[l] * (n[l - 1] + 1)
            self._net = None
            ts, vs = t.scores()
        finally:
            t.close()
            self._trainer = None
        self.scoreOnTrainingData = java_round(ts, 4)
        logger.info("Finished sucessfully.")
        logger.info("%s on training data: %s", nm, java_double_str(self.scoreOnTrainingData))
        if valid:
            self.bestScoreOnValidationData = vs
            logger.info("%s on validation data: %s", nm, java_double_str(java_round(vs, 4)))

    # --- the network's shape --------------------------------------------------------------------------------
    def _sizes(self):
        """neurons per layer as eval() sees them: the inputs (without the bias), the hidden layers, the output neuron"""
        return [len(self.features)] + list(self.hidden) + [1]

    @staticmethod
    def _out_links(n, layer, neuron):
        """[(target layer, target neuron)] of a neuron's outLinks in wire()'s order, n = _sizes(); layer 0 has the bias at index n[0]"""
        if layer == 0 and neuron == n[0]:
            return [(l, j) for l in range(1, len(n)) for j in range(n[l])]
        return [(layer + 1, j) for j in range(n[layer + 1])]

    @staticmethod
    def _in_index(n, layer, neuron, target_layer):
        """where the synapse from (layer, neuron) sits among its target's inLinks: the bias is every neuron's last source"""
        return n[target_layer - 1] if (layer == 0 and neuron == n[0]) else neuron

    # --- scoring: the forward pass in f64 on the GPU (rl_net_predict) ---------------------------------------
    def _model(self):
        if self._net is None:
            flat = np.concatenate([w.ravel() for w in self.weights])
            self._net = N.NetModel(self.features, self.hidden, flat, type(self).device)
        return self._net

    def evalList(self, rl):
        if rl.size() == 0:
            return []
        net = self._model()
        return [float(v) for v in net.predict_rows(dense_rows(rl.rl, checked=self.features))]

    def _evalDocs(self, dps):
        return self._model().predict_rows(dense_rows(dps, checked=self.features))

    def eval(self, dp):               # noqa: A003  :336-349
        return self.evalList(RankList([dp]))[0]

    def createNew(self):
        return type(self)()

    # --- model text -----------------------------------------------------------------------------------------
    def toString(self):               # :356-372: "layer neuron w0 w1 ..." per neuron of every layer but the last, by outLinks
        n = self._sizes()
        out = []
        for i in range(len(n) - 1):
            for j in range(n[i] + (1 if i == 0 else 0)):
                ws = " ".join(java_double_str(self.weights[tl - 1][tj, self._in_index(n, i, j, tl)]) for tl, tj in self._out_links(n, i, j))
                out.append("%d %d %s\n" % (i, j, ws))
        return "".join(out)

    def model(self):                  # :374-398
        out = "## " + self.name() + "\n"
        out += "## Epochs = %d\n" % type(self).nIteration
        out += "## No. of features = %d\n" % len(self.features)
        out += "## No. of hidden layers = %d\n" % len(self.hidden)
        for i, sz in enumerate(self.hidden):
            out += "## Layer %d: %d neurons\n" % (i + 1, sz)
        out += " ".join(str(f) for f in self.features) + "\n"
        out += "%d\n" % len(self.hidden)
        for sz in self.hidden:
            out += "%d\n" % sz
        return out + self.toString()

    def loadFromString(self, fullText):   # :400-448 (ListNet.java:176-224 is the same text with another message)
        try:
            lines = []
            for content in fullText.splitlines():
                content = content.strip()
                if not content or content.startswith("##"):
                    continue
                lines.append(content)
            features = [_java_int(t) for t in lines[0].split(" ")]
            nhl = _java_int(lines[1])
            if nhl < 0:
                raise ValueError("NegativeArraySizeException: %d" % nhl)
            hidden = [_java_int(lines[2 + k]) for k in range(nhl)]
            for k, sz in enumerate(hidden):
                if sz < 1:
                    raise ValueError("hidden layer %d has %d neurons: a layer without a neuron is not reproduced" % (k + 1, sz))
            n = [len(features)] + hidden + [1]
            weights = [np.zeros((n[l], n[l - 1] + 1), np.float64) for l in range(1, len(n))]
            seen = set()
            for line in lines[2 + nhl:]:
                s = line.split(" ")
                iLayer, iNeuron = _java_int(s[0]), _java_int(s[1])
                count = n[iLayer] + (1 if iLayer == 0 else 0) if 0 <= iLayer < len(n) else -1
                if not 0 <= iNeuron < count:
                    raise IndexError("no neuron %d in layer %d" % (iNeuron, iLayer))
                if iLayer == len(n) - 1:
                    continue          # the output neuron has no outLinks: nothing is read from its line
                for k, (tl, tj) in enumerate(self._out_links(n, iLayer, iNeuron)):      # tokens beyond the outLinks are ignored
                    if k + 2 >= len(s):
                        raise IndexError("Index %d out of bounds for length %d" % (k + 2, len(s)))
                    weights[tl - 1][tj, self._in_index(n, iLayer, iNeuron, tl)] = float(s[k + 2])      # a later line of the same neuron wins
                seen.add((iLayer, iNeuron))
            for i in range(len(n) - 1):
                for j in range(n[i] + (1 if i == 0 else 0)):
                    if (i, j) not in seen:
                        raise ValueError("no weight line for neuron %d of layer %d: the Java would keep its random initial weights, "
                                         "not reproduced" % (j, i))
            self.features, self.hidden, self.weights, self._net = features, hidden, weights, None
        except Exception as ex:       # noqa: BLE001 -- the reference wraps everything
            raise RankLibError("Error in %s::load(): %s" % (self._LOAD, ex))

    def printParameters(self):        # :450-456
        cls = type(self)
        logger.info("No. of epochs: %d", cls.nIteration)
        logger.info("No. of hidden layers: %d", cls.nHiddenLayer)
        logger.info("No. of hidden nodes per layer: %d", cls.nHiddenNodePerLayer)
        logger.info("Learning rate: %s", java_double_str(cls.learningRate))

    def name(self):
        return "RankNet"


class LambdaRank(RankNet):
    """learning/neuralnet/LambdaRank.java: RankNet's network, model text and eval, and RankNet's init() and learn() with four overrides
    on the device (librlhip.so rl_rn_set_lambdarank: every list re-ranked by the current weights, pairs in both directions, each weighted
    by the train metric's swap change, bit for bit the Java's doubles: DESIGN.md 17).  It trains only with LambdaRank.lamseed set
    (-lamseed n, an rlhip extension): the initial weights come from a fresh java.util.Random(lamseed) in wire() order, and the other
    statics (nIteration, nHiddenLayer, nHiddenNodePerLayer, learningRate) are RankNet's, shared as in the Java.  The attribute cannot be
    called `seed`: LambdaRank.seed is RankNet's, inherited, and opens nothing here.  The train metric is one of NDCG, DCG, MAP, ERR (the
    scorers whose swapChange is built)."""
    lamseed = None                    # rlhip extension (-lamseed): None = training refused
    _TYPE = "LAMBDARANK"
    _LAMBDARANK = True
    _METRICS = ("NDCG", "DCG", "MAP", "ERR")      # metric.TRAINABLE

    def _trains(self):
        return LambdaRank.lamseed is not None

    def _seed(self):
        return LambdaRank.lamseed

    def name(self):                   # :136-138
        return "LambdaRank"


class ListNet(RankNet):
    """learning/neuralnet/ListNet.java: RankNet's eval (:143-145) and toString; its own statics, a shorter model() header (:157-174) and
    its own message in loadFromString (:176-224), which reads hidden layers although ListNet.learn never makes any.

    init() and learn() (:84-140) run on an MI355X (librlhip.so rl_ln_*: one pass over the ranked lists per epoch, the weights updated
    after every list, bit for bit the Java's doubles) -- but only with ListNet.seed set (-netseed n, an rlhip extension): the Java draws
    the initial weights from an unseeded static Random (Synapse.java:18,29), so no two of its runs agree.  Here every init() draws them
    from a fresh java.util.Random(seed), two draws per synapse in wire() order.  With seed = None both stay refused."""
    nIteration = 1500                 # :29-31
    learningRate = 0.00001
    nHiddenLayer = 0
    seed = None                       # rlhip extension (-netseed): None = training refused
    _TYPE = "LISTNET"
    _LOAD = "ListNet"

    def __init__(self, samples=None, features=None, scorer=None):
        super().__init__(samples, features, scorer)
        self._trainer = None

    @staticmethod
    def initial_weights(seed, n):
        """n synapses as Synapse.java:29 draws them: (nextInt(2) == 0 ? 1 : -1) * nextFloat() / 10 -- an int times a float, a FLOAT division
        by 10, widened to double"""
        rnd = JavaRandom(seed)
        out = np.zeros(n, np.float64)
        for k in range(n):
            sign = np.float32(1 if rnd.nextInt(2) == 0 else -1)
            out[k] = float(np.float32(np.float32(sign * rnd.nextFloat()) / np.float32(10)))
        return out

    def init(self):                   # :84-98
        cls = type(self)
        if cls.seed is None:
            raise RankLibError(_neural_refusal(self._TYPE))
        logger.info("Initializing... ")
        metric = metric_name(self.scorer) if self.scorer is not None else None
        if metric not in N.RL_CA_METRIC:
            raise RankLibError("rlhip: the %s train metric must be one of NDCG, DCG, MAP, ERR, P, RR (got %s)"
                               % (self.name(), self.scorer.name() if self.scorer else None))
        F = len(self.features)
        start = self.initial_weights(cls.seed, F + 1)      # wire(): inputs 0 .. F - 1 to the output neuron, then the bias
        Neuron.learningRate = cls.learningRate              # :97
        t = N.ListNetTrainer(n_epochs=cls.nIteration, learning_rate=Neuron.learningRate, metric=metric, metric_k=self.scorer.getK(),
                             device=cls.device, err_max=ERRScorer.MAX)
        feed_trainer(self, t, metric)
        t.set_weights(start)
        self.hidden, self.weights, self._net = [], [start.reshape(1, F + 1)], None
        self._trainer = t

    def learn(self):                  # :101-140
        t = self._trainer
        if type(self).seed is None or t is None:
            raise RankLibError(_neural_refusal(self._TYPE))
        nm, valid = self.scorer.name(), self.validationSamples is not None
        logger.info("Training starts...")
        self.printLogLn([7, 14, 9, 9], ["#epoch", "C.E. Loss", nm + "-T", nm + "-V"])
        try:
            try:
                t.learn()
            except N.NoBestModelError:
                # bestModelOnValidation still holds its empty lists: l.get(0) throws (RankNet.java:206-223)
                raise RankLibError("Error in NeuralNetwork.restoreBestModelOnValidation(): java.lang.IndexOutOfBoundsException: "
                                   "Index 0 out of bounds for length 0") from None
            for r in t.trace():           # estimateLoss() is never called: the loss column is the initial 0.0 in every epoch (:111)
                self.printLog([7, 14], [str(int(r["epoch"])), java_double_str(java_round(0.0, 6))])
                self.printLog([9], [java_double_str(java_round(float(r["train"]), 4))])
                if valid:
                    self.printLog([9], [java_double_str(java_round(float(r["valid"]), 4))])
                self.flushLog()
            F = len(self.features)
            self.hidden, self.weights, self._net = [], [np.array(t.weights(), np.float64).reshape(1, F + 1)], None
            ts, vs = t.scores()
        finally:
            t.close()
            self._trainer = None
        self.scoreOnTrainingData = java_round(ts, 4)
        logger.info("Finished sucessfully.")
        logger.info("%s on training data: %s", nm, java_double_str(self.scoreOnTrainingData))
        if valid:
            self.bestScoreOnValidationData = vs
            logger.info("%s on validation data: %s", nm, java_double_str(java_round(vs, 4)))

    def model(self):                  # :157-174: no "hidden layers" lines, and a literal 0 whatever the network is
        out = "## " + self.name() + "\n"
        out += "## Epochs = %d\n" % type(self).nIteration
        out += "## No. of features = %d\n" % len(self.features)
        out += " ".join(str(f) for f in self.features) + "\n"
        out += "0\n"
        return out + self.toString()

    def printParameters(self):        # :226-230
        cls = type(self)
        logger.info("No. of epochs: %d", cls.nIteration)
        logger.info("Learning rate: %s", java_double_str(cls.learningRate))

    def name(self):
        return "ListNet"


# ---------------------------------------------------------------------------------------------------------
class RankerType(enum.Enum):          # learning/RankerType.java
    MART = 0
    RANKBOOST = 1
    RANKNET = 2
    ADARANK = 3
    COOR_ASCENT = 4
    LAMBDARANK = 5
    LAMBDAMART = 6
    LISTNET = 7
    RANDOM_FOREST = 8
    LINEAR_REGRESSION = 9


RFRanker.rType = RankerType.MART


class RankerFactory:                  # learning/RankerFactory.java:36-118
    def __init__(self):
        self.map = {"LAMBDAMART": LambdaMART, "MART": MART, "RANDOM_FOREST": RFRanker, "COOR_ASCENT": CoorAscent, "ADARANK": AdaRank,
                    "RANKBOOST": RankBoost, "LINEAR_REGRESSION": LinearRegRank}
        self.names = {"LAMBDAMART": "LAMBDAMART", "MART": "MART", "RANDOM FORESTS": "RANDOM_FOREST",
                      "COORDINATE ASCENT": "COOR_ASCENT", "ADARANK": "ADARANK", "RANKBOOST": "RANKBOOST",
                      "LINEAR REGRESSION": "LINEAR_REGRESSION",
                      "RANKNET": "RANKNET", "LAMBDARANK": "LAMBDARANK", "LISTNET": "LISTNET"}     # name().toUpperCase() -> type (:44-53)
        self.loadOnly = {"RANKNET": RankNet, "LAMBDARANK": LambdaRank, "LISTNET": ListNet}       # loaded and scored, not trained

    def createRanker(self, rtype, samples=None, features=None, scorer=None):
        if isinstance(rtype, str):
            try:
                rtype = RankerType[rtype]
            except KeyError:
                raise RankLibError("Could find the class \"%s\" you specified. Make sure the jar library is in your classpath." % rtype)
        if rtype.name == "LISTNET" and ListNet.seed is not None:      # trains behind a seed only
            r = ListNet()
        elif rtype.name == "RANKNET" and RankNet.seed is not None:    # likewise
            r = RankNet()
        elif rtype.name == "LAMBDARANK" and LambdaRank.lamseed is not None:      # likewise
            r = LambdaRank()
        elif rtype.name not in self.map:
            raise RankLibError(_neural_refusal(rtype.name))
        else:
            r = self.map[rtype.name]()
        if samples is not None:
            r.setTrainingSet(samples)
            r.setFeatures(features)
            r.setMetricScorer(scorer)
        return r

    def loadRankerFromString(self, fullText):      # :108-118: the first line names the algorithm
        first = fullText.split("\n", 1)[0]
        name = first.replace("## ", "").strip()
        if name.upper() not in self.names:
            raise RankLibError("Model file does not start with '## LambdaMART', '## MART', '## Random Forests', '## Coordinate Ascent', '## AdaRank', "
                               "'## RankBoost', '## Linear Regression', '## RankNet', '## LambdaRank' or '## ListNet' (got %r)" % first)
        tname = self.names[name.upper()]
        r = self.loadOnly[tname]() if tname in self.loadOnly else self.createRanker(RankerType[tname])      # createRanker refuses the three
        r.loadFromString(fullText)
        return r

    def loadRankerFromFile(self, modelFile):       # :104-106
        with open(modelFile, "r", encoding="ascii") as f:
            return self.loadRankerFromString(f.read())


class RankerTrainer:                  # learning/RankerTrainer.java:23-56
    def __init__(self):
        self.rf = RankerFactory()
        self.trainingTime = 0.0

    def train(self, rtype, train, validation_or_features, features_or_scorer, scorer=None):
        if scorer is None:
            validation, features, scorer = None, validation_or_features, features_or_scorer
        else:
            validation, features = validation_or_features, features_or_scorer
        ranker = self.rf.createRanker(rtype, train, features, scorer)
        if validation is not None:
            ranker.setValidationSet(validation)
        start = time.perf_counter_ns()
        ranker.init()
        ranker.learn()
        self.trainingTime = time.perf_counter_ns() - start
        return ranker

    def getTrainingTime(self):
        return self.trainingTime

    def printTrainingTime(self):
        logger.info("Training time: %s seconds", java_round(self.trainingTime / 1e9, 2))
