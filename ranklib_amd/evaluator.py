"""Command line of the `-ranker 6 / 0 / 8 / 4 / 3 / 2 / 9 / 7 / 1 / 5` paths: mirrors the flags of eval/Evaluator.java that reach LambdaMART, MART, Random
Forests, Coordinate Ascent, AdaRank, RankBoost, Linear Regression, ListNet, RankNet and LambdaRank (:230-377) and the train / test / load / score / rank flows (:669-708, :1076-1094, :1168-1194).

    python -m ranklib_amd.evaluator -train f -ranker 6 -metric2t NDCG@10 -tree 1000 -leaf 31 -save model.txt
    python -m ranklib_amd.evaluator -load model.txt -rank f -score out.txt

The remaining flows of the reference's `main` (:492-545):

    python -m ranklib_amd.evaluator -load f1.m -load f2.m -load f3.m -test f [-idv out]      the models of `-kcv 3 -kcvmd dir`: f is cut into
                                                                                             the same 3 folds, model i scores fold i (:953-992)
    python -m ranklib_amd.evaluator -load f1.m -load f2.m -test t1 -test t2 [-idv out]       model i scores file i (:1000-1033)
    python -m ranklib_amd.evaluator -load f1.m -load f2.m -rank f -score out | -indri out    the same folds, scores / Indri run (:1103-1130, :1225-1262)
    python -m ranklib_amd.evaluator -test f [-idv out]                                       no model: the metric of the file's own order (:885-907)
    python -m ranklib_amd.evaluator -test f -score s                                         the file re-ranked by the numbers of s, one a line (:1040-1068)
    python -m ranklib_amd.evaluator -rank f -indri out                                       the file's own order as an Indri run (:1201-1216)

`-rank f` with neither -score nor -indri raises the Java's "This function has been removed." (:516-518).  With `Evaluator.batch` every
fold, and every model-less flow, is one scoring call and one rl_eval_lists call; `Evaluator.batch = False` is the Java's loops, the same
bytes.

-metric2t takes NDCG@k, DCG@k, MAP, ERR@k, P@k and RR@k for every ranker but LambdaRank (-ranker 5: the first four).  Plain P is P@10;
plain RR has k = 0 in the Java and scores 0 everywhere, so it is refused for training ("metric k out of range").  Best@k trains nothing.

-load also takes the model files of the neural-net rankers (## RankNet, ## LambdaRank, ## ListNet: learning/neuralnet/) for -test, -rank
-score / -indri, -idv, -norm and -qrel; they are scored on the GPU.  -train stays refused for -ranker 7 unless -netseed n, for -ranker 1
unless -rnseed n and for -ranker 5 unless -lamseed n (rlhip extensions) seed the initial weights, which the Java draws from an unseeded
Random:

    python -m ranklib_amd.evaluator -train f -ranker 7 -netseed 3 -epoch 200 -metric2t NDCG@10 -validate v -save model.txt
    python -m ranklib_amd.evaluator -train f -ranker 1 -rnseed 3 -epoch 50 -layer 1 -node 10 -lr 0.00005 -validate v -save model.txt
    python -m ranklib_amd.evaluator -train f -ranker 5 -lamseed 3 -epoch 50 -metric2t NDCG@10 -validate v -save model.txt

With -ranker 7, -epoch n sets ListNet.nIteration, and -lr x, like the Java's (:294-296), sets ListNet.learningRate to Neuron.learningRate
-- 0.001 -- whatever x is; without -lr the rate is ListNet's default 0.00001.  Both, and the seed, are restored when main returns.
With -ranker 1 -rnseed n, -epoch, -layer, -node and -lr x set RankNet's nIteration, nHiddenLayer, nHiddenNodePerLayer and learningRate
(= x, no quirk) for the run, and so they do with -ranker 5 -lamseed n (LambdaRank shares RankNet's statics, as in the Java); in every
other run those flags are parsed and leave RankNet's statics alone.
"""
import logging
import math
import sys

import numpy as np

from ._native import RankLibError
from . import normalizer
from .features import FeatureManager
from .learning import (AdaRank, CoorAscent, RankBoost, LinearRegRank, RankNet, LambdaRank, ListNet, Neuron, DataPoint, FeatureHistogram, LambdaMART, RankerFactory, RankerTrainer, RankerType, RankList, RFRanker, RESUME_NOT_BAGS, REFIT_NOT_BAGS, java_double_str, java_round,
                       stable_desc_order)
from .metric import DCGScorer, ERRScorer, MetricScorerFactory, score_lists

logger = logging.getLogger("ranklib_amd")


class Evaluator:
    mustHaveRelDoc = False            # the reference's static of the same name (eval/Evaluator.java:551), set by -hr
    normalize = False                 # eval/Evaluator.java:553-554, set by -norm
    nml = normalizer.SumNormalizor()
    qrelFile = ""                     # :557, set by -qrel: TREC-style judgments, they only affect MAP and NDCG
    batch = True                      # rlhip: the test-time flows score, rank and evaluate a whole file in one GPU pass (Ranker.evalLists +
                                      # metric.score_lists); False: list by list on the host, the same output byte for byte

    def __init__(self, rType, trainMetric, testMetric):
        self.type = rType
        mf = MetricScorerFactory()
        self.trainScorer = mf.createScorer(trainMetric)
        self.testScorer = mf.createScorer(testMetric)
        if Evaluator.qrelFile:                              # :579-582
            self.trainScorer.loadExternalRelevanceJudgment(Evaluator.qrelFile)
            self.testScorer.loadExternalRelevanceJudgment(Evaluator.qrelFile)
        self.rFact = RankerFactory()

    def evaluate(self, trainFile, validationFile=None, testFile=None, featureDefFile=None, modelFile=None):   # :669-708
        train = _read_input(trainFile)
        validation = _read_input(validationFile) if validationFile else None
        test = _read_input(testFile) if testFile else None
        features = FeatureManager.readFeature(featureDefFile) if featureDefFile else FeatureManager.getFeatureFromSampleVector(train)
        if Evaluator.normalize:                              # :687-695
            self.normalizeLists(train, features)
            if validation is not None:
                self.normalizeLists(validation, features)
            if test is not None:
                self.normalizeLists(test, features)
        trainer = RankerTrainer()
        if validation is not None:
            ranker = trainer.train(self.type, train, validation, features, self.trainScorer)
        else:
            ranker = trainer.train(self.type, train, features, self.trainScorer)
        trainer.printTrainingTime()
        if test is not None:
            s = self._score_test(ranker, test)
            logger.info("%s on test data: %s", self.testScorer.name(), java_round(s, 4))
        if modelFile:
            ranker.save(modelFile)
            logger.info("Model saved to: %s", modelFile)
        return ranker

    def _score_test(self, ranker, test):
        """testScorer.score(ranker.rank(test)): the mean of the lists' values, a serial f64 sum in list order and one division"""
        if not Evaluator.batch:
            return self.testScorer.score(ranker.rank(test))
        flat, _ = ranker.evalLists(test)
        per, _ = score_lists(self.testScorer, test, flat)
        s = 0.0
        for v in per:
            s += float(v)
        return s / len(test)

    def _features(self, featureDefFile, samples):
        return FeatureManager.readFeature(featureDefFile) if featureDefFile else FeatureManager.getFeatureFromSampleVector(samples)

    def normalizeLists(self, samples, fids=None):            # Evaluator.normalize(List<RankList>[, fids]) :629-639 (the static flag has the name here)
        Evaluator.nml.normalizeAll(samples, fids)

    def _train(self, train, validation, features):
        trainer = RankerTrainer()
        if validation is not None:
            return trainer.train(self.type, train, validation, features, self.trainScorer)
        return trainer.train(self.type, train, features, self.trainScorer)

    def evaluate_tts(self, sampleFile, validationFile, featureDefFile, percentTrain, modelFile=None):     # -tts  :716-739
        samples = _read_input(sampleFile)
        features = self._features(featureDefFile, samples)
        if Evaluator.normalize:                              # prepareSplit :1329-1331: the whole file, before it is split
            self.normalizeLists(samples, features)
        train, test = FeatureManager.prepareSplit(samples, percentTrain)
        validation = _read_input(validationFile) if validationFile else None
        if validation is not None and Evaluator.normalize:   # :723-727
            self.normalizeLists(validation, features)
        ranker = self._train(train, validation, features)
        s = self._score_test(ranker, test)
        logger.info("%s on test data: %s", self.testScorer.name(), java_round(s, 4))
        if modelFile:
            ranker.save(modelFile)
            logger.info("Model saved to: %s", modelFile)
        return ranker, s

    def evaluate_tvs(self, trainFile, percentTrain, testFile, featureDefFile, modelFile=None):            # -tvs  :749-773
        samples = _read_input(trainFile)
        features = self._features(featureDefFile, samples)
        if Evaluator.normalize:
            self.normalizeLists(samples, features)
        train, validation = FeatureManager.prepareSplit(samples, percentTrain)
        test = _read_input(testFile) if testFile else None
        if test is not None and Evaluator.normalize:         # :756-760
            self.normalizeLists(test, features)
        ranker = self._train(train, validation, features)
        s = None
        if test is not None:
            s = self._score_test(ranker, test)
            logger.info("%s on test data: %s", self.testScorer.name(), java_round(s, 4))
        if modelFile:
            ranker.save(modelFile)
            logger.info("Model saved to: %s", modelFile)
        return ranker, s

    def evaluate_kcv(self, sampleFile, featureDefFile, nFold, tvs=-1.0, modelDir="", modelFile=""):      # -kcv  :798-873
        samples = _read_input(sampleFile)
        features = self._features(featureDefFile, samples)
        trainingData, validationData, testData = FeatureManager.prepareCV(samples, nFold, tvs)
        if Evaluator.normalize:
            # :816-822, kept as written: ALL folds are normalised once per fold, and the folds share their DataPoints (RankList's copy
            # constructor), so a list is normalised nFold x (the number of folds it appears in) times -- not idempotent in float arithmetic.
            # Every list is in exactly nFold of the fold lists (train, validation or test of each fold): nFold * nFold applications, which
            # the batched normaliser runs in one call on the file's own lists; where it cannot, the loop as written
            done = Evaluator.nml.normalizeBatch(samples, features, times=nFold * nFold)
            for _ in range(0 if done else nFold):
                for group in (trainingData, validationData, testData):
                    for fold in group:
                        self.normalizeLists(fold, features)
        scores, scoreOnTrain, scoreOnTest, totalScoreOnTest, totalTestSampleSize = [], 0.0, 0.0, 0.0, 0
        for i in range(nFold):
            ranker = self._train(trainingData[i], validationData[i] if tvs > 0 else None, features)
            s2 = self._score_test(ranker, testData[i])
            scoreOnTrain += ranker.getScoreOnTrainingData()
            scoreOnTest += s2
            totalScoreOnTest += s2 * len(testData[i])
            totalTestSampleSize += len(testData[i])
            scores.append((ranker.getScoreOnTrainingData(), s2))
            if modelDir:
                import os
                os.makedirs(modelDir, exist_ok=True)
                ranker.save(os.path.join(modelDir, "f%d.%s" % (i + 1, modelFile)))
                logger.info("Fold-%d model saved to: %s", i + 1, modelFile)
        logger.info("Summary:")
        logger.info("%s\t|   Train\t| Test", self.testScorer.name())
        for i, (a, b) in enumerate(scores):
            logger.info("Fold %d\t|   %s\t|  %s\t", i + 1, java_round(a, 4), java_round(b, 4))
        logger.info("Avg.\t|   %s\t|  %s\t", java_round(scoreOnTrain / nFold, 4), java_round(scoreOnTest / nFold, 4))
        logger.info("Total\t|   \t\t|  %s\t", java_round(totalScoreOnTest / totalTestSampleSize, 4))
        return scores

    # ---- several models: the k-fold flows ---------------------------------------------------------------------------------
    def _model_folds(self, modelFiles, test):
        """(ranker f, the lists it is applied to) for f = 0 .. len(modelFiles) - 1, in that order and made when asked for.  test names
        one file: it is cut into len(modelFiles) folds by FeatureManager.prepareCV, as -kcv cut the training file (:953-962).  test is a
        list of files: file f as it is (:1000-1008).  Fold f is normalised with model f's features (:969-972)."""
        nFold = len(modelFiles)
        if isinstance(test, (list, tuple)):
            if len(test) < nFold:                            # the Java ends in an IndexOutOfBoundsException
                raise RankLibError("%d models were given and only %d test files: model f is applied to test file f" % (nFold, len(test)))
            folds = None
        else:
            samples = _read_input(test)
            logger.info("Preparing %d-fold test data... ", nFold)
            _, _, folds = FeatureManager.prepareCV(samples, nFold)
        for f in range(nFold):
            fold = folds[f] if folds is not None else _read_input(test[f])
            ranker = self.rFact.loadRankerFromFile(modelFiles[f])
            if Evaluator.normalize:
                self.normalizeLists(fold, ranker.getFeatures())
            yield ranker, fold

    def _report(self, ids, scores, rankScore, prpFile):
        ids.append("all"); scores.append(rankScore)
        logger.info("%s on test data: %s", self.testScorer.name(), java_round(rankScore, 4))
        if prpFile:
            self.savePerRankListPerformanceFile(ids, scores, prpFile)
            logger.info("Per-ranked list performance saved to: %s", prpFile)
        return rankScore

    def _test_models(self, modelFiles, test, prpFile):      # test(List, String, prp) :953-992 and test(List, List, prp) :1000-1033
        ids, scores, rankScore = [], [], 0.0
        for ranker, fold in self._model_folds(modelFiles, test):
            if not fold:
                continue
            if Evaluator.batch:                              # one scoring and one metric pass per fold, in fold order
                flat, _ = ranker.evalLists(fold)
                per, _ = score_lists(self.testScorer, fold, flat)
                for rl, v in zip(fold, per):
                    ids.append(rl.getID()); scores.append(float(v))
                    rankScore += float(v)
            else:
                for rl in fold:
                    l = ranker.rank(rl)
                    sc = self.testScorer.score(l)
                    ids.append(l.getID()); scores.append(sc)
                    rankScore += sc
        rankScore = rankScore / len(ids)                     # :982: over the lists of all folds
        return self._report(ids, scores, rankScore, prpFile)

    def _write_scores(self, out, ranker, test):             # qid \t index \t Double.toString(eval)
        if Evaluator.batch:
            flat, qoff = ranker.evalLists(test)
            for q, rl in enumerate(test):
                for j, v in enumerate(flat[int(qoff[q]):int(qoff[q + 1])]):
                    out.write("%s\t%d\t%s\n" % (rl.getID(), j, java_double_str(float(v))))
            return
        for rl in test:
            for j, v in enumerate(ranker.evalList(rl)):
                out.write("%s\t%d\t%s\n" % (rl.getID(), j, java_double_str(float(v))))

    def _write_indri(self, out, ranker, test):              # qid Q0 docno rank score indri
        if Evaluator.batch:
            flat, qoff = ranker.evalLists(test)
            _, pos = score_lists(DCGScorer(1), test, flat, want_pos=True)      # any metric would do: the positions are what is read
            for q, rl in enumerate(test):
                a, b = int(qoff[q]), int(qoff[q + 1])
                order = np.empty(b - a, np.int64)
                order[pos[a:b]] = np.arange(b - a)
                for i, j in enumerate(order):
                    docno = rl.get(int(j)).getDescription().replace("#", "").strip()
                    out.write("%s Q0 %s %d %s indri\n" % (rl.getID(), docno, i + 1, java_double_str(java_round(float(flat[a + int(j)]), 5))))
            return
        for rl in test:
            sc = ranker.evalList(rl)
            for i, j in enumerate(stable_desc_order(sc)):
                docno = rl.get(int(j)).getDescription().replace("#", "").strip()
                out.write("%s Q0 %s %d %s indri\n" % (rl.getID(), docno, i + 1, java_double_str(java_round(float(sc[int(j)]), 5))))

    def score(self, modelFile, testFile, outputFile):      # :1076-1094: qid \t index \t score
        """modelFile a list: score(List, String, out) :1103-1130, the file cut into len(modelFile) folds and model f applied to fold f;
        testFile a list too: score(List, List, out) :1138-1160 (main never reaches it, in the Java either)"""
        if isinstance(modelFile, (list, tuple)):
            with open(outputFile, "w", encoding="utf-8") as out:
                for ranker, fold in self._model_folds(modelFile, testFile):
                    if fold:
                        self._write_scores(out, ranker, fold)
            return
        ranker = self.rFact.loadRankerFromFile(modelFile)
        test = _read_input(testFile)
        if Evaluator.normalize:                              # :1080-1082
            self.normalizeLists(test, ranker.getFeatures())
        with open(outputFile, "w", encoding="utf-8") as out:
            self._write_scores(out, ranker, test)

    def rank(self, modelFile, testFile, indriFile=None):   # :1168-1194: qid Q0 docno rank score indri
        """modelFile a list: rank(List, String, indri) :1225-1262, the file cut into len(modelFile) folds and model f applied to fold f;
        testFile a list too: rank(List, List, indri) :1270-1304 (main never reaches it, in the Java either).  Two arguments, or None for
        the model: rank(testFile, indri) :1201-1216, the lists in the order they have"""
        if indriFile is None:
            modelFile, testFile, indriFile = None, modelFile, testFile
        if modelFile is None:
            test = _read_input(testFile)
            with open(indriFile, "w", encoding="utf-8") as out:
                for rl in test:
                    for j in range(rl.size()):
                        docno = rl.get(j).getDescription().replace("#", "").strip()
                        out.write("%s Q0 %s %d %s indri\n" % (rl.getID(), docno, j + 1, java_double_str(java_round(1.0 - 0.0001 * j, 5))))
            return
        if isinstance(modelFile, (list, tuple)):
            with open(indriFile, "w", encoding="utf-8") as out:
                for ranker, fold in self._model_folds(modelFile, testFile):
                    if fold:
                        self._write_indri(out, ranker, fold)
            return
        ranker = self.rFact.loadRankerFromFile(modelFile)
        test = _read_input(testFile)
        if Evaluator.normalize:                              # :1173-1175
            self.normalizeLists(test, ranker.getFeatures())
        with open(indriFile, "w", encoding="utf-8") as out:
            self._write_indri(out, ranker, test)

    def readTestFile(self, ranker, testFile):
        """a -test file as `-load model -test file` scores it (:915-921): read under -hr, normalised over the model's features under
        -norm (ranklib_amd.stages prepares its files with this as well)"""
        test = _read_input(testFile)
        if Evaluator.normalize:                              # :919-921
            self.normalizeLists(test, ranker.getFeatures())
        return test

    def test(self, modelFile, testFile=None, prpFile=""):  # evaluate a saved model (:915-944); -idv: performance per ranked list
        """modelFile a list: test(List, String, prp) :953-992, the file cut into len(modelFile) folds and model f applied to fold f;
        testFile a list too: test(List, List, prp) :1000-1033, model f applied to file f.  One argument, or None for the model:
        test(testFile) / test(testFile, prp) :879-907, the lists scored in the order they have.  (Two strings are a model and a file, as
        they have always been here: the Java's test(testFile, prpFile) is test(None, testFile, prpFile).)"""
        if testFile is None:
            modelFile, testFile = None, modelFile
        if modelFile is None:
            return self._test_input_order(testFile, prpFile)
        if isinstance(modelFile, (list, tuple)):
            return self._test_models(modelFile, testFile, prpFile)
        ranker = self.rFact.loadRankerFromFile(modelFile)
        test = self.readTestFile(ranker, testFile)
        ids, scores, rankScore = [], [], 0.0
        if Evaluator.batch:
            flat, _ = ranker.evalLists(test)
            per, _ = score_lists(self.testScorer, test, flat)
            for rl, v in zip(test, per):
                ids.append(rl.getID()); scores.append(float(v))
                rankScore += float(v)
        else:
            for rl in test:
                l = ranker.rank(rl)
                sc = self.testScorer.score(l)
                ids.append(l.getID()); scores.append(sc)
                rankScore += sc
        rankScore /= len(test)
        return self._report(ids, scores, rankScore, prpFile)

    def _test_input_order(self, testFile, prpFile):         # test(testFile, prp) :885-907: testScorer.score(l) on every list as it was read
        test = _read_input(testFile)
        ids, scores, rankScore = [], [], 0.0
        if Evaluator.batch:                                  # scores that fall strictly inside every list rank it as it stands
            flat = np.concatenate([0.0 - np.arange(rl.size(), dtype=np.float64) for rl in test]) if test else np.zeros(0)
            per, _ = score_lists(self.testScorer, test, flat)
            for rl, v in zip(test, per):
                ids.append(rl.getID()); scores.append(float(v))
                rankScore += float(v)
        else:
            for rl in test:
                sc = self.testScorer.score(rl)
                ids.append(rl.getID()); scores.append(sc)
                rankScore += sc
        rankScore /= len(test)
        return self._report(ids, scores, rankScore, prpFile)

    def testWithScoreFile(self, testFile, scoreFile):      # :1040-1068
        """Ranks every list of testFile by the scores of scoreFile -- one Double.parseDouble per non-empty trimmed line (the forms
        analyzer.parse_java_double reads), dealt to the documents in file order, surplus numbers ignored -- and reports the mean of the
        test metric.  Kept from the Java: what `-rank f -score out` writes (`id \\t j \\t score` lines) is NOT such a file; its lines do not
        parse as one number.  Where the Java ends in an unchecked exception (a line that is no number, fewer numbers than documents) a
        RankLibError names the line or the two counts."""
        from .analyzer import _JAVA_TRIM, parse_java_double
        from .features import smart_reader
        test = _read_input(testFile)
        values = []
        with smart_reader(scoreFile) as f:
            for no, content in enumerate(f, 1):
                content = content.rstrip("\r\n").strip(_JAVA_TRIM)
                if not content:
                    continue
                try:
                    values.append(parse_java_double(content))
                except ValueError as ex:
                    raise RankLibError("Error in Evaluator::testWithScoreFile(): %s, line %d: %s" % (scoreFile, no, ex))
        n_docs = sum(rl.size() for rl in test)
        if len(values) < n_docs:
            raise RankLibError("Error in Evaluator::testWithScoreFile(): %s holds %d scores, %s holds %d documents" % (scoreFile, len(values), testFile, n_docs))
        flat = np.array(values[:n_docs], np.float64)
        if Evaluator.batch:
            per, _ = score_lists(self.testScorer, test, flat)
            rankScore = 0.0
            for v in per:
                rankScore += float(v)
            rankScore /= len(test)
        else:
            ranked, k = [], 0
            for rl in test:
                ranked.append(RankList(rl, list(stable_desc_order(flat[k:k + rl.size()]))))
                k += rl.size()
            rankScore = self.testScorer.score(ranked)         # evaluate(null, test) :654-660
        logger.info("%s on test data: %s", self.testScorer.name(), java_round(rankScore, 4))
        return rankScore

    def savePerRankListPerformanceFile(self, ids, scores, prpFile):       # :1343-1352: "<metric>   <qid>   <Double.toString(score)>"
        with open(prpFile, "w", encoding="utf-8") as out:
            for i, sc in zip(ids, scores):
                out.write("%s   %s   %s\n" % (self.testScorer.name(), i, java_double_str(sc)))


def _read_input(inputFile):
    """Evaluator.readInput (eval/Evaluator.java:625-627): honours the static -hr switch"""
    return FeatureManager.readInput(inputFile, Evaluator.mustHaveRelDoc)


# the command line's numbering (eval/Evaluator.java:69-73 rType2), not the enum's ordinals: 1 is RankNet and 2 is RankBoost there
_RANKER_TYPES = {0: RankerType.MART, 2: RankerType.RANKBOOST, 3: RankerType.ADARANK, 4: RankerType.COOR_ASCENT, 6: RankerType.LAMBDAMART,
                 8: RankerType.RANDOM_FOREST, 9: RankerType.LINEAR_REGRESSION}


_RANK_REMOVED = ("This function has been removed.\nConsider using -score in addition to your current parameters, "
                 "and do the ranking yourself based on these scores.")       # :516-518


class ArgCursor:
    """A command line read from left to right, by every command line of the package: iterating gives each flag in lower case (flags are
    matched case-insensitively, :230-372), nxt() the value that follows the flag in hand, and unknown() is the Java's refusal of it"""

    def __init__(self, args):
        self.args, self.i = args, 0

    def __iter__(self):
        while self.i < len(self.args):
            yield self.args[self.i].lower()
            self.i += 1

    def nxt(self):
        self.i += 1
        if self.i >= len(self.args):
            raise RankLibError("Missing value for " + self.args[self.i - 1])
        return self.args[self.i]

    def unknown(self):                # :369-371
        raise RankLibError("Unknown command-line parameter: " + self.args[self.i])


def common_flag(a, nxt, reader_only=False):
    """The flags that the tools around a loaded model (stages, importance, partial, contribs) share with this command line, with its
    meaning: True when a was one of them.  reader_only: the tool applies no metric and takes tree models alone (contribs), so it knows
    the file reader's -missingZero and -norm, a -device that is LambdaMART's alone, and none of -gmax, -qrel, -hr."""
    if a == "-missingzero": DataPoint.missingZero = True
    elif a == "-norm":
        Evaluator.nml = normalizer.create(nxt())
        Evaluator.normalize = True
    elif a == "-device":
        LambdaMART.device = int(nxt())
        if not reader_only:
            CoorAscent.device = AdaRank.device = RankBoost.device = LinearRegRank.device = RankNet.device = LambdaMART.device
    elif reader_only: return False
    elif a == "-gmax": ERRScorer.MAX = math.pow(2.0, float(nxt()))
    elif a == "-qrel": Evaluator.qrelFile = nxt()
    elif a == "-hr": Evaluator.mustHaveRelDoc = True
    else: return False
    return True


def main(argv=None):
    try:
        return _main(argv)
    finally:      # -resume / -checkpoint / -refit belong to this command line only: a later LambdaMART of the process starts from nothing again
        LambdaMART.resumeFrom, LambdaMART.checkpointFile, LambdaMART.checkpointEvery = None, None, 100
        LambdaMART.refitFrom, LambdaMART.refitDecay = None, 0.0


def _main(argv=None):
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args:
        print("Usage: -train <file> -ranker 4|3|2|9|6|0|8 [-r n -i n -tolerance t -reg slack] [-round n -noeq -max n] [-round n -tc n (RankBoost)] [-L2 reg (Linear Regression)] [-bag n -srate f -frate f -rtype 0|6 -seed n] [-fastleaf] [-resume model] [-checkpoint file [-every n]] [-refit model [-decay x]] [-metric2t NDCG@k|DCG@k|MAP|ERR@k|P@k|RR@k] [-tree n] [-leaf n] [-shrinkage f] [-tc n] [-mls n] [-estop n] "
              "[-validate f] [-test f] [-feature f] [-norm sum|zscore|linear] [-qrel f] [-gmax g] [-save model] | -load model [-test f [-idv out]] [-rank f -indri out] [-rank f -score out] "
              "(-load also reads RankNet, LambdaRank and ListNet models; several -load: the models of a -kcv run, model i for fold i of the file, "
              "or for the i-th -test file) | -test f [-idv out] | -test f -score s | -rank f -indri out (no model: the file's own order, or the order of the numbers in s) | "
              "-train <file> -ranker 7 -netseed n [-epoch n] [-lr x] (ListNet; -netseed, an rlhip extension, seeds the initial weights and is required; "
              "-lr x sets the learning rate to 0.001 whatever x is, as the Java does; without it 0.00001) | "
              "-train <file> -ranker 1 -rnseed n [-epoch n] [-layer n] [-node n] [-lr x] (RankNet; -rnseed, an rlhip extension, seeds the initial weights "
              "and is required; defaults 100 epochs, 1 hidden layer of 10 nodes, learning rate 0.00005) | "
              "-train <file> -ranker 5 -lamseed n [-epoch n] [-layer n] [-node n] [-lr x] [-metric2t NDCG@k|DCG@k|MAP|ERR@k] (LambdaRank; -lamseed, an rlhip "
              "extension, seeds the initial weights and is required; the other flags and defaults are RankNet's) | "
              "-resume model, -checkpoint file [-every n] are rlhip extensions of a -train -ranker 6|0 run: -resume continues the run that wrote the model "
              "(its trees are this run's first rounds, -tree stays the total; from a -checkpoint file the result is the uninterrupted run's bit for bit, "
              "from a final -save model early stopping restarts at its best validation prefix); -checkpoint writes all trees so far to the file after "
              "every n-th round (default 100), complete or not at all | "
              "-refit model [-decay x] is an rlhip extension of a -train -ranker 6|0 run: the model's trees keep their features and thresholds and get "
              "new leaf values from the training file, stored as x * old + (1 - x) * new (x in [0, 1), default 0: the new values alone); -tree stays "
              "the total: equal to the model's tree count the run only refits, larger it trains further behind the refit trees")
        return 0
    trainFile = validationFile = testFile = featureDescriptionFile = savedModelFile = rankFile = indriRankingFile = scoreFile = modelFile = prpFile = ""
    testFiles, savedModelFiles = [], []
    Evaluator.mustHaveRelDoc = False
    Evaluator.normalize = False                             # :86
    Evaluator.qrelFile = ""
    Evaluator.batch = True
    LambdaMART.fastLeaf = False                             # -fastleaf (rlhip extension)
    LambdaMART.resumeFrom, LambdaMART.checkpointFile, LambdaMART.checkpointEvery = None, None, 100      # -resume, -checkpoint, -every (rlhip extensions)
    LambdaMART.refitFrom, LambdaMART.refitDecay = None, 0.0                                             # -refit, -decay (rlhip extensions)
    resumeFile, everyGiven = "", False
    refitFile, decayGiven = "", None
    rankerType = 4                                          # the reference's default is Coordinate Ascent (:83)
    trainMetric, testMetric = "ERR@10", ""                  # the reference's default train metric (:84)
    ttSplit = tvSplit = 0.0
    foldCV, kcvModelDir, kcvModelFile = -1, "", ""
    epochs = netSeed = rnSeed = lamSeed = layers = nodes = lrValue = None
    lrGiven = False
    cur = ArgCursor(args)
    nxt = cur.nxt
    for a in cur:                                           # :230-372 (flags are matched case-insensitively)
        if a == "-train": trainFile = nxt()
        elif a == "-ranker": rankerType = int(nxt())
        elif a == "-feature": featureDescriptionFile = nxt()
        elif a == "-metric2t": trainMetric = nxt()          # also captures -metric2T, exactly like the reference (:237-240)
        elif a == "-gmax": ERRScorer.MAX = math.pow(2.0, float(nxt()))      # eval/Evaluator.java:241-242
        elif a == "-validate": validationFile = nxt()
        elif a == "-test":                                  # :253-255: every -test is kept, testFile is the last one
            testFile = nxt()
            testFiles.append(testFile)
        elif a == "-save": modelFile = nxt()
        elif a == "-load":                                  # :278-280: every -load is kept (the models of a -kcv run), savedModelFile is the last one
            savedModelFile = nxt()
            savedModelFiles.append(savedModelFile)
        elif a == "-rank": rankFile = nxt()
        elif a == "-score": scoreFile = nxt()
        elif a == "-indri": indriRankingFile = nxt()
        elif a == "-missingzero": DataPoint.missingZero = True
        elif a == "-cache": FeatureManager.cache = True      # not a RankLib flag: binary cache of the parsed LETOR files (features.py)
        elif a == "-sparse": pass                           # row storage only (:268-269)
        elif a == "-hr": Evaluator.mustHaveRelDoc = True    # :367-368: ranked lists without a relevant document are dropped by the reader
        elif a == "-idv": prpFile = nxt()                   # :281-282
        elif a == "-tree": LambdaMART.nTrees = RFRanker.nTrees = int(nxt())                 # :326-337: both sets of statics
        elif a == "-leaf": LambdaMART.nTreeLeaves = RFRanker.nTreeLeaves = int(nxt())
        elif a == "-shrinkage": LambdaMART.learningRate = RFRanker.learningRate = float(nxt())
        elif a == "-tc": RankBoost.nThreshold = LambdaMART.nThreshold = int(nxt())           # :300-303: NOT RFRanker.nThreshold
        elif a == "-mls": LambdaMART.minLeafSupport = RFRanker.minLeafSupport = int(nxt())
        elif a == "-estop": LambdaMART.nRoundToStopEarly = int(nxt())
        elif a == "-bag": RFRanker.nBag = int(nxt())                                         # :340-352
        elif a == "-srate": RFRanker.subSamplingRate = float(nxt())
        elif a == "-frate": RFRanker.featureSamplingRate = float(nxt())
        elif a == "-rtype":
            rt = int(nxt())
            if rt not in (0, 6):
                raise RankLibError("%s cannot be bagged. Random Forests only supports MART/LambdaMART." % rt)
            RFRanker.rType = RankerType(rt)
        elif a == "-seed": RFRanker.seed = FeatureHistogram.seed = CoorAscent.seed = int(nxt())     # rlhip extension: the Java draws are unseeded
        elif a == "-fastleaf": LambdaMART.fastLeaf = True   # rlhip extension: RL_FLAG_FAST_LEAF for -ranker 6 / 0 / 8 (leaf values within tolerance, not bit for bit)
        elif a == "-resume": resumeFile = nxt()             # rlhip extension: the saved model whose trees are this run's first rounds
        elif a == "-refit": refitFile = nxt()               # rlhip extension: the saved model whose trees get new leaf values from this run's data
        elif a == "-decay": decayGiven = float(nxt())       # rlhip extension: the share of the old leaf value a refit keeps
        elif a == "-checkpoint": LambdaMART.checkpointFile = nxt()      # rlhip extension: all trees so far, after every -every n-th round
        elif a == "-every":
            LambdaMART.checkpointEvery = int(nxt())
            everyGiven = True
        elif a == "-thread": nxt()                          # CPU thread pool of the reference: irrelevant here
        elif a == "-tts": ttSplit = float(nxt())            # :245-250
        elif a == "-tvs": tvSplit = float(nxt())
        elif a == "-kcv": foldCV = int(nxt())
        elif a == "-kcvmd": kcvModelDir = nxt()
        elif a == "-kcvmn": kcvModelFile = nxt()
        elif a == "-qrel": Evaluator.qrelFile = nxt()       # :243-244
        elif a in ("-nf", "-t"): nxt()                      # :359-364: newFeatureFile / topNew, statics that nothing in the reference reads
        elif a == "-keep": pass                             # keepOrigFeatures, likewise
        elif a == "-norm":                                   # :256-267
            Evaluator.nml = normalizer.create(nxt())
            Evaluator.normalize = True
        elif a == "-r": CoorAscent.nRestart = int(nxt())                                     # :310-323
        elif a == "-i": CoorAscent.nMaxIteration = int(nxt())
        elif a == "-reg":
            CoorAscent.slack = float(nxt())
            CoorAscent.regularized = True
        elif a == "-tolerance": AdaRank.tolerance = CoorAscent.tolerance = float(nxt())
        elif a == "-round": RankBoost.nIteration = AdaRank.nIteration = int(nxt())          # :305-318
        elif a == "-noeq": AdaRank.trainWithEnqueue = False
        elif a == "-max": AdaRank.maxSelCount = int(nxt())
        elif a == "-l2": LinearRegRank.lambda_ = float(nxt())                               # :355-356, whatever -ranker says
        elif a == "-epoch": epochs = int(nxt())              # :284-288; reaches ListNet.nIteration in a -ranker 7 run only (below)
        elif a == "-lr":                                    # :294-296; likewise (and RankNet.learningRate in a -ranker 1 run)
            lrValue = float(nxt())
            lrGiven = True
        elif a == "-netseed": netSeed = int(nxt())          # rlhip extension: seeds ListNet's initial weights (the Java's Random is unseeded)
        elif a == "-rnseed": rnSeed = int(nxt())            # rlhip extension: seeds RankNet's initial weights, likewise
        elif a == "-lamseed": lamSeed = int(nxt())          # rlhip extension: seeds LambdaRank's initial weights, likewise
        elif a == "-layer": layers = int(nxt())             # :290-293; reach RankNet's statics in a -ranker 1 -rnseed run only (below); every
        elif a == "-node": nodes = int(nxt())               # other run parses and ignores them (test:eval/EvaluatorTest.java:207-220 passes them to every ranker)
        elif a == "-device": LambdaMART.device = CoorAscent.device = AdaRank.device = RankBoost.device = LinearRegRank.device = RankNet.device = int(nxt())
        else:
            cur.unknown()                                   # :369-371 (incl. the documented -silent)
    if not testMetric:
        testMetric = trainMetric                            # :379-381
    if refitFile or decayGiven is not None:
        if not refitFile:
            raise RankLibError("rlhip: -decay x belongs to -refit model")
        if decayGiven is not None and not (0.0 <= decayGiven < 1.0):       # (NaN fails both comparisons)
            raise RankLibError("rlhip: -decay must be in [0, 1) (got %s): the share of the old leaf value a refit keeps" % decayGiven)
        if not trainFile:
            raise RankLibError("rlhip: -refit recomputes a model's leaf values on training data: it needs -train")
        if rankerType == 8:
            raise RankLibError(REFIT_NOT_BAGS)
        if rankerType not in (0, 6):
            raise RankLibError("rlhip: -refit is built for the tree trainers, -ranker 6 (LambdaMART) and -ranker 0 (MART), not for -ranker %d" % rankerType)
        if foldCV != -1:
            raise RankLibError("rlhip: -refit with -kcv: every fold is a run of its own, one model cannot be refitted into them all")
        if resumeFile:
            raise RankLibError("rlhip: -refit together with -resume: a model is either adopted as it is or refitted")
        try:
            with open(refitFile, encoding="ascii") as f:
                LambdaMART.refitFrom = f.read()
        except (OSError, UnicodeDecodeError) as ex:
            raise RankLibError("rlhip: -refit %s cannot be read as a model text: %s" % (refitFile, ex))
        LambdaMART.refitDecay = 0.0 if decayGiven is None else decayGiven
    if resumeFile or LambdaMART.checkpointFile or everyGiven:
        what = "-resume" if resumeFile else "-checkpoint" if LambdaMART.checkpointFile else "-every"
        if everyGiven and not LambdaMART.checkpointFile:
            raise RankLibError("rlhip: -every n belongs to -checkpoint file")
        if LambdaMART.checkpointEvery < 1:
            raise RankLibError("rlhip: -every must be >= 1 (got %d)" % LambdaMART.checkpointEvery)
        if not trainFile:
            raise RankLibError("rlhip: %s continues or saves a training run: it needs -train" % what)
        if rankerType == 8:
            raise RankLibError(RESUME_NOT_BAGS)
        if rankerType not in (0, 6):
            raise RankLibError("rlhip: %s is built for the tree trainers, -ranker 6 (LambdaMART) and -ranker 0 (MART), not for -ranker %d" % (what, rankerType))
        if foldCV != -1:
            raise RankLibError("rlhip: %s with -kcv: every fold is a run of its own, one file cannot continue or hold them all" % what)
        if resumeFile:
            try:
                with open(resumeFile, encoding="ascii") as f:
                    LambdaMART.resumeFrom = f.read()
            except (OSError, UnicodeDecodeError) as ex:
                raise RankLibError("rlhip: -resume %s cannot be read as a model text: %s" % (resumeFile, ex))
    listnet = rankerType == 7 and netSeed is not None        # ListNet trains behind a seed only
    ranknet = rankerType == 1 and rnSeed is not None         # RankNet likewise, behind its own
    lambdarank = rankerType == 5 and lamSeed is not None     # LambdaRank likewise
    if trainFile and rankerType not in _RANKER_TYPES and not listnet and not ranknet and not lambdarank:
        raise RankLibError("rlhip builds -ranker 6 (LambdaMART), -ranker 0 (MART), -ranker 8 (Random Forests), -ranker 4 (Coordinate Ascent), "
                           "-ranker 3 (AdaRank), -ranker 2 (RankBoost) and -ranker 9 (Linear Regression) only: the neural-net rankers "
                           "(-ranker 1 RankNet, 5 LambdaRank, 7 ListNet) are out of scope"
                           + ("; ListNet trains only with -netseed n, a seed for its initial weights" if rankerType == 7 else
                              "; RankNet trains only with -rnseed n, a seed for its initial weights" if rankerType == 1 else
                              "; LambdaRank trains only with -lamseed n, a seed for its initial weights" if rankerType == 5 else ""))

    def flows(rtype):                                       # :469-520
        nonlocal kcvModelDir, kcvModelFile
        e = Evaluator(rtype, trainMetric, testMetric)
        if trainFile:
            if foldCV != -1:                                # :469-482
                if kcvModelDir and not kcvModelFile:
                    kcvModelFile = "kcv"
                elif not kcvModelDir and kcvModelFile:
                    kcvModelDir = "kcvmodels"
                e.evaluate_kcv(trainFile, featureDescriptionFile or None, foldCV, tvSplit if tvSplit > 0 else -1.0, kcvModelDir, kcvModelFile)
            elif ttSplit > 0.0:                             # -tts overrides -tvs (:484-486)
                e.evaluate_tts(trainFile, validationFile or None, featureDescriptionFile or None, ttSplit, modelFile or None)
            elif tvSplit > 0.0:
                e.evaluate_tvs(trainFile, tvSplit, testFile or None, featureDescriptionFile or None, modelFile or None)
            else:
                e.evaluate(trainFile, validationFile or None, testFile or None, featureDescriptionFile or None, modelFile or None)
        elif savedModelFile and len(savedModelFiles) == 1:
            if rankFile and indriRankingFile:
                e.rank(savedModelFile, rankFile, indriRankingFile)
            elif rankFile and scoreFile:
                e.score(savedModelFile, rankFile, scoreFile)
            elif testFile:
                e.test(savedModelFile, testFile, prpFile)
            elif rankFile:
                raise RankLibError(_RANK_REMOVED)
        elif savedModelFile:                                # :492-545 with several models: those of a -kcv run, model f for fold f
            if rankFile:
                if scoreFile:
                    e.score(savedModelFiles, rankFile, scoreFile)
                elif indriRankingFile:
                    e.rank(savedModelFiles, rankFile, indriRankingFile)
                else:
                    raise RankLibError(_RANK_REMOVED)
            elif testFile:
                e.test(savedModelFiles, testFiles if len(testFiles) > 1 else testFile, prpFile)
        elif rankFile:                                      # no model: the input's own order
            if scoreFile:                                   # (the Java goes on to load the model "")
                raise RankLibError("-rank %s -score %s writes a model's scores: it needs -load" % (rankFile, scoreFile))
            if not indriRankingFile:
                raise RankLibError(_RANK_REMOVED)
            e.rank(rankFile, indriRankingFile)
        elif testFile:
            if scoreFile:
                e.testWithScoreFile(testFile, scoreFile)
            else:
                e.test(None, testFile, prpFile)
        return 0

    if ranknet or lambdarank:
        # RankNet's statics (LambdaRank shares them) belong to this run only, as ListNet's below
        saved = (RankNet.nIteration, RankNet.nHiddenLayer, RankNet.nHiddenNodePerLayer, RankNet.learningRate, RankNet.seed, Neuron.learningRate,
                 LambdaRank.lamseed)
        try:
            if ranknet:
                RankNet.seed = rnSeed
            else:
                LambdaRank.lamseed = lamSeed
            if epochs is not None:
                RankNet.nIteration = epochs                     # :284-288
            if layers is not None:
                RankNet.nHiddenLayer = layers                   # :290-291
            if nodes is not None:
                RankNet.nHiddenNodePerLayer = nodes             # :292-293
            if lrGiven:
                RankNet.learningRate = lrValue                  # :295
            return flows(RankerType.RANKNET if ranknet else RankerType.LAMBDARANK)
        finally:
            (RankNet.nIteration, RankNet.nHiddenLayer, RankNet.nHiddenNodePerLayer, RankNet.learningRate, RankNet.seed, Neuron.learningRate,
             LambdaRank.lamseed) = saved
    if not listnet:
        return flows(_RANKER_TYPES.get(rankerType, RankerType.LAMBDAMART))
    # ListNet's statics belong to this run only: the refusals and defaults other callers see are the same before and after it
    saved = (ListNet.nIteration, ListNet.learningRate, ListNet.seed, Neuron.learningRate)
    try:
        ListNet.seed = netSeed
        if epochs is not None:
            ListNet.nIteration = epochs                     # :284-288 (RankNet's statics, which the Java sets too, are not touched here)
        if lrGiven:
            ListNet.learningRate = Neuron.learningRate      # :296, as written: -lr x never reaches ListNet
        return flows(RankerType.LISTNET)
    finally:
        ListNet.nIteration, ListNet.learningRate, ListNet.seed, Neuron.learningRate = saved


if __name__ == "__main__":
    sys.exit(main())
