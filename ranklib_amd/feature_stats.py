"""ciir.umass.edu.features.FeatureStats (features/FeatureStats.java:25-194): how often a saved model uses each feature, with the summary
statistics of those frequencies.  Reached from `python -m ranklib_amd.features -feature_stats model.txt`.

The statistics restate commons-math's DescriptiveStatistics as FeatureStats uses it: getMin, getMax, getPercentile(50) (the legacy
estimate), getMean (the two-pass corrected mean), getVariance (bias-corrected) and getStandardDeviation.  `%10.2f` rounds HALF_UP, as
java.util.Formatter does; it is applied here to the double's exact value (not checked against a JVM: DESIGN.md 22).
"""
import decimal
import logging
import math
import os

from ._native import RankLibError

logger = logging.getLogger("ranklib_amd")

ALL_FEATURES = ("Coordinate Ascent", "LambdaRank", "Linear Regression", "ListNet", "RankNet")       # :144-145
FEATURE_WEIGHT = ("AdaRank", "RankBoost")                                                            # :151
TREES = ("LambdaMART", "MART", "Random Forests")                                                     # :156


def java_format_2f(v, width=10):
    """String.format("%10.2f", v): two decimals rounded HALF_UP, right-aligned"""
    if v != v:
        s = "NaN"
    elif v in (math.inf, -math.inf):
        s = "Infinity" if v > 0 else "-Infinity"
    else:
        s = str(decimal.Decimal(v).quantize(decimal.Decimal("0.01"), rounding=decimal.ROUND_HALF_UP))
    return s.rjust(width)


def _java_split(s, sep):               # String.split(sep) for a one-character separator: trailing empty strings are dropped
    parts = s.split(sep)
    while parts and parts[-1] == "":
        parts.pop()
    return parts if parts or s != "" else [""]


class DescriptiveStatistics:
    """org.apache.commons.math3.stat.descriptive.DescriptiveStatistics, the six values FeatureStats prints"""

    def __init__(self):
        self.values = []

    def addValue(self, v):
        self.values.append(float(v))

    def getMin(self):
        return min(self.values) if self.values else math.nan

    def getMax(self):
        return max(self.values) if self.values else math.nan

    def getPercentile(self, p):       # Percentile's legacy estimate: pos = p (n + 1) / 100 on the sorted values
        x, n = sorted(self.values), len(self.values)
        if n == 0:
            return math.nan
        if n == 1:
            return x[0]
        pos = p * (n + 1) / 100.0
        fpos = math.floor(pos)
        if pos < 1:
            return x[0]
        if pos >= n:
            return x[n - 1]
        lower, upper = x[int(fpos) - 1], x[int(fpos)]
        return lower + (pos - fpos) * (upper - lower)

    def getMean(self):                # Mean.evaluate: xbar = sum / n, then the correction sum(x - xbar) / n
        n = len(self.values)
        if n == 0:
            return math.nan
        s = 0.0
        for v in self.values:
            s += v
        xbar = s / n
        corr = 0.0
        for v in self.values:
            corr += v - xbar
        return xbar + corr / n

    def getVariance(self):            # Variance.evaluate, bias-corrected: (sum(dev^2) - sum(dev)^2 / n) / (n - 1); 0 for one value
        n = len(self.values)
        if n == 0:
            return math.nan
        if n == 1:
            return 0.0
        m = self.getMean()
        accum = accum2 = 0.0
        for v in self.values:
            dev = v - m
            accum += dev * dev
            accum2 += dev
        return (accum - (accum2 * accum2 / n)) / (n - 1.0)

    def getStandardDeviation(self):
        n = len(self.values)
        if n == 0:
            return math.nan
        return math.sqrt(self.getVariance()) if n > 1 else 0.0


class FeatureStats:
    def __init__(self, modelFileName):
        self.modelFileName = os.path.abspath(modelFileName)          # File.getAbsolutePath :38-39
        self.modelName = None

    @staticmethod
    def _count(tm, text):
        try:
            fid = int(text)                                          # Integer.valueOf
        except ValueError:
            raise RankLibError("Exception: java.lang.NumberFormatException: For input string: \"%s\"" % text)
        tm[fid] = tm.get(fid, 0) + 1

    def getFeatureWeightFeatureFrequencies(self, lines):            # :42-81: every token's text before its first ':'
        tm = {}
        for line in lines:
            line = line.strip().lower()
            if not line or "##" in line:
                continue
            for tok in _java_split(line, " "):
                self._count(tm, _java_split(tok, ":")[0] if tok else "")
        return tm

    def getTreeFeatureFrequencies(self, lines):                     # :83-119: the text between the first '>' and the next '<'
        tm = {}
        for line in lines:
            line = line.strip().lower()
            if not line or "##" in line:
                continue
            if "<feature>" in line:
                q1 = line.index(">")
                q2 = line.find("<", q1 + 1)
                if q2 < 0:
                    raise RankLibError("Exception: java.lang.StringIndexOutOfBoundsException: no '<' after the feature id in \"%s\"" % line)
                self._count(tm, line[q1 + 1:q2].strip())
        return tm

    def writeFeatureStats(self):                                    # :121-192
        try:
            with open(self.modelFileName, "r", encoding="utf-8") as f:
                lines = f.read().splitlines()
        except OSError as ex:
            raise RankLibError("IOException on file %s: %s" % (self.modelFileName, ex))
        nameparts = _java_split(lines[0].strip(), " ") if lines else []
        if len(nameparts) == 2:
            self.modelName = nameparts[1].strip()
        elif len(nameparts) == 3:
            self.modelName = nameparts[1].strip() + " " + nameparts[2].strip()
        if self.modelName is None:
            raise RankLibError("No model name defined.  Quitting.")
        if self.modelName in ALL_FEATURES:
            logger.info("%s uses all features.  Can't do selected model statistics for this algorithm.", self.modelName)
            return
        if self.modelName in FEATURE_WEIGHT:
            tm = self.getFeatureWeightFeatureFrequencies(lines[1:])
        elif self.modelName in TREES:
            tm = self.getTreeFeatureFrequencies(lines[1:])
        else:                          # (the Java goes on with a null map and ends in a NullPointerException)
            raise RankLibError("Failure processing saved %s model file: '%s' is not a model FeatureStats knows" % (self.modelFileName, self.modelName))
        logger.info("Model File: %s", self.modelFileName)
        logger.info("Algorithm : %s", self.modelName)
        logger.info("Feature frequencies : ")
        ds = DescriptiveStatistics()
        for fid in sorted(tm):                                       # a TreeMap: ascending ids
            logger.info("\tFeature[%d] : %7d", fid, tm[fid])
            ds.addValue(tm[fid])
        logger.info("Total Features Used: %d", len(tm))
        logger.info("Min frequency    : %s", java_format_2f(ds.getMin()))
        logger.info("Max frequency    : %s", java_format_2f(ds.getMax()))
        logger.info("Median frequency : %s", java_format_2f(ds.getPercentile(50)))
        logger.info("Avg frequency    : %s", java_format_2f(ds.getMean()))
        logger.info("Variance         : %s", java_format_2f(ds.getVariance()))
        logger.info("STD              : %s", java_format_2f(ds.getStandardDeviation()))
