"""ciir.umass.edu.eval.Analyzer: compares the per-ranked-list performance files that `-test ... -idv out` writes
(Evaluator.savePerRankListPerformanceFile) of several systems with a baseline's: win and loss counts, an improvement histogram and a
Fisher randomisation p-value (ranklib_amd/stats.py; its sums run on the GPU).  DESIGN.md 18.

    python -m ranklib_amd.analyzer -all <directory> -base <file> [-np n] [-npseed s]

The log lines are the Java's.  Two deviations in the file layer, both stated in DESIGN.md 18: the directory's names are sorted (the Java
takes File.list()'s unspecified order), and where the Java ends in an unchecked exception (a short line, a number that does not parse,
a missing "all" entry, a change above 1000 or NaN, a target skipped as not comparable when the break-down is printed) a RankLibError
says which file and what.
"""
import logging
import math
import os
import re
import sys

from .features import smart_reader
from .learning import java_double_str, java_round
from .stats import RandomPermutationTest, java_hashmap_order
from ._native import RankLibError

logger = logging.getLogger("ranklib_amd")

_JAVA_TRIM = "".join(chr(c) for c in range(0x21))          # String.trim(): every char <= ' '
# Double.parseDouble's decimal grammar (FloatingDecimal.readJavaFormatString): optional sign, NaN / Infinity, or digits with an optional
# point, an optional exponent and an optional type suffix.  Hex floats are refused here (the Java takes them; no writer of these files
# produces one).
_JAVA_DECIMAL = re.compile(r"^[+-]?(?:NaN|Infinity|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?[fFdD]?)$")
_JAVA_HEX = re.compile(r"^[+-]?0[xX]")


def parse_java_double(text):
    """Double.parseDouble(text) for the forms DESIGN.md 18 lists; ValueError (with a message) for everything else"""
    s = text.strip(_JAVA_TRIM)
    if _JAVA_HEX.match(s):
        raise ValueError("hexadecimal floating-point literal '%s' is not read here" % text)
    if not _JAVA_DECIMAL.match(s):
        raise ValueError("'%s' is not a Java double" % text)
    body = s.lstrip("+-")
    neg = s.startswith("-")
    if body == "NaN":
        return float("nan")
    if body == "Infinity":
        return float("-inf") if neg else float("inf")
    if body[-1] in "fFdD":
        body = body[:-1]
    v = float(body)
    return -v if neg else v


def _file_name(pathName):             # FileUtils.getFileName :230-235
    return pathName[max(pathName.rfind("/"), pathName.rfind("\\")) + 1:]


class Result:                         # Analyzer.java:51-56
    def __init__(self):
        self.status = 0               # success
        self.win = 0
        self.loss = 0
        self.countByImprovementRange = None


class Analyzer:
    improvementRatioThreshold = [-1, -0.75, -0.5, -0.25, 0, 0.25, 0.5, 0.75, 1, 1000]      # :59
    indexOfZero = 4

    def __init__(self):
        self.randomizedTest = RandomPermutationTest()

    def locateSegment(self, value):   # :62-77
        thr = Analyzer.improvementRatioThreshold
        if value > 0:
            for i in range(Analyzer.indexOfZero, len(thr)):
                if value <= thr[i]:
                    return i
        elif value < 0:
            for i in range(0, Analyzer.indexOfZero + 1):
                if value < thr[i]:
                    return i
        return -1

    def read(self, filename):         # :84-109; the dict keeps HashMap.put's rule: a later line with the same id replaces the value in place
        performance = {}
        try:
            with smart_reader(filename) as f:
                for lineno, content in enumerate(f, 1):
                    content = content.rstrip("\r\n").strip(_JAVA_TRIM)
                    if len(content) == 0:
                        continue
                    while "  " in content:
                        content = content.replace("  ", " ")
                    s = content.replace(" ", "\t").split("\t")
                    if len(s) < 3:
                        raise RankLibError("%s line %d: expecting 'metric id performance', found %d field(s) "
                                           "(an ArrayIndexOutOfBoundsException in the Java)" % (filename, lineno, len(s)))
                    try:
                        performance[s[1]] = parse_java_double(s[2])
                    except ValueError as ex:
                        raise RankLibError("%s line %d: %s (a NumberFormatException in the Java)" % (filename, lineno, ex))
        except OSError as ex:
            raise RankLibError(str(ex))
        java_hashmap_order(list(performance.keys()), filename)          # refuses ids whose HashMap order is not restated
        logger.info("Reading %s... %d ranked lists", filename, len(performance))
        return performance

    def compare(self, a, b):
        """the Java's overloads: (directory, baseFile) :116-128, (targetFiles, baseFile) :135-192, (base, targets) :200-207 and
        (base, target) :215-245"""
        if isinstance(a, str):
            return self._compare_directory(a, b)
        if isinstance(a, dict):
            return self._compare_maps(a, b) if isinstance(b, dict) else [self._compare_maps(a, t) for t in b]
        return self._compare_files(list(a), b)

    def _compare_directory(self, directory, baseFile):
        if directory[-1:] not in ("/", "\\"):                 # FileUtils.makePathStandard
            directory += os.sep
        names = sorted(os.listdir(directory)) if os.path.isdir(directory) else []          # File.list(): here sorted
        self._compare_files([directory + n for n in names if n != baseFile], directory + baseFile)

    def _compare_maps(self, base, target):
        r = Result()
        if len(base) != len(target):
            r.status = -1
            return r
        r.countByImprovementRange = [0] * len(Analyzer.improvementRatioThreshold)
        for key in java_hashmap_order(list(base.keys())):
            if key not in target:
                r.status = -2
                return r
            if key == "all":
                continue
            p, pt = base[key], target[key]
            if pt > p:
                r.win += 1
            elif pt < p:
                r.loss += 1
            change = pt - p
            if change != 0:
                seg = self.locateSegment(change)
                if seg < 0:
                    raise RankLibError("Analyzer: ranked list '%s' changes by %s, outside every improvement range "
                                       "(an ArrayIndexOutOfBoundsException in the Java)" % (key, java_double_str(change)))
                r.countByImprovementRange[seg] += 1
        return r

    def _compare_files(self, targetFiles, baseFile):
        base = self.read(baseFile)
        targets = [self.read(f) for f in targetFiles]
        rs = self.compare(base, targets)
        ok = [i for i in range(len(rs)) if rs[i].status == 0]
        logger.info("Overall comparison")
        logger.info("System\tPerformance\tImprovement\tWin\tLoss\tp-value")
        if "all" not in base:
            raise RankLibError("%s has no 'all' entry (a NullPointerException in the Java)" % baseFile)
        logger.info("%s [baseline]\t%s", _file_name(baseFile), java_double_str(_round(base["all"], 4)))
        pvalue = dict(zip(ok, self.randomizedTest.test_all([targets[i] for i in ok], base, baseFile)))       # one launch for all targets
        for i in range(len(rs)):
            if rs[i].status == 0:
                delta = targets[i]["all"] - base["all"]
                dp = _java_div(delta * 100, base["all"])
                plus = "+" if delta > 0 else ""
                logger.info("%s\t%s\t%s%s (%s%s%%)\t%d\t%d\t%s", _file_name(targetFiles[i]), java_double_str(_round(targets[i]["all"], 4)),
                            plus, java_double_str(_round(delta, 4)), plus, java_double_str(_round(dp, 2)), rs[i].win, rs[i].loss,
                            java_double_str(pvalue[i]))
            else:
                logger.warning("WARNING: [%s] skipped: NOT comparable to the baseline due to different ranked list IDs.", targetFiles[i])
        logger.info("Detailed break down")
        thr = Analyzer.improvementRatioThreshold
        tmp = [("+" if v > 0 else "") + "%d%%" % int(v * 100) for v in thr]
        header = "[ < " + tmp[0] + ")\t"
        for i in range(len(thr) - 2):
            header += ("(%s, %s]\t" if i >= Analyzer.indexOfZero else "[%s, %s)\t") % (tmp[i], tmp[i + 1])
        header += "( > " + tmp[len(thr) - 2] + "]"
        logger.info("\t" + header)
        for i in range(len(targets)):
            if rs[i].countByImprovementRange is None:
                raise RankLibError("%s holds %d ranked lists, the baseline %d: no break-down for it (a NullPointerException in the Java)"
                                   % (targetFiles[i], len(targets[i]), len(base)))
            logger.info(_file_name(targetFiles[i]) + "".join("\t%d" % e for e in rs[i].countByImprovementRange))


def _round(val, n):
    """SimpleMath.round(val, n) :54-60 for every double (Math.floor passes NaN and the infinities through)"""
    x = val * 10 ** n + .5
    return java_round(val, n) if math.isfinite(x) else x / 10 ** n


def _java_div(a, b):
    """a / b of two Java doubles (no ZeroDivisionError)"""
    if b != 0:
        return a / b
    if a != a or a == 0:
        return float("nan")
    return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def main(argv=None):                  # :24-49
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if len(args) < 2:
        logger.info("Usage: java -cp bin/RankLib.jar ciir.umass.edu.eval.Analyzer <Params>")
        logger.info("Params:")
        logger.info("\t-all <directory>\tDirectory of performance files (one per system)")
        logger.info("\t-base <file>\t\tPerformance file for the baseline (MUST be in the same directory)")
        logger.info("\t[ -np ] \t\tNumber of permutation (Fisher randomization test) [default=%d]", RandomPermutationTest.nPermutation)
        logger.info("\t[ -npseed ] \t\tSeed of the permutations' java.util.Random (rlhip extension) [default=drawn and logged]")
        return 0
    directory = baseline = ""
    saved = (RandomPermutationTest.nPermutation, RandomPermutationTest.seed)
    try:
        i = 0
        while i < len(args):
            if args[i] in ("-all", "-base", "-np", "-npseed"):
                if i + 1 >= len(args):
                    raise RankLibError("Missing value for " + args[i])
                i += 1
                if args[i - 1] == "-all":
                    directory = args[i]
                elif args[i - 1] == "-base":
                    baseline = args[i]
                else:
                    if not re.match(r"^[+-]?[0-9]+$", args[i]):
                        raise RankLibError("%s takes an integer, not '%s' (a NumberFormatException in the Java)" % (args[i - 1], args[i]))
                    v = int(args[i])
                    if args[i - 1] == "-np":
                        if not -2 ** 31 <= v < 2 ** 31:
                            raise RankLibError("-np takes a Java int, not '%s'" % args[i])
                        RandomPermutationTest.nPermutation = v
                    else:
                        if not -2 ** 63 <= v < 2 ** 63:
                            raise RankLibError("-npseed takes a Java long, not '%s'" % args[i])
                        RandomPermutationTest.seed = v
            i += 1
        if not directory:
            raise RankLibError("-all <directory> is missing (a StringIndexOutOfBoundsException in the Java)")
        Analyzer().compare(directory, baseline)
        return 0
    finally:
        RandomPermutationTest.nPermutation, RandomPermutationTest.seed = saved


if __name__ == "__main__":
    sys.exit(main())
