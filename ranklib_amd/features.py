"""LETOR input: mirrors features/FeatureManager.java (readInput :187-245, readFeature :267-292,
getFeatureFromSampleVector :303-322) and utilities/FileUtils.smartReader (.gz by extension); and the way back, save :455-476, with
FeatureManager's own command line (main :37-169):

    python -m ranklib_amd.features -input f [-input g ...] -output dir [-shuffle [-seed n]] [-k n [-tvs x]] [-tts x]
    python -m ranklib_amd.features -feature_stats model.txt
"""
import gzip
import logging
import os

import numpy as np

from ._native import RankLibError
from .learning import DataPoint, JavaRandom, RankList

logger = logging.getLogger("ranklib_amd")


def smart_reader(path):
    return gzip.open(path, "rt", encoding="utf-8") if path.endswith(".gz") else open(path, "r", encoding="utf-8")


class FeatureManager:
    @staticmethod
    def readInput(inputFile, mustHaveRelDoc=False, useSparseRepresentation=False):
        samples = []
        countEntries = 0
        try:
            fast = FeatureManager._read_native(inputFile, mustHaveRelDoc)
            if fast is not None:
                samples, countEntries = fast
                logger.info("(%d ranked lists, %d entries read)", len(samples), countEntries)
                return samples
            with smart_reader(inputFile) as f:
                lastID, hasRel, rl = "", False, []
                for content in f:
                    content = content.strip()
                    if not content or content[0] == "#":
                        continue
                    qp = DataPoint(content)          # sparse only changes row storage in the reference
                    if lastID and lastID != qp.getID():
                        if not mustHaveRelDoc or hasRel:
                            samples.append(RankList(rl))
                        rl, hasRel = [], False
                    if qp.getLabel() > 0:
                        hasRel = True
                    lastID = qp.getID()
                    rl.append(qp)
                    countEntries += 1
                if rl and (not mustHaveRelDoc or hasRel):
                    samples.append(RankList(rl))
            logger.info("(%d ranked lists, %d entries read)", len(samples), countEntries)
        except RankLibError:
            raise
        except Exception as ex:       # noqa: BLE001
            raise RankLibError("Error in FeatureManager::readInput(): %s" % ex)
        return samples

    native = True                     # parse with librlhip's rl_letor_* (host code); False = the pure-Python reader below

    @staticmethod
    def _read_native(inputFile, mustHaveRelDoc):
        """The same lists as the loop in readInput, with the lines parsed by rl_letor_parse on all host threads.  Lines the native
        parser flags (anything but plain `number qid:token (digits:number)*`) go through DataPoint's own parser, in file order,
        so malformed input raises exactly what it raised before."""
        if not FeatureManager.native:
            return None
        try:
            from . import _native as N
            N.lib()
        except Exception:             # noqa: BLE001 -- no library (e.g. a CPU-only checkout): the Python reader still works
            return None
        cached = FeatureManager._cache_load(inputFile) if FeatureManager.cache else None
        if cached is not None:
            return FeatureManager._lists_from_arrays(cached, mustHaveRelDoc)
        raw = (gzip.open(inputFile, "rb") if inputFile.endswith(".gz") else open(inputFile, "rb")).read()
        try:
            raw.decode("ascii")
        except UnicodeDecodeError:    # non-ASCII text: offsets into the bytes would not be offsets into the str
            return None
        p = N.letor_parse(raw)
        text = raw.decode("ascii")     # ASCII: byte offsets are character offsets
        n, X, mf = p["n"], p["X"], p["max_fid"]
        rows = list(X)                 # row views, created at C speed
        labels, last, slow = p["labels"].tolist(), p["last_fid"].tolist(), p["slow"].tolist()
        qo, do, lo = p["qid_off"].tolist(), p["desc_off"].tolist(), p["line_off"].tolist()
        qe = (p["qid_off"] + p["qid_len"]).tolist()
        de = (p["desc_off"] + p["desc_len"]).tolist()
        le = (p["line_off"] + p["line_len"]).tolist()
        if FeatureManager.cache and not any(slow):
            FeatureManager._cache_save(inputFile, dict(
                X=X, labels=p["labels"], last_fid=p["last_fid"], max_fid=np.int32(mf),
                qids=np.array([text[qo[i]:qe[i]] for i in range(n)], dtype="S"), descs=np.array([text[do[i]:de[i]] for i in range(n)], dtype="S")))
        from_parsed = DataPoint.from_parsed
        samples, rl, lastID, hasRel = [], [], "", False
        for i in range(n):
            if slow[i]:
                qp = DataPoint(text[lo[i]:le[i]])
            else:
                row = rows[i]
                qp = from_parsed(labels[i], text[qo[i]:qe[i]], text[do[i]:de[i]], row if last[i] == mf else row[:last[i] + 1])
            if lastID and lastID != qp.id:
                if not mustHaveRelDoc or hasRel:
                    samples.append(RankList(rl))
                rl, hasRel = [], False
            if qp.label > 0:
                hasRel = True
            lastID = qp.id
            rl.append(qp)
        if rl and (not mustHaveRelDoc or hasRel):
            samples.append(RankList(rl))
        return samples, n

    # ---- binary cache of a parsed LETOR file (the text of an MSLR-WEB30K fold is 5 GB) -------------------------------
    # `<file>.rlcache.npz` next to the text: the dense row matrix, labels, largest feature id per line, qid and description strings.
    # Written after a native parse without irregular lines, used when it is newer than the text.  Off by default (the reference has
    # no such file); `python -m ranklib_amd.evaluator -cache ...` or FeatureManager.cache = True turn it on.
    cache = False

    @staticmethod
    def _cache_path(inputFile):
        return inputFile + ".rlcache.npz"

    @staticmethod
    def _cache_save(inputFile, arrays):
        try:
            tmp = FeatureManager._cache_path(inputFile) + ".tmp.npz"
            st = os.stat(inputFile)
            np.savez(tmp, src_size=np.int64(st.st_size), src_mtime_ns=np.int64(st.st_mtime_ns), **arrays)
            os.replace(tmp, FeatureManager._cache_path(inputFile))
        except OSError as ex:          # read-only directory: the cache is an optimisation
            logger.info("no LETOR cache written: %s", ex)

    @staticmethod
    def _cache_load(inputFile):
        path = FeatureManager._cache_path(inputFile)
        try:
            st = os.stat(inputFile)
            with np.load(path) as z:
                # the cache names the text it was made from (size and mtime in ns): a file rewritten within the timestamp granularity, or
                # restored with an older mtime (cp -p, rsync -t, git checkout), never yields stale rows
                if int(z["src_size"]) != st.st_size or int(z["src_mtime_ns"]) != st.st_mtime_ns:
                    return None
                return {k: z[k] for k in ("X", "labels", "last_fid", "max_fid", "qids", "descs")}
        except (OSError, KeyError, ValueError):
            return None

    @staticmethod
    def _lists_from_arrays(a, mustHaveRelDoc):
        X, mf = a["X"], int(a["max_fid"])
        rows, labels, last = list(X), a["labels"].tolist(), a["last_fid"].tolist()
        qids, descs = [q.decode("ascii") for q in a["qids"]], [d.decode("ascii") for d in a["descs"]]
        from_parsed = DataPoint.from_parsed
        samples, rl, lastID, hasRel = [], [], "", False
        for i in range(len(labels)):
            row = rows[i]
            qp = from_parsed(labels[i], qids[i], descs[i], row if last[i] == mf else row[:last[i] + 1])
            if lastID and lastID != qp.id:
                if not mustHaveRelDoc or hasRel:
                    samples.append(RankList(rl))
                rl, hasRel = [], False
            if qp.label > 0:
                hasRel = True
            lastID = qp.id
            rl.append(qp)
        if rl and (not mustHaveRelDoc or hasRel):
            samples.append(RankList(rl))
        return samples, len(labels)

    @staticmethod
    def readFeature(featureDefFile):
        fids = []
        with smart_reader(featureDefFile) as f:
            for content in f:
                content = content.strip()
                if not content or content[0] == "#":
                    continue
                fids.append(int(content.split("\t")[0].strip()))
        return fids

    @staticmethod
    def getFeatureFromSampleVector(samples):
        if not samples:
            raise RankLibError("Error in FeatureManager::getFeatureFromSampleVector(): There are no training samples.")
        fc = max(rl.getFeatureCount() for rl in samples)
        return list(range(1, fc + 1))

    @staticmethod
    def prepareSplit(samples, percentTrain):           # features/FeatureManager.java:432-443 (no shuffling: file order)
        size = int(len(samples) * percentTrain)
        return [RankList(rl) for rl in samples[:size]], [RankList(rl) for rl in samples[size:]]

    @staticmethod
    def prepareCV(samples, nFold, tvs=-1.0):           # :349-413: contiguous folds, the last one takes the remainder
        size = len(samples) // nFold
        folds, start, total = [], 0, 0
        for _ in range(nFold):
            t = [start + i for i in range(size) if start + i < len(samples)]
            folds.append(t)
            total += len(t)
            start += size
        while total < len(samples):
            folds[-1].append(total)
            total += 1
        trainingData, validationData, testData = [], [], []
        for t in folds:
            ts = set(t)
            train = [RankList(samples[j]) for j in range(len(samples)) if j not in ts]
            test = [RankList(samples[j]) for j in range(len(samples)) if j in ts]
            vali = []
            if tvs > 0:                                # the LAST lists of the training part, taken back to front (:391-397)
                validationSize = int(len(train) * (1.0 - tvs))
                for _ in range(validationSize):
                    vali.append(train.pop())
            trainingData.append(train)
            testData.append(test)
            if tvs > 0:
                validationData.append(vali)
        return trainingData, validationData, testData

    @staticmethod
    def printQueriesForSplit(name, split):              # :413-428
        if split is None:
            logger.info("No %s split.", name)
            return
        for i, rankLists in enumerate(split):
            logger.info("%s[%d]=", name, i)
            for rl in rankLists:
                logger.info(" \"%s\"", rl.getID())

    @staticmethod
    def readInputs(inputFiles):                          # readInput(List<String>) :252-260: the files in order, one after the other
        samples = []
        for f in inputFiles:
            samples.extend(FeatureManager.readInput(f, False, False))
        return samples

    @staticmethod
    def shuffle(samples, seed):
        """Collections.shuffle(samples, new Random(seed)) in place: for i = size .. 2: swap(i - 1, rnd.nextInt(i)).  Past the JDK's
        SHUFFLE_THRESHOLD the Java shuffles an array copy with the same draws and swaps, so this one loop is both.  The Java's own call is
        unseeded (:116); the seed is an rlhip extension."""
        rnd = JavaRandom(seed)
        for i in range(len(samples), 1, -1):
            j = rnd.nextInt(i)
            samples[i - 1], samples[j] = samples[j], samples[i - 1]
        return samples

    # ---- writing LETOR text: save :455-476, a DataPoint.toString() and a newline per document ------------------------------------------
    SAVE_CHUNK = 65536                # documents formatted per native call: bounds the text held in memory

    @staticmethod
    def save(samples, outputFile):
        """The lines go through rl_letor_format (FeatureManager.native, like the reader) in chunks of SAVE_CHUNK documents; a chunk with
        a non-ASCII id or description, and every chunk when the library does not load, goes through DataPoint.toString.  The bytes are
        the same either way.  Kept from the Java: (int) label truncates a fractional label."""
        docs = [dp for rl in samples for dp in rl.rl]
        fmt = FeatureManager._native_format()
        try:
            with open(outputFile, "wb") as out:
                buf = None
                for a in range(0, len(docs), FeatureManager.SAVE_CHUNK):
                    chunk = docs[a:a + FeatureManager.SAVE_CHUNK]
                    text = None
                    if fmt is not None:
                        text, buf = FeatureManager._format_chunk(fmt, chunk, buf)
                    if text is None:
                        text = "".join(dp.toString() + "\n" for dp in chunk).encode("utf-8")
                    out.write(text)
        except RankLibError:
            raise
        except Exception as ex:       # noqa: BLE001 -- the reference wraps everything
            raise RankLibError("Error in FeatureManager::save(): %s" % ex)

    @staticmethod
    def _native_format():
        if not FeatureManager.native:
            return None
        try:
            from . import _native as N
            return N.letor_format if hasattr(N.lib(), "rl_letor_format") else None
        except Exception:             # noqa: BLE001 -- no library (e.g. a CPU-only checkout): the Python writer still works
            return None

    @staticmethod
    def _format_chunk(fmt, chunk, buf):
        """(text of the chunk or None when it is not ASCII, the buffer to reuse)"""
        n = len(chunk)
        ids, descs = [dp.id for dp in chunk], [dp.description for dp in chunk]
        try:
            strings = ("".join(ids) + "".join(descs)).encode("ascii")
        except UnicodeEncodeError:    # offsets into the bytes would not be offsets into the str
            return None, buf
        qid_len = np.fromiter(map(len, ids), np.int32, count=n)
        desc_len = np.fromiter(map(len, descs), np.int32, count=n)
        qid_off = np.cumsum(qid_len, dtype=np.int64) - qid_len
        desc_off = int(qid_len.sum(dtype=np.int64)) + np.cumsum(desc_len, dtype=np.int64) - desc_len
        row_len = np.fromiter((len(dp.fVals) for dp in chunk), np.int32, count=n)
        stride = int(row_len.max())
        if int(row_len.min()) == stride:
            X = np.array([dp.fVals for dp in chunk], np.float32).reshape(n, stride)
        else:
            X = np.full((n, stride), np.nan, np.float32)
            for i, dp in enumerate(chunk):
                X[i, :row_len[i]] = dp.fVals
        labels = np.fromiter((dp.label for dp in chunk), np.float32, count=n)
        # an upper bound of the text: "-2147483648 qid:" id " ", per cell "fid:" a Float.toString of at most 15 characters and a space,
        # " " description "\n".  Pages the text does not reach are never touched
        bound = len(strings) + n * 19 + int(row_len.sum(dtype=np.int64)) * (len(str(stride)) + 17)
        if buf is None or buf.size < bound:
            buf = np.empty(bound, np.uint8)
        return fmt(X, row_len, labels, strings, qid_off, qid_len, desc_off, desc_len, buf), buf


def _file_name(pathName):             # FileUtils.getFileName :230-235
    return pathName[max(pathName.rfind("/"), pathName.rfind("\\")) + 1:]


USAGE = """Usage: python -m ranklib_amd.features <Params>
Params:
\t-input <file>\t\tSource data (ranked lists)
\t-output <dir>\t\tThe output directory
  [+] Shuffling
\t-shuffle\t\tCreate a copy of the input file in which the ordering of all ranked lists (e.g. queries) is randomized.
\t\t\t\t(the order among objects (e.g. documents) within each ranked list is certainly unchanged).
\t[ -seed <n> ]\t\tSeed of the shuffle (rlhip extension; without it one is drawn and logged)
  [+] k-fold Partitioning (sequential split)
\t-k <fold>\t\tThe number of folds
\t[ -tvs <x \\in [0..1]> ] Train-validation split ratio (x)(1.0-x)
  [+] Train-test split
\t-tts <x \\in [0..1]> ] Train-test split ratio (x)(1.0-x)
  NOTE: If both -shuffle and -k are specified, the input data will be shuffled and then sequentially partitioned.
Feature Statistics -- Saved model feature use frequencies and statistics.
-input and -output parameters are not used.
\t-feature_stats\tName of a saved, feature-limited, LTR model text file.
\t\t\tDoes not process Coordinate Ascent, LambdaRank, ListNet or RankNet models.
\t\t\tas they include all features rather than selected feature subsets."""


def main(argv=None):                  # features/FeatureManager.java:37-169
    """python -m ranklib_amd.features: -input f (repeatable) -output dir [-shuffle [-seed n]] [-k n [-tvs x]] [-tts x] | -feature_stats model.
    Flags are matched case-insensitively and unknown ones ignored, as written; -seed is an rlhip extension (the Java's shuffle is unseeded)."""
    import sys
    args = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    has_stats = "-feature_stats" in args                 # :50-51: this test, unlike the loop below, is case-sensitive
    if (len(args) < 3 and not has_stats) or (len(args) != 2 and has_stats):
        for line in USAGE.split("\n"):
            logger.info(line)
        return 0
    rankingFiles, outputDir, modelFileName = [], "", ""
    shuffle = doFeatureStats = False
    nFold, tvs, tts, seed = 0, np.float32(-1), np.float32(-1), None
    from .evaluator import ArgCursor                     # (the evaluator imports this module)
    cur = ArgCursor(args)
    nxt = cur.nxt
    for a in cur:                                        # :79-96
        if a == "-input": rankingFiles.append(nxt())
        elif a == "-k": nFold = int(nxt())
        elif a == "-shuffle": shuffle = True
        elif a == "-tvs": tvs = np.float32(nxt())       # Float.parseFloat: the splits below are computed from the float's value
        elif a == "-tts": tts = np.float32(nxt())
        elif a == "-output":
            outputDir = nxt()                            # FileUtils.makePathStandard :237-244
            if outputDir[-1:] not in ("/", "\\"):
                outputDir += os.sep
        elif a == "-feature_stats":
            doFeatureStats = True
            modelFileName = nxt()
        elif a == "-seed": seed = int(nxt())
    if nFold > 0 and tts != -1:                          # :98-101
        logger.info("Error: Only one of k or tts should be specified.")
        return 0
    if shuffle or nFold > 0 or tts != -1:
        samples = FeatureManager.readInputs(rankingFiles)
        if not samples:
            logger.info("Error: The input file is empty.")
            return 0
        fn = _file_name(rankingFiles[0])
        if shuffle:                                      # :113-119
            fn += ".shuffled"
            logger.info("Shuffling... ")
            if seed is None:
                seed = int.from_bytes(os.urandom(8), "little", signed=True)
                logger.info("seed = %d", seed)
            FeatureManager.shuffle(samples, seed)
            logger.info("Saving... ")
            FeatureManager.save(samples, outputDir + fn)
        if tts != -1:                                    # :121-135
            logger.info("Splitting... ")
            trains, tests = FeatureManager.prepareSplit(samples, float(tts))
            logger.info("Saving splits...")
            FeatureManager.save(trains, outputDir + "train." + fn)
            FeatureManager.save(tests, outputDir + "test." + fn)
        if nFold > 0:                                    # :137-158
            logger.info("Partitioning... ")
            trains, valis, tests = FeatureManager.prepareCV(samples, nFold, float(tvs))
            FeatureManager.printQueriesForSplit("Train", trains)         # prepareCV's own lines :408-410, on this path only
            FeatureManager.printQueriesForSplit("Validate", valis)
            FeatureManager.printQueriesForSplit("Test", tests)
            for f in range(len(trains)):
                logger.info("Saving fold %d/%d... ", f + 1, nFold)
                FeatureManager.save(trains[f], outputDir + "f%d.train.%s" % (f + 1, fn))
                FeatureManager.save(tests[f], outputDir + "f%d.test.%s" % (f + 1, fn))
                if tvs > 0:
                    FeatureManager.save(valis[f], outputDir + "f%d.validation.%s" % (f + 1, fn))
    elif doFeatureStats:                                 # :159-168
        from .feature_stats import FeatureStats
        FeatureStats(modelFileName).writeFeatureStats()
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
