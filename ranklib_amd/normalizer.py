"""Feature normalisation of the reference's command line (`-norm sum | zscore | linear`, eval/Evaluator.java:256-267): every ranked list
is normalised on its own, in place, before training / scoring.  Mirrors features/SumNormalizor.java, ZScoreNormalizor.java and
LinearNormalizer.java operation by operation -- the sums are sequential f64 sums over the list in document order, the casts to float
happen where the Java's do -- because the normalised values are what LambdaMART.init() builds its thresholds from.

normalize(rl, fids) -- one list -- is host numpy, as the reference's is host-side Java.  normalizeAll hands a whole file to the GPU in one
call (rl_normalize_lists, DESIGN.md 20: the same operations, one lane per list and column) where that changes nothing but the time; with
Normalizer.batch = False, without a device, and for every file whose rows do not all hold every requested feature it runs list by list."""
import numpy as np

from .learning import DataPoint, RankLibError


def _unique(fids):                    # features/Normalizer.java:31-44 (a HashSet: order is irrelevant, the features are independent)
    seen, out = set(), []
    for f in fids:
        if f not in seen:
            seen.add(f)
            out.append(int(f))
    return out


def _gather(rl, fids, who):
    """[documents, len(fids)] float32 through DataPoint.getFeatureValue (NaN = unknown -> 0; a feature past a row's end is an error
    unless -missingZero, learning/DenseDataPoint.java:21-32)"""
    if rl.size() == 0:
        raise RankLibError("Error in %s::normalize(): The input ranked list is empty" % who)
    if fids and min(fids) > 0 and all(len(dp.fVals) > max(fids) for dp in rl.rl):
        # every row names every requested feature: one fancy index per list instead of a Python visit per cell
        # (rows are ragged -- each ends at its own last feature id -- so every row is cut to the requested ids before the stack)
        return np.nan_to_num(np.stack([np.asarray(dp.fVals, np.float32)[fids] for dp in rl.rl]), nan=0.0, posinf=np.inf, neginf=-np.inf)
    M = np.zeros((rl.size(), len(fids)), np.float32)
    for i, dp in enumerate(rl.rl):
        fv = dp.fVals
        for j, f in enumerate(fids):
            if f <= 0 or f >= len(fv):
                if not DataPoint.missingZero:
                    raise RankLibError("Error in DenseDataPoint::getFeatureValue(): requesting unspecified feature, fid=%d" % f)
            elif not np.isnan(fv[f]):
                M[i, j] = fv[f]
    return M


def _scatter(rl, fids, M, mask):
    """DataPoint.setFeatureValue for the columns in `mask` (learning/DenseDataPoint.java:35-40: a feature past the row's end is an error)"""
    cols = [j for j in range(len(fids)) if mask[j]]
    if cols and min(fids[j] for j in cols) > 0 and all(len(dp.fVals) > max(fids[j] for j in cols) for dp in rl.rl):
        ids = [fids[j] for j in cols]
        for i, dp in enumerate(rl.rl):
            dp.fVals[ids] = M[i, cols]
        return
    for i, dp in enumerate(rl.rl):
        fv = dp.fVals
        for j, f in enumerate(fids):
            if mask[j]:
                if f <= 0 or f >= len(fv):
                    raise RankLibError("Error in DenseDataPoint::setFeatureValue(): feature (id=%d) not found." % f)
                fv[f] = M[i, j]


def _seq_sum(A):                      # `acc += a[i]` over the documents, in order, in f64 (np.sum would add pairwise)
    return np.add.accumulate(A.astype(np.float64), axis=0)[-1]


def _device_visible():
    try:
        from . import _native as N
        return hasattr(N.lib(), "rl_normalize_lists") and N.device_count() > 0
    except Exception:                 # noqa: BLE001 -- no library (a CPU-only checkout): the host path still works
        return False


def _row_matrix(fvs, lens):
    """(B, first row) when the rows `fvs` are, in order, consecutive row views of one C-contiguous float32 matrix B (what the native
    reader and the -cache reader make: `list(X)`, a short row cut to its own length); else None.  O(1) attribute reads per row."""
    B = fvs[0].base
    if not (isinstance(B, np.ndarray) and B.ndim == 2 and B.dtype == np.float32 and B.flags.c_contiguous and B.flags.writeable):
        return None
    step = B.shape[1] * 4
    if step == 0 or max(lens) > B.shape[1]:
        return None
    for fv in fvs:
        if fv.base is not B or fv.strides != (4,):
            return None
    addr = np.fromiter((fv.__array_interface__["data"][0] for fv in fvs), np.int64, len(fvs))
    off = int(addr[0]) - B.ctypes.data
    if off < 0 or off % step or off // step + len(fvs) > B.shape[0] or np.any(np.diff(addr) != step):
        return None
    return B, off // step


class Normalizer:
    batch = True                      # rlhip: normalizeAll hands a whole file to the GPU in one call (_native.normalize_lists)
                                      # when a device is visible; False: list by list on the host, the same bits
    kind = None                       # the name rl_normalize_lists knows the subclass by

    def normalize(self, rl, fids=None):
        raise NotImplementedError

    def normalizeAll(self, samples, fids=None):       # Normalizer.normalize(List<RankList>[, fids])
        if self.normalizeBatch(samples, fids):
            return
        for rl in samples:
            self.normalize(rl, fids)

    def normalizeBatch(self, samples, fids=None, times=1):
        """Every list of `samples` normalised `times` times in a row on the GPU; True when done.  False -- and nothing touched -- when
        `batch` is off, no device is visible, or the list-by-list path would do anything but plain arithmetic on rows that hold every
        requested feature: an empty list, a feature id a row does not name (an error, or -missingZero's 0), lists of different feature
        counts without `fids`.  Rows that are views of one matrix are normalised there, in place; other rows are copied in and out."""
        if not (Normalizer.batch and self.kind and samples and _device_visible()):
            return False
        if any(rl.size() == 0 for rl in samples):
            return False
        if fids is None:
            fc = samples[0].getFeatureCount()
            if any(rl.getFeatureCount() != fc for rl in samples):
                return False
            cols = list(range(1, fc + 1))
        else:
            cols = _unique(fids)
        if not cols or min(cols) < 1:
            return False
        fvs = [dp.fVals for rl in samples for dp in rl.rl]
        if any(not isinstance(fv, np.ndarray) or fv.dtype != np.float32 or fv.ndim != 1 or not fv.flags.writeable for fv in fvs):
            return False
        lens = list(map(len, fvs))
        need = max(cols) + 1
        if min(lens) < need or len(set(map(id, fvs))) != len(fvs):   # (a row listed twice would be normalised twice over, one after the other)
            return False
        from . import _native as N
        qoff = np.zeros(len(samples) + 1, np.int32)
        np.cumsum([rl.size() for rl in samples], out=qoff[1:])
        whole = _row_matrix(fvs, lens)
        if whole is not None:
            B, r0 = whole
            N.normalize_lists(B[r0:r0 + len(fvs)], qoff, cols, self.kind, row_len=lens, times=times)
            return True
        M = np.stack([fv[:need] for fv in fvs])       # one visit per DataPoint; the columns past the last requested one stay where they are
        N.normalize_lists(M, qoff, cols, self.kind, times=times)
        for fv, row in zip(fvs, M):
            fv[:need] = row                           # the cells the kernel left alone come back with the bits they went with
        return True

    @staticmethod
    def _fids(rl, fids):
        return list(range(1, rl.getFeatureCount() + 1)) if fids is None else _unique(fids)


class SumNormalizor(Normalizer):      # features/SumNormalizor.java:18-70
    kind = "sum"

    def name(self):
        return "sum"

    def normalize(self, rl, fids=None):
        fids = self._fids(rl, fids)
        M = _gather(rl, fids, "SumNormalizor")
        norm = _seq_sum(np.abs(M))                                   # norm[j] += Math.abs(value): double += float
        ok = norm > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            out = (M.astype(np.float64) / norm).astype(np.float32)   # (float)(value / norm[j])
        _scatter(rl, fids, out, ok)


class ZScoreNormalizor(Normalizer):   # features/ZScoreNormalizor.java:18-92
    kind = "zscore"

    def name(self):
        return "zscore"

    def normalize(self, rl, fids=None):
        fids = self._fids(rl, fids)
        M = _gather(rl, fids, "ZScoreNormalizor").astype(np.float64)
        n = M.shape[0]
        means = _seq_sum(M) / n
        d = M - means                                                # x = value - mean (double)
        with np.errstate(divide="ignore", invalid="ignore"):
            std = np.sqrt(_seq_sum(d * d) / (n - 1))                 # a list of one document: 0 / 0 = NaN, `std > 0` is false
            out = (d / std).astype(np.float32)
        _scatter(rl, fids, out, std > 0)


class LinearNormalizer(Normalizer):   # features/LinearNormalizer.java:18-68
    kind = "linear"

    def name(self):
        return "linear"

    def normalize(self, rl, fids=None):
        fids = self._fids(rl, fids)
        M = _gather(rl, fids, "LinearNormalizor")
        # min starts at Float.MAX_VALUE, max at Float.MIN_VALUE -- the smallest POSITIVE float (:38-39): a column without a positive value keeps it
        lo = np.minimum(M.min(axis=0), np.finfo(np.float32).max)
        hi = np.maximum(M.max(axis=0), np.float32(1.4e-45))
        span = hi - lo                                               # float arithmetic throughout (:52)
        ok = hi > lo
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(ok, (M - lo) / span, np.float32(0)).astype(np.float32)
        _scatter(rl, fids, out, np.ones(len(fids), bool))            # else: setFeatureValue(fid, 0)


def create(name):                     # eval/Evaluator.java:258-267
    n = name.lower()
    if n == "sum":
        return SumNormalizor()
    if n == "zscore":
        return ZScoreNormalizor()
    if n == "linear":
        return LinearNormalizer()
    raise RankLibError("Unknown normalizor: " + name)
