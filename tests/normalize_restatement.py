"""A flat restatement of the three normalisers (features/SumNormalizor.java, ZScoreNormalizor.java, LinearNormalizer.java) on the arguments
of rl_normalize_lists: (X, qoff, cols, row_len, times).  Written from the Java, not from ranklib_amd/normalizer.py nor from the kernel:
serial over a list's documents, as the Java's loops over rl.get(i) are, vectorised over the columns only (the columns are independent).
test_normalize_cpu.py holds it equal to normalizer.py list by list; test_gpu_normalize.py holds the GPU equal to it."""
import numpy as np

F32_MAX = np.finfo(np.float32).max            # Float.MAX_VALUE
F32_MIN = np.float32(1.4e-45)                 # Float.MIN_VALUE: the smallest positive subnormal
KINDS = ("sum", "zscore", "linear")


def java_min(a, b):
    """Math.min(float, float) elementwise: NaN if a is NaN; -0.0f below +0.0f; else a <= b ? a : b"""
    both_zero = (a == 0) & (b == 0)
    return np.where(np.isnan(a), a, np.where(both_zero & np.signbit(b), b, np.where(a <= b, a, b)))


def java_max(a, b):
    """Math.max(float, float) elementwise: NaN if a is NaN; +0.0f above -0.0f; else a >= b ? a : b"""
    both_zero = (a == 0) & (b == 0)
    return np.where(np.isnan(a), a, np.where(both_zero & np.signbit(a), b, np.where(a >= b, a, b)))


def _val(row):                                # DataPoint.getFeatureValue: NaN (unknown) reads as 0.0f
    return np.where(np.isnan(row), np.float32(0), row).astype(np.float32)


def _one_list(kind, L, cols):
    """L: the list's rows [n, stride] (a view, written in place); cols: an index array"""
    n = L.shape[0]
    with np.errstate(all="ignore"):
        if kind == "sum":
            norm = np.zeros(len(cols), np.float64)
            for i in range(n):
                norm = norm + np.abs(_val(L[i, cols])).astype(np.float64)
            ok = norm > 0
            for i in range(n):
                v = _val(L[i, cols]).astype(np.float64)
                L[i, cols[ok]] = (v[ok] / norm[ok]).astype(np.float32)
        elif kind == "zscore":
            mean = np.zeros(len(cols), np.float64)
            for i in range(n):
                mean = mean + _val(L[i, cols]).astype(np.float64)
            mean = mean / np.float64(n)
            std = np.zeros(len(cols), np.float64)
            for i in range(n):
                x = _val(L[i, cols]).astype(np.float64) - mean
                std = std + x * x
            std = np.sqrt(std / np.float64(n - 1))                 # n = 1: 0 / 0 = NaN
            ok = std > 0
            for i in range(n):
                v = _val(L[i, cols]).astype(np.float64)
                L[i, cols[ok]] = ((v[ok] - mean[ok]) / std[ok]).astype(np.float32)
        elif kind == "linear":
            lo = np.full(len(cols), F32_MAX, np.float32)
            hi = np.full(len(cols), F32_MIN, np.float32)
            for i in range(n):
                v = _val(L[i, cols])
                lo, hi = java_min(lo, v).astype(np.float32), java_max(hi, v).astype(np.float32)
            ok = hi > lo
            for i in range(n):
                v = _val(L[i, cols])
                L[i, cols] = np.where(ok, ((v - lo) / (hi - lo)).astype(np.float32), np.float32(0))
        else:
            raise ValueError(kind)


def normalize_lists(X, qoff, cols, kind, row_len=None, times=1):
    """A normalised copy of X.  row_len only says which cells exist: a requested column at or past a row's end is the caller's error."""
    X = np.array(X, np.float32, copy=True, order="C")
    cols = np.asarray(cols, np.int64)
    assert len(set(cols.tolist())) == len(cols) and cols.min() >= 1 and cols.max() < X.shape[1] and times >= 1
    if row_len is not None:
        assert np.min(row_len) > cols.max()
    for q in range(len(qoff) - 1):
        L = X[qoff[q]:qoff[q + 1]]
        for _ in range(times):
            _one_list(kind, L, cols)
    return X


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- test data ------------------------------------------------------------------------------------------------------------------------------
def adversarial_columns(n, rng):
    """columns of n documents built to break a normaliser, by name"""
    sub = np.float32(2.0 ** -149)
    c = {}
    c["constant"] = np.full(n, 7.5, np.float32)
    c["all +0"] = np.zeros(n, np.float32)
    z = np.zeros(n, np.float32); z[0::2] = -0.0
    c["-0 then +0"] = z
    z = np.zeros(n, np.float32); z[1::2] = -0.0
    c["+0 then -0"] = z
    c["no positive"] = -np.abs(rng.randn(n)).astype(np.float32)
    v = rng.randn(n).astype(np.float32); v[rng.rand(n) < 0.4] = np.nan
    c["nan cells"] = v
    c["all nan"] = np.full(n, np.nan, np.float32)
    v = np.full(n, np.nan, np.float32).view(np.uint32); v[:] = 0x7FC01234 + np.arange(n, dtype=np.uint32)   # payloads must survive where nothing is set
    c["nan payloads"] = v.view(np.float32)
    v = rng.randn(n).astype(np.float32); v[0] = np.inf
    c["+inf"] = v
    v = rng.randn(n).astype(np.float32); v[-1] = -np.inf
    c["-inf"] = v
    v = rng.randn(n).astype(np.float32); v[0] = np.inf; v[-1] = -np.inf
    c["both inf"] = v
    c["subnormals"] = (rng.randint(-40, 40, n).astype(np.float32) * sub).astype(np.float32)
    c["near FLT_MAX"] = (F32_MAX * (1 - rng.rand(n) * 1e-3) * rng.choice([-1, 1], n)).astype(np.float32)
    v = np.abs(rng.randn(n)).astype(np.float32) * np.float32(1e30); v[0] = np.float32(3e-12)
    c["subnormal quotient"] = v                                      # 3e-12 / ~1e30: sum's result is an f32 subnormal
    c["tiny and huge"] = (rng.randn(n) * 10.0 ** rng.randint(-30, 30, n)).astype(np.float32)
    return c


def make_file(lengths, n_cols, stride, seed, adversarial=True, scattered=False):
    """(X [n, stride], qoff, cols): one list per length, random columns of mixed scales with the adversarial columns dealt round robin
    over the lists' columns; column 0 and the columns not requested hold values that must survive"""
    rng = np.random.RandomState(seed)
    qoff = np.zeros(len(lengths) + 1, np.int32)
    qoff[1:] = np.cumsum(lengths)
    n = int(qoff[-1])
    X = (rng.randn(n, stride) * 10.0 ** rng.randint(-3, 4, (1, stride))).astype(np.float32)
    X[:, 0] = np.nan
    cols = (rng.permutation(np.arange(1, stride))[:n_cols] if scattered else np.arange(1, n_cols + 1)).astype(np.int32)
    if adversarial:
        for q, ln in enumerate(lengths):
            adv = adversarial_columns(ln, rng)
            names = sorted(adv)
            names = names[(5 * q) % len(names):] + names[:(5 * q) % len(names)]      # few columns: every list starts at another pattern
            for j, name in enumerate(names[:n_cols]):
                X[qoff[q]:qoff[q + 1], cols[(j + q) % n_cols]] = adv[name]
    return X, qoff, cols
