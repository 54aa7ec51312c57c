"""RL_FLAG_FAST_LEAF restated in numpy: the fixed f64 reduction of a leaf's values and the output rule.  Test infrastructure only.

    B(v), at most 256 values: pad to 256 with +0.0; for s = 128, 64, .., 1: a[i] = a[i] + a[i + s] for all i < s; the result is a[0]
    R(x): n == 0 -> 0.0; else replace the sequence by [B(x[256 j : 256 j + 256]) for j] until one value is left (n == 1 still passes through one B);
          finally add +0.0
    LambdaMART: s1 = (float) R(pseudoResponses), s2 = (float) R(weights), output = 0 if s2 == 0 else s1 / s2 in float (LambdaMART.java:409-413)
    MART:       output = s1 / (float) count                                                                    (MART.java:64)

numpy's float64 `+` is the IEEE add, one rounding per operation, nothing fused: every line below is the definition as written.
"""
import numpy as np

TILE = 256
F32 = np.float32


def B_rows(a):
    """B of every row of a [T, 256] float64 array (already padded)"""
    a = np.array(a, np.float64, copy=True)
    assert a.ndim == 2 and a.shape[1] == TILE
    s = TILE // 2
    while s >= 1:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    return a[:, 0].copy()


def B(v):
    v = np.asarray(v, np.float64)
    assert 0 < len(v) <= TILE
    a = np.zeros((1, TILE), np.float64)          # +0.0 padding
    a[0, :len(v)] = v
    return B_rows(a)[0]


def level(x):
    """one level: the B of every run of 256 consecutive values"""
    x = np.asarray(x, np.float64)
    t = (len(x) + TILE - 1) // TILE
    a = np.zeros(t * TILE, np.float64)
    a[:len(x)] = x
    return B_rows(a.reshape(t, TILE))


def R(x):
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.float64(0.0)
    x = level(x)
    while len(x) > 1:
        x = level(x)
    return np.float64(x[0]) + np.float64(0.0)


def leaf_output(lam, w, members, mart=False):
    """the float a leaf stores: members = the leaf's sample indices in ascending order"""
    members = np.asarray(members, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s1 = F32(R(np.asarray(lam, np.float64)[members]))
        if mart:
            return F32(s1 / F32(len(members)))
        s2 = F32(R(np.asarray(w, np.float64)[members]))
        return F32(0) if s2 == 0 else F32(s1 / s2)


def serial_f64(x):
    """the plain left-to-right f64 sum, for contrast"""
    s = np.float64(0.0)
    for v in np.asarray(x, np.float64):
        s = s + v
    return s
