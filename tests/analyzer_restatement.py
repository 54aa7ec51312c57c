"""Restatement of stats/RandomPermutationTest.java:23-73 and of java.util.Random (the javadoc's LCG), in two forms held equal by
tests/test_analyzer_cpu.py: a literal one (nextDouble, digit strings, element-wise copies into pb / pt, BasicStats.mean) and a
vectorised numpy one (the 10 bits of a chunk read off the state by a shift, all permutations at once, the sums still serial over j).
No JVM exists where these tests run: parity of the GPU kernel is against this file.

The one rlhip extension: one Random(seed) per test() call; permutation p takes nextDouble draws [p D, (p + 1) D), D = n / 10 + 1."""
import numpy as np

MASK = (1 << 48) - 1
A, C = 0x5DEECE66D, 0xB


class JavaRandom:
    def __init__(self, seed):
        self.state = (seed ^ A) & MASK

    def next(self, bits):
        self.state = (self.state * A + C) & MASK
        v = self.state >> (48 - bits)
        return v - (1 << 32) if v >= (1 << 31) else v          # (int) of the shifted long

    def nextDouble(self):
        hi = self.next(26) << 27
        return float(hi + self.next(27)) * 2.0 ** -53


def lcg_jump(k):
    """(A_k, C_k): k steps of the LCG as one affine map mod 2^48, by square-and-multiply"""
    ra, rc, ba, bc = 1, 0, A, C
    while k:
        if k & 1:
            ra, rc = (ba * ra) & MASK, (ba * rc + bc) & MASK
        ba, bc = (ba * ba) & MASK, (ba * bc + bc) & MASK
        k >>= 1
    return ra, rc


def random_at(seed, draws):
    """a JavaRandom(seed) that has made `draws` nextDouble calls"""
    r = JavaRandom(seed)
    a, c = lcg_jump(2 * draws)
    r.state = (a * r.state + c) & MASK
    return r


_PAD = ["", "0", "00", "000", "0000", "00000", "000000", "0000000", "00000000", "000000000"]


def random_bit_vector(r, size):                    # :60-73, on the caller's Random
    output = ""
    for _ in range(size // 10 + 1):
        x = int((1 << 10) * r.nextDouble())
        s = bin(x)[2:]                             # Integer.toBinaryString
        if len(s) == 11:
            output += s[1:]
        else:
            output += _PAD[10 - len(s)] + s
    return output


def mean(values):                                  # BasicStats.mean
    m = 0.0
    for v in values:
        m += v
    return m / len(values)


def true_diff(b, t):
    return abs(mean([float(v) for v in b]) - mean([float(v) for v in t]))


def perm_literal(b, t, seed, perm_begin, perm_count):
    """(count, trueDiff, pDiff[perm_count]) of permutations perm_begin .. perm_begin + perm_count - 1, as the Java writes the loop"""
    b, t = [float(v) for v in b], [float(v) for v in t]
    n = len(b)
    td = abs(mean(b) - mean(t))
    r = random_at(seed, perm_begin * (n // 10 + 1))
    pb, pt = [0.0] * n, [0.0] * n
    pd, count = np.zeros(perm_count, np.float64), 0
    for i in range(perm_count):
        bits = random_bit_vector(r, n)
        for j in range(n):
            if bits[j] == "0":
                pb[j] = b[j]
                pt[j] = t[j]
            else:
                pb[j] = t[j]
                pt[j] = b[j]
        pDiff = abs(mean(pb) - mean(pt))
        if pDiff >= td:
            count += 1
        pd[i] = pDiff
    return count, td, pd


def perm_bits(n, seed, perm_begin, perm_count):
    """bool [perm_count][n]: the sign vectors, ten bits per chunk read as bits 47..38 of the state after the draw's first step"""
    D = n // 10 + 1
    s = np.zeros(perm_count, np.uint64)
    cur = random_at(seed, perm_begin * D).state
    ja, jc = lcg_jump(2 * D)
    for p in range(perm_count):
        s[p] = cur
        cur = (ja * cur + jc) & MASK
    a64, c64, m64 = np.uint64(A), np.uint64(C), np.uint64(MASK)
    bits = np.zeros((perm_count, D * 10), bool)
    with np.errstate(over="ignore"):
        for c in range(D):
            s = (s * a64 + c64) & m64
            x = s >> np.uint64(38)
            s = (s * a64 + c64) & m64
            for q in range(10):
                bits[:, c * 10 + q] = ((x >> np.uint64(9 - q)) & np.uint64(1)).astype(bool)
    return bits[:, :n]


def perm_numpy(b, t, seed, perm_begin, perm_count):
    """perm_literal's results, every permutation at once (f64 adds in the same order: serial over j)"""
    b, t = np.asarray(b, np.float64), np.asarray(t, np.float64)
    n = len(b)
    bits = perm_bits(n, seed, perm_begin, perm_count)
    sb, st = np.zeros(perm_count, np.float64), np.zeros(perm_count, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            sb = sb + np.where(bits[:, j], t[j], b[j])
            st = st + np.where(bits[:, j], b[j], t[j])
        pd = np.abs(sb / np.float64(n) - st / np.float64(n))
    td = true_diff(b, t)
    return int(np.sum(pd >= td)), td, pd


def hashmap_order_closed_form(keys):
    """HashMap iteration order without simulating the table: while no bin treeifies, a bin's chain is its keys in insertion order
    (splits keep relative order, new keys go to the tail), so the order is a stable sort of the distinct keys by slot in the final table"""
    seen = list(dict.fromkeys(keys))
    cap = 16
    while len(seen) > cap * 3 // 4:
        cap *= 2

    def slot(k):
        h = 0
        u = k.encode("utf-16-be")
        for i in range(0, len(u), 2):
            h = (31 * h + (u[i] << 8 | u[i + 1])) & 0xFFFFFFFF
        return (h ^ (h >> 16)) & (cap - 1)
    return sorted(seen, key=slot)
