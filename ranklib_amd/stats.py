"""ciir.umass.edu.stats: BasicStats and the Fisher randomisation test the Analyzer runs.

The test's sums run on the GPU (rl_perm_test, ranklib_amd/csrc/rl_perm.inc): one lane per permutation, each lane the Java's serial f64
chain.  There is no CPU fallback.  Two things decide the bits of every sum and are restated here: the iteration order of the Java's
HashMap<String, Double> (java_hashmap_order) and the random stream (RandomPermutationTest.seed, an rlhip extension: the Java builds an
unseeded Random for every bit vector, so no two of its runs agree).
"""
import logging
import os

import numpy as np

from . import _native
from ._native import RankLibError

logger = logging.getLogger("ranklib_amd")

_TREEIFY_THRESHOLD = 8


def java_string_hash(s):
    """String.hashCode: h = 31 h + unit over the UTF-16 code units, int32 wrap (returned unsigned)"""
    h = 0
    raw = s.encode("utf-16-be", "surrogatepass")
    for i in range(0, len(raw), 2):
        h = (31 * h + ((raw[i] << 8) | raw[i + 1])) & 0xFFFFFFFF
    return h


def java_hashmap_order(keys, where=""):
    """The order in which a java.util.HashMap<String, .> (OpenJDK 8 and later) that received put(key) for every entry of `keys`, in that
    order, iterates its keySet().  hash = h ^ (h >>> 16); 16 slots and threshold 12 to start with; a put that makes size > threshold
    doubles both and splits every bin into a low and a high list that keep their relative order; a new key goes to its bin's tail; a
    key already present keeps its place; iteration runs over the slots ascending and each bin in chain order.  A bin of up to 8 nodes
    is a plain list.  The ninth node would make it a tree (or force a resize of a small table), whose order is not restated: that put
    raises RankLibError naming `where` and the bin."""
    cap, threshold, size = 16, 12, 0
    table = [[] for _ in range(cap)]
    for key in keys:
        h = java_string_hash(key)
        h ^= h >> 16
        chain = table[h & (cap - 1)]
        if any(k == key for _, k in chain):
            continue
        if len(chain) >= _TREEIFY_THRESHOLD:
            raise RankLibError("%s: id '%s' would be the ninth entry of HashMap bin %d of %d (ids %s): the Java turns the bin into a tree, "
                               "whose iteration order is not restated here" % (where or "HashMap", key, h & (cap - 1), cap,
                                                                                ", ".join("'%s'" % k for _, k in chain)))
        chain.append((h, key))
        size += 1
        if size > threshold:
            new = [[] for _ in range(2 * cap)]
            for old in table:
                for e in old:
                    new[e[0] & (2 * cap - 1)].append(e)
            table, cap, threshold = new, 2 * cap, 2 * threshold
    return [k for chain in table for _, k in chain]


class BasicStats:
    @staticmethod
    def mean(values):                 # stats/BasicStats.java:7-16
        if len(values) == 0:
            raise RankLibError("Error in BasicStats::mean(): Empty input array.")
        mean = 0.0
        for value in values:
            mean += float(value)
        return mean / len(values)


class RandomPermutationTest:
    """stats/RandomPermutationTest.java.  seed (-npseed, rlhip extension): every test() call, that is every target, draws from one
    java.util.Random(seed); permutation i takes its nextDouble draws [i D, (i + 1) D), D = n / 10 + 1.  None: a seed from os.urandom,
    logged so that the run can be repeated."""
    nPermutation = 10000
    seed = None

    @staticmethod
    def arrays(target, baseline, where=""):
        """b[], t[] of test() :24-31: filled in the iteration order of baseline.keySet(), the "all" entry included"""
        order = java_hashmap_order(list(baseline.keys()), where)
        try:
            return [float(baseline[k]) for k in order], [float(target[k]) for k in order]
        except KeyError as ex:
            raise RankLibError("RandomPermutationTest: the target has no entry for id %s (a NullPointerException in the Java)" % ex)

    @classmethod
    def run_seed(cls):
        if cls.seed is not None:
            return int(cls.seed)
        s = int.from_bytes(os.urandom(8), "little", signed=True)
        logger.info("npseed = %d", s)
        return s

    def test(self, target, baseline):                     # :23-53
        return self.test_all([target], baseline)[0]

    def test_all(self, targets, baseline, where=""):
        """test(target, baseline) of every target, one launch for all (each target's p-value is what test() alone returns)"""
        cls = RandomPermutationTest
        if not targets:
            return []
        b, ts = None, []
        for tg in targets:
            b, t = self.arrays(tg, baseline, where)
            ts.append(t)
        if len(b) == 0:
            raise RankLibError("Error in BasicStats::mean(): Empty input array.")
        np_ = int(cls.nPermutation)
        if np_ < 1:                                       # the loop does not run: 0.0 / nPermutation
            return [float("nan") if np_ == 0 else -0.0 for _ in targets]
        count, _, _ = _native.perm_test(np.asarray(b, np.float64), np.asarray(ts, np.float64).reshape(len(ts), len(b)), self.run_seed(), 0, np_)
        return [float(c) / np_ for c in count]
