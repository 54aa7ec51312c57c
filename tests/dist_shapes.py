"""Named data sets of the sharded tests: the parent test (tests/test_gpu_dist_shapes.py, tests/test_dist_cpu.py) and every rank of
tests/dist_worker.py (option `shape=<name>`) build the same arrays from the name alone.

Each shape selects kernels of the tree trainer that the dense `mslr` / `ns` data of tests/test_gpu_dist.py never reaches under sharding (the
one-GPU suite reaches them in tests/test_gpu_parity.py and tests/test_gpu_kernel_variants.py).  SHAPES holds what a run needs besides the arrays;
`make(name)` returns (X float32 [N, F], labels float32 [N], qoff int32 [Q + 1]) of the UNSHARDED data set.  A plain module: no pytest in here.
"""
import numpy as np

from ranklib_amd import dist as D
from ranklib_amd import synth


class Shape:
    def __init__(self, docs, feat, leaves, rounds, metric="NDCG", k=10, tc=256, tie_on=True):
        self.docs, self.feat, self.leaves, self.rounds, self.metric, self.k, self.tc, self.tie_on = docs, feat, leaves, rounds, metric, k, tc, tie_on


SHAPES = {
    # Yahoo-style columns: about a quarter all zero, the rest 85 % zeros behind 20 dense ones -> compact rows in the child passes, dense rows at the root
    "sparse": Shape(6000, 96, 12, 4),
    # set B of tests/test_gpu_kernel_variants.py: duplicated columns and five query-level columns -> the RUNS instantiations of k_hist
    "runs": Shape(12000, 24, 20, 4),
    # query-level columns and a sparse block on the first half of the lists only: the ranks of one job decide any_runs differently
    "split_decision": Shape(8000, 56, 12, 3),
    # no column in runs; the first half of the lists has 7 cells a 16-column group outside the mode bins, the second 1: the all-reduced counts allow the
    # compact rows (4 a group on average), and only the ranks of the second half build them
    "split_crows": Shape(8000, 64, 12, 3),
    # columns that are constant on one rank, constant everywhere, or whose global mode bin is empty on one rank
    "dead_here": Shape(9000, 16, 12, 4),
    # -tc 300 on columns of more than 300 distinct values: 301 bins a row, more than the compile-time LDS row stride of 264
    "wide_table": Shape(4000, 6, 10, 3, tc=300),
    # -tc 1200: tables beyond what the sharded tie-break's sort holds in LDS -- the first tied candidate is kept (rl_init.inc, init_hist_features)
    "wide_table_tie_off": Shape(4000, 6, 10, 3, tc=1200, tie_on=False),
    # 188 feature groups: the fused finish over every column (one GPU splits the finish at this width)
    "wide": Shape(4000, 3000, 15, 2),
    # 300 leaves: beyond piece mode and beyond the device plan of the leaf-owner exchange
    "deep": Shape(20000, 17, 300, 2),
    # one list of 5 600 documents, then 60 lists of 8 .. 12: one rank holds the long list alone, the others a few hundred documents or fewer
    "one_long_list": Shape(0, 12, 8, 3),
    "one_long_list_map": Shape(0, 12, 8, 2, metric="MAP", k=0),          # (two rounds: the oracle's MAP lambdas of the long list take seconds a round)
    # +-Infinity in two columns, labels up to 34 (gains wrap as Java ints do)
    "inf_and_wrapped": Shape(6000, 12, 10, 3),
}

LONG_LIST = 5600


def duplicate_columns(X):
    """two columns repeat two others (one rescaled: other thresholds, the same cuts): exact ties over several features"""
    X = X.copy()
    X[:, 18] = X[:, 2]
    X[:, 22] = 2.0 * X[:, 10] + 1.0
    return X


def query_level_columns(X, qoff, seed, lists=None):
    """five columns with one value per query (of the first `lists` lists; default all): rl_init finds their bins in runs"""
    rng = np.random.default_rng(seed)
    X = X.copy()
    nq = len(qoff) - 1
    end = int(qoff[nq if lists is None else lists])
    for j in range(5):
        vals = rng.random(nq).astype(np.float32) if j % 2 else np.floor(rng.random(nq) * 3).astype(np.float32)
        X[:end, 2 * j + 1] = np.repeat(vals, np.diff(qoff))[:end]
    return X


def half(qoff):
    """(lists, documents) of the first of two ranks: the cut D.partition_queries makes for world = 2"""
    q = D.partition_queries(qoff, 2)[0][1]
    return q, int(qoff[q])


QLEVEL_COLS = (1, 3, 5, 7, 9)
SPARSE_BLOCK = range(24, 56)


def _split_decision(s):
    X, lab, qoff = synth.make_dataset(s.docs, s.feat, "mslr", seed_offset=71)
    rng = np.random.default_rng(71)
    X = X.copy()
    for f in list(QLEVEL_COLS) + list(SPARSE_BLOCK):         # continuous and dense everywhere ...
        X[:, f] = rng.random(s.docs).astype(np.float32)
    q, h = half(qoff)
    X = query_level_columns(X, qoff, 72, lists=q)            # ... but on the first half of the lists: one value per query,
    for f in SPARSE_BLOCK:                                   # and a block of columns that are 85 % zeros
        X[:h, f][rng.random(h) < 0.85] = 0.0
    return X, lab, qoff


CROWS_ZEROS = (0.55, 0.93)          # share of zeros in every column: first half, second half of the lists


def _split_crows(s):
    X, lab, qoff = synth.make_dataset(s.docs, s.feat, "mslr", seed_offset=77)
    rng = np.random.default_rng(77)
    _, h = half(qoff)
    X = rng.random(X.shape).astype(np.float32) + np.float32(0.5)          # (only the labels and the lists of the synthetic set are kept)
    X[:, :8] += lab[:, None] * rng.random((s.docs, 8)).astype(np.float32)      # eight columns that say something about the label
    zero = rng.random(X.shape) < np.where(np.arange(s.docs) < h, CROWS_ZEROS[0], CROWS_ZEROS[1])[:, None]
    X[zero] = 0.0
    return X, lab, qoff


DEAD_HALF_COLS, DEAD_COL, MODE_ABSENT_COL, MODE_VALUE = (4, 5), 8, 12, 7.0


def _dead_here(s):
    X, lab, qoff = synth.make_dataset(s.docs, s.feat, "mslr", seed_offset=73)
    rng = np.random.default_rng(73)
    X = X.copy()
    _, h = half(qoff)
    X[:h, DEAD_HALF_COLS[0]] = 20.0                          # constant on the first half of the documents, varied on the second
    X[:h, DEAD_HALF_COLS[1]] = 0.5
    X[:, DEAD_COL] = 3.0                                     # constant everywhere
    c = X[:, MODE_ABSENT_COL]                                # small integer counts; 7 becomes the most frequent value, and only the second half has it
    c[:h][c[:h] == MODE_VALUE] = MODE_VALUE + 1.0
    c[h:][rng.random(s.docs - h) < 0.7] = MODE_VALUE
    return X, lab, qoff


def _one_long_list(s):
    rng = np.random.default_rng(74)
    sizes = np.concatenate([[LONG_LIST], rng.integers(8, 13, 60)])
    qoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(qoff[-1])
    X = rng.random((n, s.feat)).astype(np.float32)
    X[:, 0] = np.floor(X[:, 0] * 12)
    lab = np.clip(np.floor(X[:, 0] / 3 + X[:, 1] * 2 + rng.random(n)), 0, 4).astype(np.float32)
    return X, lab, qoff


def _inf_and_wrapped(s):
    X, _, qoff = synth.make_dataset(s.docs, s.feat, "mslr", seed_offset=75)
    rng = np.random.default_rng(75)
    X = X.copy()
    n = s.docs
    X[:, 0] = np.floor(rng.random(n) * 9)                    # few distinct values, +-Infinity among them
    X[rng.random(n) < 0.03, 0] = np.inf; X[rng.random(n) < 0.02, 0] = -np.inf
    X[rng.random(n) < 0.04, 3] = np.inf; X[rng.random(n) < 0.04, 3] = -np.inf       # a 256-step table: [-Inf, NaN, .., MAX_VALUE]
    lab = rng.choice(np.array([0, 1, 2, 3, 4, 30, 31, 32, 33, 34], np.float32), n)
    return X, lab, qoff


def make(name):
    s = SHAPES[name]
    if name == "sparse":
        return synth.make_dataset(s.docs, s.feat, "yahoo", seed_offset=31)
    if name == "runs":
        X, lab, qoff = synth.make_dataset(s.docs, s.feat, "mslr", seed_offset=61)
        return query_level_columns(duplicate_columns(X), qoff, 5), lab, qoff
    if name == "split_decision":
        return _split_decision(s)
    if name == "split_crows":
        return _split_crows(s)
    if name == "dead_here":
        return _dead_here(s)
    if name in ("wide_table", "wide_table_tie_off"):
        return synth.make_dataset(s.docs, s.feat, "mslr", seed_offset=76)
    if name in ("wide", "deep"):
        return synth.make_dataset(s.docs, s.feat, "mslr", seed_offset=5)
    if name in ("one_long_list", "one_long_list_map"):
        return _one_long_list(s)
    if name == "inf_and_wrapped":
        return _inf_and_wrapped(s)
    raise KeyError(name)


# ---- the statistics rl_init thresholds, restated in numpy (tests/test_dist_cpu.py: the shapes are what they claim without a GPU) -------------
def share_outside_mode(col):
    """share of a column's cells outside its most frequent value"""
    _, cnt = np.unique(col, return_counts=True)
    return 1.0 - cnt.max() / len(col)


def share_equal_neighbours(col):
    """share of the cells outside the most frequent value that are followed by an equal value (k_run_stats: a column comes in runs at 0.9)"""
    v, cnt = np.unique(col, return_counts=True)
    out = col[:-1] != v[np.argmax(cnt)]
    return float((col[:-1][out] == col[1:][out]).mean()) if out.any() else 0.0
