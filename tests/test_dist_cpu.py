"""CPU (gloo, world_size 2) coverage of the multi-rank host logic: query sharding, the torch host transport that
plugs into rl_dist_init_callback, and the int64-limb representation that makes the histogram all-reduce exact."""
import os
import random
import subprocess
import sys

import numpy as np

from ranklib_amd import dist as D
from ranklib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_is_contiguous_balanced_and_complete():
    _, _, qoff = synth.make_dataset(50000, 2, "mslr")
    for R in (1, 2, 3, 8):
        parts = D.partition_queries(qoff, R)
        assert parts[0][0] == 0 and parts[-1][1] == len(qoff) - 1
        assert all(parts[i][1] == parts[i + 1][0] for i in range(R - 1))
        sizes = [int(qoff[e] - qoff[b]) for b, e in parts]
        assert min(sizes) > 0 and max(sizes) - min(sizes) < 2 * 1251
    X = np.arange(20, dtype=np.float32).reshape(10, 2)
    lab = np.arange(10, dtype=np.float32)
    q = np.array([0, 3, 4, 8, 10], np.int32)
    got = [D.shard(X, lab, q, r, 2) for r in range(2)]
    assert np.array_equal(np.concatenate([g[0] for g in got]), X)
    assert list(got[0][2]) == [0, 3, 4, 8] and list(got[1][2]) == [0, 2]


def test_limbs_are_exact():
    rnd = random.Random(5)
    for _ in range(2000):
        v = rnd.randrange(-(1 << 100), 1 << 100)
        a, b = D.to_limbs(v)
        assert 0 <= b < (1 << 44) and -(1 << 63) <= a < (1 << 63)
        assert D.from_limbs(a, b) == v


WORKER = r'''
import os, sys, random
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from ranklib_amd import dist as D
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
tr = D.TorchHostTransport()
# 1. exact histogram exchange: every rank holds 128-bit partial totals; limbs are summed as plain int64
rnd = random.Random(100 + rank)
mine = [rnd.randrange(-(1 << 75), 1 << 75) for _ in range(500)]
limbs = np.array([x for v in mine for x in D.to_limbs(v)], dtype=np.int64)
tr.allreduce(limbs, tr.SUM)
total = [D.from_limbs(limbs[2 * i], limbs[2 * i + 1]) for i in range(500)]
ref = [sum(random.Random(100 + r).randrange(-(1 << 75), 1 << 75) for _ in range(1)) for r in range(world)]
allv = [[random.Random(100 + r).randrange(-(1 << 75), 1 << 75) for _ in range(500)] for r in range(world)]
for r in range(world):
    rr = random.Random(100 + r); allv[r] = [rr.randrange(-(1 << 75), 1 << 75) for _ in range(500)]
assert total == [sum(allv[r][i] for r in range(world)) for i in range(500)]
# 2. unsigned keys: order-preserving max / min (float keys are >= 2^31 for positive floats)
k = np.array([0x80000001 + rank, 0x3fffffff - rank, 0xfffffff0 + rank], dtype=np.uint32)
kmax = k.copy(); tr.allreduce(kmax, tr.MAX)
kmin = k.copy(); tr.allreduce(kmin, tr.MIN)
assert list(kmax) == [0x80000001 + world - 1, 0x3fffffff, 0xfffffff0 + world - 1]
assert list(kmin) == [0x80000001, 0x3fffffff - (world - 1), 0xfffffff0]
m = np.array([np.float64(1.5 + rank).view(np.uint64)], dtype=np.uint64); tr.allreduce(m, tr.MAX)
assert m.view(np.float64)[0] == 1.5 + world - 1
# 3. all-gather keeps rank order
g = tr.allgather(np.full(5, rank, np.uint8))
assert list(g) == [r for r in range(world) for _ in range(5)]
# 4. the leaf-owner exchange (ranklib_amd/dist.py leaf_exchange_plan = what rl_chain_host.inc enqueue_leaf_chains_owner does per round): documents of a global data set
#    live on the ranks in contiguous ascending ranges; every leaf's values must reach its owner in global document order
rg = np.random.RandomState(7)
Ndoc, L = 5000, 9
leaf_of = rg.randint(0, L - 2, Ndoc)                 # two leaf slots stay empty
val = rg.rand(Ndoc, 2)                                # (lambda, weight) per document
cut = [0] + sorted(rg.choice(np.arange(1, Ndoc), world - 1, replace=False).tolist()) + [Ndoc]
lens = [[int(np.sum(leaf_of[cut[r]:cut[r + 1]] == l)) for l in range(L)] for r in range(world)]
own, send, recv = D.leaf_exchange_plan(lens, rank)
loads = [sum(sum(lens[r][l] for r in range(world)) for l in range(L) if own[l] == o) for o in range(world)]
big = max(sum(lens[r][l] for r in range(world)) for l in range(L))
assert max(loads) <= max(big, -(-Ndoc // world) + big), (loads, big)          # LPT bound: no worse than the mean plus the largest leaf
mine = np.arange(cut[rank], cut[rank + 1])
def block(l):                                         # this rank's block of leaf l: lambda segment, then weight segment
    d = mine[leaf_of[mine] == l]
    return np.concatenate([val[d, 0], val[d, 1]])
sbuf = [np.concatenate([block(l) for l, n in send[d]] + [np.zeros(0)]).view(np.uint8) for d in range(world)]
got = tr.alltoallv(sbuf, [16 * sum(n for _, n in recv[r]) for r in range(world)])
for l in range(L):
    if own[l] != rank:
        continue
    lam, w = [], []
    for r in range(world):
        buf = got[r].view(np.float64); off = 0
        for l2, n in recv[r]:
            if l2 == l:
                lam.append(buf[off:off + n]); w.append(buf[off + n:off + 2 * n])
            off += 2 * n
    d = np.nonzero(leaf_of == l)[0]                   # global document order inside the leaf
    assert np.array_equal(np.concatenate(lam), val[d, 0]) and np.array_equal(np.concatenate(w), val[d, 1])
recv_bytes = sum(len(got[r]) for r in range(world) if r != rank)
assert recv_bytes <= 16 * max(loads)                  # never the 16 * Ndoc * (world - 1) / world an all-gather of every document would deliver ... unless one leaf is that big
dist.barrier()
sys.stdout.write("ok%d\n" % rank); sys.stdout.flush()
'''


import pytest


@pytest.mark.parametrize("world", [2, 3])
def test_host_transport_over_gloo(world, tmp_path):
    script = tmp_path / "w.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(29505 + world), str(script), ROOT]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert all(("ok%d" % k) in r.stdout for k in range(world))


@pytest.fixture(scope="module")
def shapes():
    import dist_shapes
    return {name: dist_shapes.make(name) for name in dist_shapes.SHAPES}


def test_shards_of_every_named_shape_concatenate_to_the_unsharded_arrays(shapes):
    """tests/dist_shapes.py: what the ranks of tests/dist_worker.py train on, put together again, is what the oracle of
    tests/test_gpu_dist_shapes.py trains on -- and a second call builds the same arrays (parent and workers build them separately)"""
    import dist_shapes
    for name, (X, lab, qoff) in shapes.items():
        s = dist_shapes.SHAPES[name]
        assert X.dtype == np.float32 and lab.dtype == np.float32 and qoff.dtype == np.int32 and X.shape == (int(qoff[-1]), s.feat), name
        assert s.docs in (0, X.shape[0]) and qoff[0] == 0 and (np.diff(qoff) > 0).all(), name
        assert not np.isnan(X).any(), name
        for world in (2, 3):
            parts = [D.shard(X, lab, qoff, r, world) for r in range(world)]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), X), (name, world)
            assert np.array_equal(np.concatenate([p[1] for p in parts]), lab), (name, world)
            assert all(p[2][0] == 0 and p[2][-1] == len(p[0]) for p in parts), (name, world)
            assert np.array_equal(np.concatenate([np.diff(p[2]) for p in parts]), np.diff(qoff)), (name, world)
    X2, lab2, qoff2 = dist_shapes.make("split_decision")
    X, lab, qoff = shapes["split_decision"]
    assert np.array_equal(X2, X) and np.array_equal(lab2, lab) and np.array_equal(qoff2, qoff)


def test_named_shapes_are_what_they_claim(shapes):
    """the statistics that rl_init thresholds, in numpy: share of cells outside a column's most frequent value (compact rows: at most 5 cells a row
    of a 16-column group), share of such cells followed by an equal value (k_run_stats: a column comes in runs at 0.9)"""
    import dist_shapes as S
    out, eq = S.share_outside_mode, S.share_equal_neighbours
    # sparse: about a quarter of the columns all zero, the others behind the first 20 are ~85 % zeros
    X, _, _ = shapes["sparse"]
    dead = [f for f in range(X.shape[1]) if not X[:, f].any()]
    assert 0.15 * X.shape[1] <= len(dead) <= 0.35 * X.shape[1] and min(dead) >= 20, dead
    assert all(0.8 <= float((X[:, f] == 0).mean()) <= 0.9 for f in range(20, X.shape[1]) if f not in dead)
    # runs: five query-level columns, two duplicated ones
    X, _, qoff = shapes["runs"]
    assert all(eq(X[:, f]) >= 0.9 for f in S.QLEVEL_COLS) and np.array_equal(X[:, 18], X[:, 2])
    # split_decision: the halves of world = 2 differ in both statistics, on the columns built for it and on no other
    X, _, qoff = shapes["split_decision"]
    q, h = S.half(qoff)
    assert D.shard(X, X[:, 0], qoff, 0, 2)[0].shape[0] == h and 0.4 * len(X) < h < 0.6 * len(X)
    for f in S.QLEVEL_COLS:
        assert eq(X[:h, f]) >= 0.95 and eq(X[h:, f]) <= 0.1, (f, eq(X[:h, f]), eq(X[h:, f]))
    for f in S.SPARSE_BLOCK:
        assert out(X[:h, f]) <= 0.2 and out(X[h:, f]) >= 0.95, (f, out(X[:h, f]), out(X[h:, f]))
    others = [f for f in range(X.shape[1]) if f not in S.QLEVEL_COLS and f not in S.SPARSE_BLOCK]
    assert all(eq(X[:h, f]) < 0.9 and eq(X[h:, f]) < 0.9 for f in others)
    # (the first rank's rows of the sparse block average under 5 cells outside the mode a group, the second rank's all 16)
    blk = X[:, list(S.SPARSE_BLOCK)]
    assert (blk[:h] != 0).sum() <= 5.0 * h * 2 and (blk[h:] != 0).sum() >= 15.0 * (len(X) - h) * 2
    # split_crows: no column in runs; per 16-column group the first half has more than 5 cells a row outside the mode bins, the second far fewer,
    # and the whole file fewer than 5 -- the all-reduced look allows the compact rows, the per-rank verdict differs
    X, _, qoff = shapes["split_crows"]
    _, h = S.half(qoff)
    assert all(eq(X[:, f]) < 0.5 and abs(out(X[:, f]) - float((X[:, f] != 0).mean())) < 1e-9 for f in range(X.shape[1]))      # (every column's mode is zero)
    per_group = lambda A: (A != 0).reshape(len(A), -1, 16).sum(2)
    assert per_group(X[:h]).mean(0).min() > 6.0 and per_group(X[h:]).mean(0).max() < 2.0 and per_group(X).mean() < 5.0
    assert (per_group(X[h:]) > 8).mean() < 0.01
    # dead_here
    X, _, qoff = shapes["dead_here"]
    _, h = S.half(qoff)
    for f in S.DEAD_HALF_COLS:
        assert len(np.unique(X[:h, f])) == 1 and len(np.unique(X[h:, f])) > 16, f
    assert len(np.unique(X[:, S.DEAD_COL])) == 1
    v, cnt = np.unique(X[:, S.MODE_ABSENT_COL], return_counts=True)
    assert v[np.argmax(cnt)] == S.MODE_VALUE and not (X[:h, S.MODE_ABSENT_COL] == S.MODE_VALUE).any() and len(np.unique(X[:h, S.MODE_ABSENT_COL])) > 4
    # wide tables: more distinct values than -tc
    for name in ("wide_table", "wide_table_tie_off"):
        X, _, _ = shapes[name]
        assert sum(len(np.unique(X[:, f])) > S.SHAPES[name].tc for f in range(X.shape[1])) >= 2, name
    assert S.SHAPES["wide_table"].tc + 1 > 264 and 16 * (S.SHAPES["wide_table"].tc + 1) * 4 <= 60 * 1024 < 16 * (S.SHAPES["wide_table_tie_off"].tc + 1) * 4
    assert S.SHAPES["deep"].leaves > 256 and shapes["wide"][0].shape[1] == 3000
    # one_long_list: rank 0 holds the long list alone; every other rank has less than a partition tile, one of three less than a chunk
    for name in ("one_long_list", "one_long_list_map"):
        X, lab, qoff = shapes[name]
        assert qoff[1] == S.LONG_LIST > 5000 and len(qoff) == 62 and 8 <= np.diff(qoff)[1:].min() and np.diff(qoff)[1:].max() <= 12
        for world in (2, 3):
            sizes = [D.shard(X, lab, qoff, r, world)[0].shape[0] for r in range(world)]
            assert sizes[0] == S.LONG_LIST and max(sizes[1:]) < 2048, sizes
        assert min(sizes) < 256, sizes
    # inf_and_wrapped
    X, lab, _ = shapes["inf_and_wrapped"]
    assert sorted(f for f in range(X.shape[1]) if np.isinf(X[:, f]).any()) == [0, 3]
    assert all((X[:, f] == np.inf).any() and (X[:, f] == -np.inf).any() for f in (0, 3)) and lab.max() == 34 and (lab > 30).sum() > 100


def test_leaf_owners_are_balanced_and_rank_invariant():
    rg = np.random.RandomState(3)
    for R in (1, 2, 3, 8):
        for _ in range(50):
            glen = (rg.pareto(1.2, 31) * 1000).astype(np.int64)
            glen[rg.randint(0, 31, 4)] = 0
            own = D.leaf_owners(glen, R)
            assert own == D.leaf_owners(list(glen), R) and all(0 <= o < R for o in own)
            load = [int(sum(glen[l] for l in range(31) if own[l] == o)) for o in range(R)]
            assert max(load) <= max(int(glen.max()), -(-int(glen.sum()) // R) + int(glen.max()))
