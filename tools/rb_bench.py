"""RankBoost (-ranker 2) on one MI355X: init (the pair table, the take orders, the upload) and the wall time per round.

    python tools/rb_bench.py --shape small --metric NDCG --k 10     # ~800 lists x ~20 documents x 46 features (LETOR 4.0-like)
    python tools/rb_bench.py --shape c2 --rounds 3                  # ranklib_amd.synth c2 (3.77 M x 136, 31 520 lists)

First prints the number of crucial pairs P (the length of the Z_t chain) and the bytes of the pair table, counted on the host.  Then two
rl_rb_learn runs on the same data: -round 0 (init, the final score) and -round R; per-round = (wall(R) - wall(0)) / R.  A refusal of
the library (the pair table does not fit, a non-finite round) is printed and ends the run.  One JSON line per step; the kernels' split, and
with it the ns per element of the two serial chains (k_rb_zsum over P, k_rb_cand over the N documents of a feature), comes from a
`rocprofv3 --kernel-trace --stats` run of the same command.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402
from ca_bench import small_shape              # noqa: E402  (tools/ is on sys.path when run as a script)


def crucial_pairs(lab, qoff):
    """sum over the lists of the pairs with different labels: n (n - 1) / 2 less the pairs inside each label group"""
    total = 0
    for q in range(len(qoff) - 1):
        l = lab[qoff[q]:qoff[q + 1]]
        n = len(l)
        _, c = np.unique(l, return_counts=True)
        total += n * (n - 1) // 2 - int(np.sum(c.astype(np.int64) * (c - 1) // 2))
    return total


def run(X, lab, qoff, metric, k, rounds, tc):
    t = N.RankBoostTrainer(n_iteration=rounds, n_threshold=tc, metric=metric, metric_k=k)
    t.set_train(X, lab, qoff)
    t0 = time.perf_counter()
    t.learn()
    wall = time.perf_counter() - t0
    n = len(t.trace())
    ts, _ = t.scores()
    t.close()
    return wall, n, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small", help="small | c2 (or any ranklib_amd.synth.SHAPES entry)")
    ap.add_argument("--metric", default="NDCG")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--tc", type=int, default=10)
    a = ap.parse_args()
    if a.shape == "small":
        X, lab, qoff = small_shape()
    else:
        n_docs, n_feat, kind, _, _ = synth.SHAPES[a.shape]
        X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    lens = np.diff(qoff)
    P = crucial_pairs(lab, qoff)
    head = dict(shape=a.shape, n_docs=int(qoff[-1]), n_lists=int(len(lens)), n_features=int(X.shape[1]), max_list=int(lens.max()),
                mean_list=round(float(lens.mean()), 1), crucial_pairs=P, pair_table_gb=round(8 * P / 1e9, 3),
                take_orders_gb=round(4 * int(qoff[-1]) * X.shape[1] / 1e9, 3))
    print(json.dumps(head), flush=True)
    try:
        e = min(8, len(qoff) - 1)
        run(X[:qoff[e]], lab[:qoff[e]], qoff[:e + 1], a.metric, a.k, 1, a.tc)     # warm-up
        w0, _, _ = run(X, lab, qoff, a.metric, a.k, 0, a.tc)
        w1, n, ts = run(X, lab, qoff, a.metric, a.k, a.rounds, a.tc)
    except N.RankLibError as ex:
        print(json.dumps(dict(head, refused=str(ex))))
        return 1
    print(json.dumps(dict(head, metric="%s@%d" % (a.metric, a.k), tc=a.tc, init_s=round(w0, 4), rounds=n, wall_s=round(w1, 4),
                          ms_per_round=round((w1 - w0) / max(n, 1) * 1e3, 3), train_score=ts)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
