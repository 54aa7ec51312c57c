"""AdaRank (-ranker 3) on one MI355X: the weak-ranker table (init) and the wall time per round.

    python tools/ada_bench.py --shape small --metric NDCG --k 10     # ~800 lists x ~20 documents x 46 features (LETOR 4.0-like)
    python tools/ada_bench.py --shape c2 --metric MAP --k 0          # ranklib_amd.synth c2 (3.77 M x 136, 31 520 lists)

Two rl_ada_learn runs on the same data: -round 0 (upload, the weak-ranker table, the final score) and -round R with -noeq, a tolerance
of 1e300 and -max R + 1, so that exactly R rounds run (each: the candidate pass, one ranking of the ensemble, the host's log / exp and
the sample-weight upload).  per-round = (wall(R) - wall(0)) / R.  Prints one JSON line; the kernels' split comes from a
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


def run(X, lab, qoff, metric, k, rounds):
    t = N.AdaRankTrainer(n_iteration=rounds, tolerance=1e300, train_with_enqueue=False, max_sel_count=rounds + 1, metric=metric,
                         metric_k=k)
    t.set_train(X, lab, qoff)
    t0 = time.perf_counter()
    t.learn()
    wall = time.perf_counter() - t0
    tr = t.trace()
    n = int(np.sum(tr["kind"] == N.ADA_ROUND))
    ts, _ = t.scores()
    t.close()
    return wall, n, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small", help="small | c2 (or any ranklib_amd.synth.SHAPES entry)")
    ap.add_argument("--metric", default="NDCG")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=50)
    a = ap.parse_args()
    if a.shape == "small":
        X, lab, qoff = small_shape()
    else:
        n_docs, n_feat, kind, _, _ = synth.SHAPES[a.shape]
        X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    run(X[:qoff[min(8, len(qoff) - 1)]], lab[:qoff[min(8, len(qoff) - 1)]], qoff[:min(9, len(qoff))], a.metric, a.k, 1)     # warm-up
    w0, _, _ = run(X, lab, qoff, a.metric, a.k, 0)
    w1, n, ts = run(X, lab, qoff, a.metric, a.k, a.rounds)
    lens = np.diff(qoff)
    print(json.dumps(dict(shape=a.shape, n_docs=int(qoff[-1]), n_lists=int(len(lens)), n_features=int(X.shape[1]), max_list=int(lens.max()),
                          mean_list=round(float(lens.mean()), 1), metric="%s@%d" % (a.metric, a.k), init_s=round(w0, 4), rounds=n,
                          wall_s=round(w1, 4), ms_per_round=round((w1 - w0) / max(n, 1) * 1e3, 3), train_score=ts)))


if __name__ == "__main__":
    main()
