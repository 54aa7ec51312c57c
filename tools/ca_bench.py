"""Coordinate Ascent (-ranker 4) throughput on one MI355X: trials per second and microseconds per search direction.

    python tools/ca_bench.py --shape small            # ~800 lists x ~20 documents x 46 features (LETOR 4.0-like), the default run -r 5 -i 25
    python tools/ca_bench.py --shape c2 --one-pass    # ranklib_amd.synth c2 (3.77 M x 136, MSLR-like lists), one pass of -r 1

One trial is one `scorer.score(rank(samples))` of CoorAscent.learn (a score update, a stable sort of every list and the metric);
a direction is the nMaxIteration trials of one (feature, sign), evaluated in one pass on the GPU (ranklib_amd/csrc/rl_ca.hip).
The wall time covers rl_ca_learn only (upload, every restart, the final scores), host decisions and transfers included.
Prints one JSON line per run.
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


def small_shape(n_lists=800, n_features=46, seed=7):
    rng = np.random.default_rng(seed)
    n = rng.integers(5, 36, n_lists)
    qoff = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    X = synth.features(int(qoff[-1]), n_features, 0, synth.SEED_DATA + seed)
    lab, _ = synth.labels_from(X, 0, synth.SEED_LABEL + seed, cuts=None)
    lab = np.minimum(lab, 2).astype(np.float32)  # LETOR 4.0 grades 0..2
    return X, lab, qoff


def run(X, lab, qoff, metric, k, restarts, iters, tolerance):
    t = N.CoorAscentTrainer(n_restart=restarts, n_max_iteration=iters, tolerance=tolerance, metric=metric, metric_k=k, seed=1)
    t.set_train(X, lab, qoff)
    t0 = time.perf_counter()
    t.learn()
    wall = time.perf_counter() - t0
    tr = t.trace()
    trials = int(np.sum(tr["kind"] == N.CA_TRIAL))
    directions = int(np.sum((tr["kind"] == N.CA_TRIAL) & (tr["j"] == 0)))
    passes = int(np.sum(tr["kind"] == N.CA_PASS))
    ts, _ = t.scores()
    t.close()
    return dict(wall_s=round(wall, 4), trials=trials, directions=directions, passes=passes, trials_per_s=round(trials / wall, 1),
                us_per_direction=round(wall / max(directions, 1) * 1e6, 1), us_per_trial=round(wall / max(trials, 1) * 1e6, 2),
                train_score=ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small", help="small | c2 (or any ranklib_amd.synth.SHAPES entry)")
    ap.add_argument("--metric", default="NDCG")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("-r", "--restarts", type=int, default=None, help="default: 5 (small) / 1 (others)")
    ap.add_argument("-i", "--iters", type=int, default=25)
    ap.add_argument("--one-pass", action="store_true", help="stop every restart after its first pass over the features (tolerance = inf)")
    a = ap.parse_args()
    if a.shape == "small":
        X, lab, qoff = small_shape()
    else:
        n_docs, n_feat, kind, _, _ = synth.SHAPES[a.shape]
        X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    restarts = a.restarts if a.restarts is not None else (5 if a.shape == "small" else 1)
    res = run(X, lab, qoff, a.metric, a.k, restarts, a.iters, float("inf") if a.one_pass else 0.001)
    lens = np.diff(qoff)
    res.update(shape=a.shape, n_docs=int(qoff[-1]), n_lists=int(len(lens)), n_features=int(X.shape[1]), max_list=int(lens.max()),
               mean_list=round(float(lens.mean()), 1), metric="%s@%d" % (a.metric, a.k), restarts=restarts, iters=a.iters, one_pass=a.one_pass)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
