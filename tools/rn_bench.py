"""RankNet training (-ranker 1) on one MI355X: the epoch kernel, scoring + ranking + pair counting after every epoch, and the wall time
with the upload.

    python tools/rn_bench.py --shape small                # ~800 lists x ~20 documents x 46 features (LETOR 4.0-like), hidden [10]
    python tools/rn_bench.py --shape c2 --epochs 1        # ranklib_amd.synth c2 (3.77 M x 136)
    python tools/rn_bench.py --shape c2 --skip 0,1,2,4    # k_rn_epoch whole, then without its forward pass / deltas / update
    python tools/rn_bench.py --shape small --lambdarank   # LambdaRank (-ranker 5): k_lrk_epoch, DESIGN.md 17

One JSON line per run.  epoch_ms is k_rn_epoch between two device events, per epoch; score_ms is k_rn_score + k_rn_misordered + k_ca_trials
on the training set after an epoch (a host clock around work that ends in a stream synchronisation), per epoch; wall_s is set_train +
learn, the host's column-major copy and the upload included.  floor_ms is the model of DESIGN.md 16, built from nothing but 5.5 ns per
dependent f64 add: a step with P pairs walks the delta_i chain (P adds) and then, in every round of the update a thread
takes (ceil(weights / 1024)), a sum_j chain of P adds, so an epoch cannot take less than 5.5 ns * total pairs * (1 + rounds).
ratio = epoch_ms / floor_ms.  --skip runs a variant of the kernel that leaves one phase out (RLHIP_RN_SKIP, a measuring aid: its weights
mean nothing): the difference to the whole kernel is what that phase costs.  With --lambdarank a step's pairs are every document whose
label differs, in both directions, so the model's pair count is twice total_pairs (pairs in the JSON line); --skip 2 does not exist there
(without the deltas the update would read values nobody wrote: the library runs the whole kernel).
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
from ranklib_amd.learning import RankNet      # noqa: E402
from ca_bench import small_shape              # noqa: E402  (tools/ is on sys.path when run as a script)

ADD_NS = 5.5                                  # a lone dependent f64 add


THREADS = 1024                                # k_rn_epoch's workgroup (rl_rn.inc kRnThreads)


def total_pairs(lab, qoff):
    """pairs of a list whose labels differ, summed: the sum of every step's pair count"""
    total = 0
    for q in range(len(qoff) - 1):
        _, c = np.unique(lab[qoff[q]:qoff[q + 1]], return_counts=True)
        n = int(c.sum())
        total += (n * n - int(np.sum(c.astype(np.int64) ** 2))) // 2
    return total


def n_weights(F, hidden):
    n = [F] + list(hidden) + [1]
    return sum(n[l] * (n[l - 1] + 1) for l in range(1, len(n)))


def floor_ms(pairs, nw):
    return float(ADD_NS * pairs * (1 + -(-nw // THREADS)) * 1e-6)


def run(X, lab, qoff, metric, k, epochs, lr, seed, skip, hidden, lambdarank=False):
    if skip:
        os.environ["RLHIP_RN_SKIP"] = str(skip)
    else:
        os.environ.pop("RLHIP_RN_SKIP", None)
    t = N.RankNetTrainer(n_epochs=epochs, learning_rate=lr, hidden_sizes=hidden, metric=metric, metric_k=k, lambdarank=lambdarank)
    t0 = time.perf_counter()
    t.set_train(X, lab, qoff)
    t.set_weights(np.concatenate([m.ravel() for m in RankNet.initial_weights(seed, [X.shape[1]] + list(hidden) + [1])]))
    t.learn()
    wall = time.perf_counter() - t0
    tm = t.times()
    ts, _ = t.scores()
    w = t.weights()
    tr = t.trace()
    t.close()
    pairs = (int(tr["total_pairs"][0]) if len(tr) else total_pairs(lab, qoff)) * (2 if lambdarank else 1)
    fl = floor_ms(pairs, len(w))
    per = tm["epoch_ms"] / max(1, epochs)
    return dict(ranker="LambdaRank" if lambdarank else "RankNet", skip=skip, epochs=epochs, hidden=list(hidden), n_weights=len(w), total_pairs=pairs, epoch_ms=round(per, 4),
                floor_ms=round(fl, 4), ratio=round(per / fl, 3) if fl else None, score_ms=round(tm["score_ms"] / max(1, epochs), 3),
                wall_s=round(wall, 4), max_abs_weight=float(np.max(np.abs(w))), train_score=ts,
                misordered=[int(v) for v in tr["misordered"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small", help="small | c2 | c3 (or any ranklib_amd.synth.SHAPES entry)")
    ap.add_argument("--metric", default="NDCG")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.00005)
    ap.add_argument("--hidden", default="10", help="comma-separated hidden layer sizes; empty: -layer 0")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--skip", default="0", help="comma-separated variants to run: 0 (the whole kernel), 1 (no forward pass), 2 (no deltas), 4 (no update)")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--lambdarank", action="store_true", help="train LambdaRank (k_lrk_epoch) instead of RankNet")
    a = ap.parse_args()
    if a.shape == "small":
        X, lab, qoff = small_shape()
    else:
        n_docs, n_feat, kind, _, _ = synth.SHAPES[a.shape]
        X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    lens = np.diff(qoff)
    hidden = [int(v) for v in a.hidden.split(",") if v]
    head = dict(shape=a.shape, n_docs=int(qoff[-1]), n_lists=int(len(lens)), n_features=int(X.shape[1]), max_list=int(lens.max()),
                metric="%s@%d" % (a.metric, a.k), lr=a.lr)
    try:
        e = min(8, len(qoff) - 1)
        run(X[:qoff[e]], lab[:qoff[e]], qoff[:e + 1], a.metric, a.k, 1, a.lr, a.seed, 0, hidden, a.lambdarank)      # warm-up
        for skip in [int(v) for v in a.skip.split(",")]:
            for _ in range(a.repeat):
                print(json.dumps(dict(head, **run(X, lab, qoff, a.metric, a.k, a.epochs, a.lr, a.seed, skip, hidden, a.lambdarank))), flush=True)
    except N.RankLibError as ex:
        print(json.dumps(dict(head, refused=str(ex))))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
