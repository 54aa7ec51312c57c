"""ListNet training (-ranker 7) on one MI355X: the epoch kernel, scoring + ranking after every epoch, and the wall time with the upload.

    python tools/ln_bench.py --shape small                # ~800 lists x ~20 documents x 46 features (LETOR 4.0-like)
    python tools/ln_bench.py --shape c2 --epochs 3        # ranklib_amd.synth c2 (3.77 M x 136)
    python tools/ln_bench.py --shape c2 --skip 0,1,2,4    # k_ln_epoch whole, then without its forward pass / sum chain / update

One JSON line per run.  epoch_ms is k_ln_epoch between two device events, per epoch; score_ms is k_ln_score + k_ca_trials on the training
set after an epoch (a host clock around work that ends in a stream synchronisation), per epoch; wall_s is set_train + learn, the host's
column-major copy and the upload included.  floor_ms is the model of DESIGN.md 15: one workgroup walks the lists in order, and per list
the longest serial chains are F + 1 dependent f64 adds (the forward pass), n adds (the sum of exp(o)), and n adds (a weight's update), so
with 5.5 ns per dependent add an epoch cannot take less than 5.5 ns * sum over lists of [2 (F + 1) + 3 n] -- the issue's
form of it, which also counts the label sum this library computes once per set.  ratio = epoch_ms / floor_ms.  --skip runs a variant of
the kernel that leaves one phase out (RLHIP_LN_SKIP, a measuring aid: its weights mean nothing): the difference to the whole kernel is
what that phase costs.  The kernels' split comes from a `rocprofv3 --kernel-trace --stats` run of the same command.
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
from ranklib_amd.learning import ListNet      # noqa: E402
from ca_bench import small_shape              # noqa: E402  (tools/ is on sys.path when run as a script)

ADD_NS = 5.5                                  # a lone dependent f64 add


def floor_ms(qoff, F):
    n = np.diff(qoff).astype(np.float64)
    return float(ADD_NS * np.sum(2.0 * (F + 1) + 3.0 * n) * 1e-6)


def run(X, lab, qoff, metric, k, epochs, lr, seed, skip):
    if skip:
        os.environ["RLHIP_LN_SKIP"] = str(skip)
    else:
        os.environ.pop("RLHIP_LN_SKIP", None)
    t = N.ListNetTrainer(n_epochs=epochs, learning_rate=lr, metric=metric, metric_k=k)
    t0 = time.perf_counter()
    t.set_train(X, lab, qoff)
    t.set_weights(ListNet.initial_weights(seed, X.shape[1] + 1))
    t.learn()
    wall = time.perf_counter() - t0
    tm = t.times()
    ts, _ = t.scores()
    w = t.weights()
    t.close()
    fl = floor_ms(qoff, X.shape[1])
    per = tm["epoch_ms"] / max(1, epochs)
    return dict(skip=skip, epochs=epochs, epoch_ms=round(per, 4), floor_ms=round(fl, 4), ratio=round(per / fl, 3),
                score_ms=round(tm["score_ms"] / max(1, epochs), 3), wall_s=round(wall, 4), max_abs_weight=float(np.max(np.abs(w))),
                train_score=ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small", help="small | c2 | c3 (or any ranklib_amd.synth.SHAPES entry)")
    ap.add_argument("--metric", default="NDCG")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.00001)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--skip", default="0", help="comma-separated variants to run: 0 (the whole kernel), 1 (no forward pass), 2 (no sum chain), 4 (no update)")
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    if a.shape == "small":
        X, lab, qoff = small_shape()
    else:
        n_docs, n_feat, kind, _, _ = synth.SHAPES[a.shape]
        X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    lens = np.diff(qoff)
    head = dict(shape=a.shape, n_docs=int(qoff[-1]), n_lists=int(len(lens)), n_features=int(X.shape[1]), max_list=int(lens.max()),
                metric="%s@%d" % (a.metric, a.k), lr=a.lr)
    try:
        e = min(8, len(qoff) - 1)
        run(X[:qoff[e]], lab[:qoff[e]], qoff[:e + 1], a.metric, a.k, 1, a.lr, a.seed, 0)      # warm-up
        for skip in [int(v) for v in a.skip.split(",")]:
            for _ in range(a.repeat):
                print(json.dumps(dict(head, **run(X, lab, qoff, a.metric, a.k, a.epochs, a.lr, a.seed, skip))), flush=True)
    except N.RankLibError as ex:
        print(json.dumps(dict(head, refused=str(ex))))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
