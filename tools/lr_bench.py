"""Linear Regression (-ranker 9) on one MI355X: the accumulation kernel, the host solve, scoring + ranking, and the wall time with the upload.

    python tools/lr_bench.py --shape small                # ~800 lists x ~20 documents x 46 features (LETOR 4.0-like)
    python tools/lr_bench.py --shape c2 --rb 0,1,2,4      # ranklib_amd.synth c2 (3.77 M x 136); the register blocks one after another
    python tools/lr_bench.py --shape c3                   # the Yahoo-set1 shape: 473 k x 700 sparse columns, 181 of them empty

One JSON line per run.  gram_ms is k_lr_gram between two device events; a wavefront of the kernel adds RB x RB cells per lane, so
ns_per_doc = gram_ms / N is one step of every chain it carries and ns_per_doc_cell = ns_per_doc / RB^2 is the pace per (document, cell of
a lane): the figure to hold against the 5.5 ns of a lone dependent f64 add.  solve_ms and score_ms (scoring + ranking the
training set) are host clocks; wall_s is set_train + learn, the host's column-major copy and the upload included.  --rb 0 is the
library's own choice (RLHIP_LR_RB unset).  The kernels' split comes from a `rocprofv3 --kernel-trace --stats` run of the same command.
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


def run(X, lab, qoff, metric, k, lam, rb):
    if rb:
        os.environ["RLHIP_LR_RB"] = str(rb)
    else:
        os.environ.pop("RLHIP_LR_RB", None)
    t = N.LinearRegTrainer(lambda_=lam, metric=metric, metric_k=k)
    t0 = time.perf_counter()
    t.set_train(X, lab, qoff)
    t.learn()
    wall = time.perf_counter() - t0
    tm = t.times()
    ts, _ = t.scores()
    w = t.weights()
    t.close()
    n, F, r = X.shape[0], X.shape[1], tm["register_block"]
    return dict(rb=r, gram_ms=round(tm["gram_ms"], 4), ns_per_doc=round(tm["gram_ms"] * 1e6 / n, 3),
                ns_per_doc_cell=round(tm["gram_ms"] * 1e6 / n / (r * r), 3), solve_ms=round(tm["solve_ms"], 3),
                score_ms=round(tm["score_ms"], 3), wall_s=round(wall, 4), max_abs_weight=float(np.max(np.abs(w))), train_score=ts,
                cells=F * (F + 1) // 2 + F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small", help="small | c2 | c3 (or any ranklib_amd.synth.SHAPES entry)")
    ap.add_argument("--metric", default="NDCG")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--l2", type=float, default=1E-10)
    ap.add_argument("--rb", default="0", help="comma-separated register blocks to run: 0 (the library's choice), 1, 2, 4")
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    if a.shape == "small":
        X, lab, qoff = small_shape()
    else:
        n_docs, n_feat, kind, _, _ = synth.SHAPES[a.shape]
        X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    lens = np.diff(qoff)
    head = dict(shape=a.shape, n_docs=int(qoff[-1]), n_lists=int(len(lens)), n_features=int(X.shape[1]), metric="%s@%d" % (a.metric, a.k),
                l2=a.l2)
    try:
        e = min(8, len(qoff) - 1)
        run(X[:qoff[e]], lab[:qoff[e]], qoff[:e + 1], a.metric, a.k, 0.5, 0)      # warm-up
        for rb in [int(v) for v in a.rb.split(",")]:
            for _ in range(a.repeat):
                print(json.dumps(dict(head, **run(X, lab, qoff, a.metric, a.k, a.l2, rb))), flush=True)
    except N.RankLibError as ex:
        print(json.dumps(dict(head, refused=str(ex))))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
