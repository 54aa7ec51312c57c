"""Test-time evaluation (rl_eval_lists) on one MI355X, on ranklib_amd/synth.py data:

    python tools/eval_bench.py                     # the test-fold shape (720 000 documents, 136 features, 1 000 trees of 31 leaves) and a small one
    python tools/eval_bench.py --shapes small      # one shape
    python tools/eval_bench.py --shapes none       # the length sweep only

One JSON line per measurement.
  (a) "kernel": N.eval_lists alone on the file's scores, for each metric: call_ms is the best of --repeat calls on the host clock (uploads,
      launches, copies back: what a caller waits for), kernel_ms the launches alone between device events (rl_debug_eval_times).  Beside
      them the two bounds a ranking kernel can sit on: bytes (what the launches must read and write once: scores, labels, offsets, tables,
      results) over the HBM peak (--hbm-tbs, a datasheet figure, not measured here) as hbm_floor_ms, and compares = sum of n^2 over the
      lists with the rate kernel_ms makes of them (gcompares_per_s).  Whichever of the two times is nearer to kernel_ms names the bound.
  (b) "lists": Evaluator.test with Evaluator.batch = False, list by list: the parent commit's behaviour and the yardstick.
  (c) "batch": Evaluator.test with Evaluator.batch = True.
      Both write an -idv file; the tool stops if the two differ by a byte.  The ranked lists are built in memory from the synthetic arrays
      and handed to the flow in place of the LETOR reader (the same objects for both; parsing a file is not what differs between them).
      Best of --repeat-flow runs each, after one warm-up run of the batch path.
  "sweep": one list of growing length, eval_lists (NDCG@10) against the host's stable_desc_order + scorer.score, to place
      metric.EVAL_HOST_LEN.  One block ranks one list, so inside a file's call a long list costs its kernel_ms while the other lists
      run beside it, and on the host path it costs host_ms: crossover is the first length from which host_ms stays below kernel_ms.
      (call_ms of a lone list carries the call's fixed cost, uploads and copies of about 0.15 ms, which a file pays once.)
Clocks are whatever the device runs at: nothing here assumes a frequency."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import evaluator as E        # noqa: E402
from ranklib_amd import metric as M           # noqa: E402
from ranklib_amd import synth                 # noqa: E402
from ranklib_amd.learning import DataPoint, RankList, RankerFactory, RankerType, stable_desc_order     # noqa: E402
import tree_models as T                       # noqa: E402  (the model text is built as the tests build it)

SHAPES = {"fold": (720000, 136, 1000, 31), "small": (12000, 136, 100, 31)}
METRICS = (("NDCG", 10), ("DCG", 10), ("MAP", 0), ("ERR", 10), ("P", 10), ("RR", 10), ("BEST", 10))


def best_of(n, fn):
    best = None
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def make_samples(X, lab, qoff):
    rows = np.full((X.shape[0], X.shape[1] + 1), np.nan, np.float32)       # fVals[0] is unused
    rows[:, 1:] = X
    out = []
    for q in range(len(qoff) - 1):
        out.append(RankList([DataPoint.from_parsed(float(lab[i]), str(q + 1), "", rows[i]) for i in range(qoff[q], qoff[q + 1])]))
    return out


def model_text(n_features, n_trees, n_leaves):
    rng = np.random.default_rng(n_trees)
    g = T.Gen(rng, features=range(1, n_features + 1), thresholds=np.linspace(0.05, 0.95, 64).astype(np.float32))
    return T.model_text([T.random_tree(g, n_leaves) for _ in range(n_trees)], np.full(n_trees, 0.1, np.float32))


def run_shape(name, a, tmp):
    n_docs, F, n_trees, n_leaves = SHAPES[name]
    X, lab, qoff = synth.make_dataset(n_docs, F)
    samples = make_samples(X, lab, qoff)
    lens = np.diff(qoff).astype(np.int64)
    shape = dict(shape=name, docs=int(n_docs), lists=len(samples), features=F, trees=n_trees, leaves=n_leaves, longest=int(lens.max()))
    model = os.path.join(tmp, name + ".model.txt")
    with open(model, "w", encoding="ascii") as f:
        f.write(model_text(F, n_trees, n_leaves))
    ranker = RankerFactory().loadRankerFromFile(model)
    t_score, (flat, _) = best_of(1, lambda: ranker.evalLists(samples))
    compares = int((lens * lens).sum())
    nbytes = int(n_docs * (8 + 4) + (len(samples) + 1) * 4 + len(samples) * (4 + 8 + 8) + (int(lens.max()) + 2) * 8)
    for m, k in METRICS:
        N.eval_lists(flat, lab, qoff, m, k)                                  # warm-up
        kms = []
        call_ms, _ = best_of(a.repeat, lambda: (N.eval_lists(flat, lab, qoff, m, k), kms.append(N.eval_kernel_ms())))
        kernel_ms = min(kms)
        print(json.dumps(dict(shape, what="kernel", metric="%s@%d" % (m, k), call_ms=round(call_ms, 4), kernel_ms=round(kernel_ms, 4),
                              bytes=nbytes, hbm_floor_ms=round(nbytes / (a.hbm_tbs * 1e12) * 1e3, 5), compares=compares,
                              gcompares_per_s=round(compares / (kernel_ms * 1e-3) / 1e9, 2))), flush=True)
    real = E._read_input
    E._read_input = lambda _f: samples
    try:
        idv = {}

        def flow(batch):
            E.Evaluator.batch = batch
            ev = E.Evaluator(RankerType.LAMBDAMART, a.metric, a.metric)
            path = os.path.join(tmp, "%s.%s.idv" % (name, "batch" if batch else "lists"))
            ev.test(model, "synthetic", path)
            idv[batch] = open(path, "rb").read()
        flow(True)                                                          # warm-up
        batch_ms, _ = best_of(a.repeat_flow, lambda: flow(True))
        lists_ms, _ = best_of(a.repeat_flow, lambda: flow(False))
    finally:
        E._read_input = real
        E.Evaluator.batch = True
    if idv[True] != idv[False]:
        raise SystemExit("%s: the -idv files of the batch and the list by list path differ" % name)
    print(json.dumps(dict(shape, what="flow", metric=a.metric, score_rows_ms=round(t_score, 2), lists_ms=round(lists_ms, 2),
                          batch_ms=round(batch_ms, 2), ratio=round(lists_ms / batch_ms, 2), idv_bytes=len(idv[True]), idv_equal=True)), flush=True)


def sweep(a):
    rng = np.random.default_rng(7)
    scorer = M.NDCGScorer(10)
    crossover, rows = None, []
    for n in [int(v) for v in a.sweep.split(",")]:
        sc = rng.standard_normal(n).round(2)                                # ties included
        lab = rng.integers(0, 5, n).astype(np.float32)
        rl = RankList([DataPoint.from_parsed(float(l), "1", "", np.zeros(1, np.float32)) for l in lab])
        qoff = np.array([0, n], np.int32)
        N.eval_lists(sc, lab, qoff, "NDCG", 10)
        kms = []
        call_ms, got = best_of(a.repeat, lambda: (N.eval_lists(sc, lab, qoff, "NDCG", 10), kms.append(N.eval_kernel_ms()))[0])

        def host():
            scorer.idealGains.clear()
            return scorer.score(RankList(rl, list(stable_desc_order(sc))))
        host_ms, want = best_of(a.repeat, host)
        if np.float64(got[0][0]).view(np.int64) != np.float64(want).view(np.int64):
            raise SystemExit("sweep: kernel and host disagree at length %d" % n)
        rows.append((n, min(kms), host_ms))
        print(json.dumps(dict(what="sweep", length=n, call_ms=round(call_ms, 4), kernel_ms=round(min(kms), 4), host_ms=round(host_ms, 4))), flush=True)
    for n, kernel_ms, host_ms in reversed(rows):
        if host_ms >= kernel_ms:
            break
        crossover = n
    print(json.dumps(dict(what="sweep_summary", eval_host_len=M.EVAL_HOST_LEN,
                          crossover=crossover if crossover is not None else "none up to the longest length")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--metric", default="NDCG@10", help="the flows' test metric")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--repeat-flow", type=int, default=2)
    ap.add_argument("--sweep", default="256,1024,1536,2048,3072,4096,6144,6145,8192,16384,32768,65536")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s the byte floor is taken against (MI355X datasheet: 8)")
    a = ap.parse_args()
    import logging
    logging.getLogger("ranklib_amd").setLevel(logging.WARNING)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for name in [s for s in a.shapes.split(",") if s and s != "none"]:
                run_shape(name, a, tmp)
        if a.sweep:
            sweep(a)
    except N.RankLibError as ex:
        print(json.dumps(dict(refused=str(ex))))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
