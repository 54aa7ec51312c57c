"""Second-order accumulated local effects (rl_model_predict_ale2) on one MI355X, on ranklib_amd/synth.py data, the two
shapes of tools/ale_bench.py:

    python tools/ale2_bench.py                    # 12 000 x 136 with 100 trees, 720 000 x 136 with 1 000 trees of 31 leaves
    python tools/ale2_bench.py --shapes small     # one shape

One JSON line per shape, printed and appended to --out (profiles/ale2_bench.jsonl).  --pairs (16) pairs of columns spread over the file,
--intervals (10) per axis: intervals + 1 order statistics of a column's values as its edges.  The rows are built once; the legs:
  (a) what answers the same question without the entry point: per pair the four substituted copies of the rows are materialised on the
      host and scored by predict_rows, then the second differences, the cells (partial.ale_intervals) and the sums in their fixed
      order (partial.ale2_cell_sums) on the host.  a_call_ms is the four passes with their copies, a_numpy_ms the rest.  With
      --sample n (the fold shape's default: 2) only n pairs are taken and both times are SCALED to all pairs by pairs / n: a_scaled
      says so;
  (b) one predict_ale2 call for all pairs, corners and cells not asked for -- the tool stops unless (a) and (b) agree bit for bit on
      the counts and the sums of the pairs (a) made;
  (c) one plain scoring pass, predict_rows of the rows as they are.
--repeat rounds after one warm-up round, the legs taking turns inside every round; host clock around the calls (uploads, launches,
copies back: what a caller waits for).  Reported: the median and least - largest of every leg, and b_faster = (a)'s least is above (b)'s
largest.  walk_ms / reduce_ms: rl_debug_ale2_times of leg (b), medians; walk_per_batch_over_score = walk_ms / batches / (c)'s median
(the latter holds the upload of the rows, the former does not); batches: leg (b)'s blockIdx.y in all (--batch: the RL_ALE2_BATCH of an
A/B library selected with RLHIP_LIB).  Clocks are whatever the device runs at: nothing here reads or assumes a frequency."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch                                  # (its HIP runtime has to be initialised before librlhip.so's: tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import partial as P          # noqa: E402
from ranklib_amd import synth                 # noqa: E402
from partial_bench import model_text, spread  # noqa: E402  (the same model and the same summary as tools/partial_bench.py)

SHAPES = {"fold": (720000, 136, 1000, 31, 2), "small": (12000, 136, 100, 31, 0)}      # the last: leg (a)'s default sample (0 = every pair)


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves, sample = SHAPES[name]
    sample = a.sample if a.sample >= 0 else sample
    X, _, _ = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    model = N.Model(model_text(F, n_trees, n_leaves))
    z = {c: P.order_statistics(rows[:, c], a.intervals + 1) for c in range(1, F + 1)}
    cols = [c for c in z if len(z[c]) >= 2]                  # (a column of one value has no interval)
    pairs = [(cols[(7 * j) % len(cols)], cols[(7 * j + 3 + j) % len(cols)]) for j in range(a.pairs)]
    pairs = [(x, y) for x, y in pairs if x != y]
    edges = [(z[x], z[y]) for x, y in pairs]
    off = np.concatenate([[0], np.cumsum([(len(za) - 1) * (len(zb) - 1) for za, zb in edges])])
    some = list(range(len(pairs))) if not sample or sample >= len(pairs) else sorted({int(v) for v in np.linspace(0, len(pairs) - 1, sample)})
    scale = len(pairs) / len(some)
    split_b = []

    def leg_a():
        call = host = 0.0
        counts, sums = [], []
        for j in some:
            (x, y), (za, zb) = pairs[j], edges[j]
            t0 = time.perf_counter()
            k, l = P.ale_intervals(rows[:, x], za), P.ale_intervals(rows[:, y], zb)
            inside = (k > 0) & (l > 0)
            cell = np.where(inside, (k - 1) * (len(zb) - 1) + (l - 1), -1)
            t1 = time.perf_counter()
            sc = []
            for ua in (0, 1):
                for ub in (0, 1):
                    m = rows.copy()
                    m[:, x] = np.where(inside, za[np.maximum(k, 1) - 1 + ua], rows[:, x])
                    m[:, y] = np.where(inside, zb[np.maximum(l, 1) - 1 + ub], rows[:, y])
                    sc.append(model.predict_rows(m).astype(np.float64))
            t2 = time.perf_counter()
            n, s = P.ale2_cell_sums((sc[3] - sc[1]) - (sc[2] - sc[0]), cell, (len(za) - 1) * (len(zb) - 1))
            t3 = time.perf_counter()
            counts.append(n); sums.append(s)
            call += t2 - t1
            host += (t1 - t0) + (t3 - t2)
        return (np.concatenate(counts), np.concatenate(sums)), (call * 1e3 * scale, host * 1e3 * scale)

    def leg_b():
        t0 = time.perf_counter()
        count, total = model.predict_ale2(rows, pairs, edges)[:2]
        ms = (time.perf_counter() - t0) * 1e3
        split_b.append(N.ale2_times())
        at = np.concatenate([np.arange(off[j], off[j + 1]) for j in some])
        return (count[at], total[at]), (ms, 0.0)

    def leg_c():
        t0 = time.perf_counter()
        model.predict_rows(rows)
        return None, ((time.perf_counter() - t0) * 1e3, 0.0)

    legs = (("a", leg_a), ("b", leg_b), ("c", leg_c))
    ms = {n: [] for n, _ in legs}
    res = {}
    for r in range(a.repeat + 1):                           # round 0 warms up
        for n, fn in legs:
            res[n], t = fn()
            if r:
                ms[n].append(t)
    if not (np.array_equal(res["a"][0], res["b"][0]) and np.array_equal(res["a"][1].view(np.uint64), res["b"][1].view(np.uint64))):
        raise SystemExit("%s: the four predict_rows passes with the NumPy sums and predict_ale2 differ in a count or a sum" % name)
    med = lambda v: round(statistics.median(v), 3)      # noqa: E731
    sa, sb, sc_ = spread([c + h for c, h in ms["a"]]), spread([c for c, _ in ms["b"]]), spread([c for c, _ in ms["c"]])
    batches = -(-len(pairs) // a.batch)
    walk = med([w for w, _ in split_b[1:]])
    return dict(shape=name, docs=int(n_docs), features=F, trees=n_trees, leaves=n_leaves, pairs=len(pairs), intervals=a.intervals, cells=int(off[-1]),
                batch=a.batch, batches=batches, repeats=a.repeat, a_pairs_timed=len(some), a_scaled=len(some) != len(pairs),
                a_ms=sa, a_call_ms=med([c for c, _ in ms["a"]]), a_numpy_ms=med([h for _, h in ms["a"]]), b_ms=sb, score_ms=sc_,
                a_over_b=round(sa["median"] / sb["median"], 2), a_call_over_b=round(med([c for c, _ in ms["a"]]) / sb["median"], 2),
                b_faster=bool(sa["least"] > sb["largest"]), equal_bits=True, walk_ms=walk, reduce_ms=med([r for _, r in split_b[1:]]),
                walk_per_batch_over_score=round(walk / batches / sc_["median"], 3), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--intervals", type=int, default=10, help="intervals per axis")
    ap.add_argument("--batch", type=int, default=N.ALE2_BATCH, help="RL_ALE2_BATCH of the library under RLHIP_LIB, where it was built with another")
    ap.add_argument("--sample", type=int, default=-1, help="leg (a): take this many pairs and scale (0: every pair; default: the shape's own)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ale2_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.init()
    try:
        for name in [s for s in a.shapes.split(",") if s]:
            line = json.dumps(run_shape(name, a))
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    except N.RankLibError as ex:
        print(json.dumps(dict(refused=str(ex))))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
