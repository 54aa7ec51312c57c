"""Accumulated local effects (rl_model_predict_ale) on one MI355X, on ranklib_amd/synth.py data, the two shapes of
tools/partial_bench.py:

    python tools/ale_bench.py                    # 12 000 x 136 with 100 trees, 720 000 x 136 with 1 000 trees of 31 leaves
    python tools/ale_bench.py --shapes small     # one shape

One JSON line per shape, printed and appended to --out (profiles/ale_bench.jsonl).  All 136 columns, --intervals (20): intervals + 1
order statistics of every column's values as its edges (partial.order_statistics).  The rows are built once; the legs:
  (a) what answers the same question without the entry point: predict_partial with the column's K + 1 edges as its grid and the ICE
      scores asked for, then on the host every document's interval (partial.ale_intervals), its two scores picked out of the ICE
      matrix, and the sums in their fixed order (partial.ale_cell_sums).  a_call_ms is the call, a_numpy_ms the selection and the sums.
      With --sample n (the fold shape's default: 8) only n columns spread over the file are taken -- the ICE matrix of all of them
      is 4 (K + 1) n_docs bytes per column -- and both times are SCALED to all columns by columns / n: a_scaled says so;
  (b) one predict_ale call for all columns, lo / hi / interval not asked for -- the tool stops unless (a) and (b) agree bit for bit on
      the counts and the sums of the columns (a) made.
--repeat rounds after one warm-up round, the legs taking turns inside every round; host clock around the calls (uploads, launches,
copies back: what a caller waits for).  Reported: the median and least - largest of every leg, and b_faster = (a)'s least is above (b)'s
largest, i.e. the gap is more than either leg's own spread.
walk_ms / reduce_ms: rl_debug_ale_times of leg (b), medians; a_walk_ms / a_reduce_ms: rl_debug_partial_times of leg (a), scaled alike;
batches: leg (b)'s blockIdx.y in all (--batch: the RL_ALE_BATCH of an A/B library selected with RLHIP_LIB).  Clocks are whatever the
device runs at: nothing here reads or assumes a frequency."""
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

SHAPES = {"fold": (720000, 136, 1000, 31, 8), "small": (12000, 136, 100, 31, 0)}      # the last: leg (a)'s default sample (0 = every column)


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves, sample = SHAPES[name]
    sample = a.sample if a.sample >= 0 else sample
    X, _, _ = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    model = N.Model(model_text(F, n_trees, n_leaves))
    cols = np.arange(1, F + 1, dtype=np.int32)
    edges = [P.order_statistics(rows[:, c], a.intervals + 1) for c in cols]
    keep = [j for j, z in enumerate(edges) if len(z) >= 2]   # (a column of one value has no interval)
    cols, edges = cols[keep], [edges[j] for j in keep]
    off = np.concatenate([[0], np.cumsum([len(z) - 1 for z in edges])])
    some = list(range(len(cols))) if not sample or sample >= len(cols) else sorted({int(v) for v in np.linspace(0, len(cols) - 1, sample)})
    scale = len(cols) / len(some)
    split_a, split_b = [], []

    def leg_a():
        t0 = time.perf_counter()
        _, _, _, ice = model.predict_partial(rows, cols[some], [edges[j] for j in some], ice=True)
        t1 = time.perf_counter()
        split_a.append(N.partial_times())
        counts, sums, g0, doc = [], [], 0, np.arange(n_docs)
        for j in some:
            iv = P.ale_intervals(rows[:, cols[j]], edges[j])
            sc, at = ice[g0:g0 + len(edges[j])], np.maximum(iv, 1)
            n, s = P.ale_cell_sums(sc[at - 1, doc].astype(np.float64), sc[at, doc].astype(np.float64), iv, len(edges[j]) - 1)
            counts.append(n); sums.append(s)
            g0 += len(edges[j])
        t2 = time.perf_counter()
        return (np.concatenate(counts), np.concatenate(sums)), ((t1 - t0) * 1e3 * scale, (t2 - t1) * 1e3 * scale)

    def leg_b():
        t0 = time.perf_counter()
        count, total = model.predict_ale(rows, cols, edges)[:2]
        ms = (time.perf_counter() - t0) * 1e3
        split_b.append(N.ale_times())
        at = np.concatenate([np.arange(off[j], off[j + 1]) for j in some])
        return (count[at], total[at]), (ms, 0.0)

    legs = (("a", leg_a), ("b", leg_b))
    ms = {n: [] for n, _ in legs}
    res = {}
    for r in range(a.repeat + 1):                           # round 0 warms up
        for n, fn in legs:
            res[n], t = fn()
            if r:
                ms[n].append(t)
    if not (np.array_equal(res["a"][0], res["b"][0]) and np.array_equal(res["a"][1].view(np.uint64), res["b"][1].view(np.uint64))):
        raise SystemExit("%s: predict_partial with the NumPy selection and predict_ale differ in a count or a sum" % name)
    med = lambda v: round(statistics.median(v), 3)      # noqa: E731
    sa, sb = spread([c + h for c, h in ms["a"]]), spread([c for c, _ in ms["b"]])
    return dict(shape=name, docs=int(n_docs), features=int(len(cols)), trees=n_trees, leaves=n_leaves, intervals=a.intervals, cells=int(off[-1]),
                batch=a.batch, batches=-(-len(cols) // a.batch), repeats=a.repeat, a_columns_timed=len(some), a_scaled=len(some) != len(cols),
                a_ms=sa, a_call_ms=med([c for c, _ in ms["a"]]), a_numpy_ms=med([h for _, h in ms["a"]]), b_ms=sb,
                a_over_b=round(sa["median"] / sb["median"], 2), a_call_over_b=round(med([c for c, _ in ms["a"]]) / sb["median"], 2),
                b_faster=bool(sa["least"] > sb["largest"]), equal_bits=True,
                walk_ms=med([w for w, _ in split_b[1:]]), reduce_ms=med([r for _, r in split_b[1:]]),
                a_walk_ms=med([w * scale for w, _ in split_a[1:]]), a_reduce_ms=med([r * scale for _, r in split_a[1:]]), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--intervals", type=int, default=20, help="intervals per column")
    ap.add_argument("--batch", type=int, default=N.ALE_BATCH, help="RL_ALE_BATCH of the library under RLHIP_LIB, where it was built with another")
    ap.add_argument("--sample", type=int, default=-1, help="leg (a): take this many columns and scale (0: every column; default: the shape's own)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ale_bench.jsonl"))
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
