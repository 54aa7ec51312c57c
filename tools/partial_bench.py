"""Partial dependence (rl_model_predict_partial) on one MI355X, on ranklib_amd/synth.py data, the two shapes of
tools/importance_bench.py:

    python tools/partial_bench.py                    # 12 000 x 136 with 100 trees, 720 000 x 136 with 1 000 trees of 31 leaves
    python tools/partial_bench.py --shapes small     # one shape

One JSON line per shape, printed and appended to --out (profiles/partial_bench.jsonl).  All 136 columns, --grid (20) order statistics
of every column's values as its grid (partial.order_statistics).  The rows are built once; the legs:
  (a) what exists without the entry point: per cell a substituted copy of the rows (made outside the clock), predict_rows, and the two
      sums in their fixed order on the host (outside the clock too: the leg is the walk and the bus).  With --sample n (the fold shape's
      default: 20) only n cells spread over the columns are timed and the sum is SCALED to all cells by n_cells / n: a_scaled says so;
  (b) one predict_partial call for all cells, ICE not asked for -- the tool stops unless (a) and (b) agree bit for bit on the means and
      shifts of the cells (a) made, and unless a second (b) call WITH the ICE scores agrees with (a)'s scores on those cells.
--repeat rounds after one warm-up round, the legs taking turns inside every round; host clock around the calls (uploads, launches,
copies back: what a caller waits for).  Reported: the median and least - largest of every leg, and b_faster = (a)'s least is above (b)'s
largest, i.e. the gap is more than either leg's own spread.
walk_ms / reduce_ms: rl_debug_partial_times of leg (b), medians; batches: the launches' blockIdx.y in all (the base's one included), and
walk_ms_per_batch = walk_ms / batches (--batch: the RL_PARTIAL_BATCH of an A/B library selected with RLHIP_LIB).  predict_device_ms: rl_model_predict_device on the same rows resident on the device, between
two device events, median of 20 launches after 3; cells_x_predict_ms = (n_cells + 1) x that -- what a walk without the path rule would
need at the least -- and walk_over_product = walk_ms over it.  Clocks are whatever the device runs at: nothing here reads or assumes a
frequency."""
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
import tree_models as T                       # noqa: E402  (the model text is built as the tests build it)

SHAPES = {"fold": (720000, 136, 1000, 31, 20), "small": (12000, 136, 100, 31, 0)}      # the last: leg (a)'s default sample (0 = every cell)


def model_text(n_features, n_trees, n_leaves):
    rng = np.random.default_rng(n_trees)
    g = T.Gen(rng, features=range(1, n_features + 1), thresholds=np.linspace(0.05, 0.95, 64).astype(np.float32))
    return T.model_text([T.random_tree(g, n_leaves) for _ in range(n_trees)], np.full(n_trees, 0.1, np.float32))


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def count_batches(sizes, B, chunk):
    """the batches of a call, the base's included, by rl_partial_host.h's rule: up to B cells of one column, and a chunk of at most `chunk`
    cells ends where the next batch would not fit whole (a batch larger than a chunk is cut)"""
    n = 1
    used = 0
    for size in sizes:
        while size:
            want, left = min(B, size), chunk - used
            if left == 0 or (want > left and used > 0 and want <= chunk):
                used = 0
                continue
            cnt = min(want, left)
            n, size, used = n + 1, size - cnt, used + cnt
    return n


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves, sample = SHAPES[name]
    sample = a.sample if a.sample >= 0 else sample
    X, _, _ = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    model = N.Model(model_text(F, n_trees, n_leaves))
    cols = np.arange(1, F + 1, dtype=np.int32)
    grids = [P.order_statistics(rows[:, c], a.grid) for c in cols]
    off = np.concatenate([[0], np.cumsum([len(g) for g in grids])])
    n_cells = int(off[-1])
    batches = count_batches([len(g) for g in grids], a.batch, max(1, min(n_cells, 65535, ((256 << 20) - 4 * n_docs) // (4 * n_docs))))
    cells = list(range(n_cells)) if not sample or sample >= n_cells else sorted({int(v) for v in np.linspace(0, n_cells - 1, sample)})
    col_of = np.repeat(np.arange(F), [len(g) for g in grids])
    flat = np.concatenate(grids)

    def leg_a():
        out, ms = np.zeros((len(cells), n_docs), np.float32), 0.0
        for i, j in enumerate(cells):
            sub = rows.copy()
            sub[:, cols[col_of[j]]] = flat[j]
            t0 = time.perf_counter()
            out[i] = model.predict_rows(sub)
            ms += (time.perf_counter() - t0) * 1e3
        return out, ms * (n_cells / len(cells))

    split = []

    def leg_b():
        t0 = time.perf_counter()
        base, mean, shift2, _ = model.predict_partial(rows, cols, grids)
        ms = (time.perf_counter() - t0) * 1e3
        split.append(N.partial_times())
        return (base, mean[cells], shift2[cells]), ms

    legs = (("a", leg_a), ("b", leg_b))
    ms = {n: [] for n, _ in legs}
    res = {}
    for r in range(a.repeat + 1):                           # round 0 warms up
        for n, fn in legs:
            res[n], t = fn()
            if r:
                ms[n].append(t)
    base, mean, shift2 = res["b"]
    sums = [P.fixed_order_sums(s.astype(np.float64), base.astype(np.float64)) for s in res["a"]]
    want_m, want_s = np.array([s1 for s1, _ in sums]) / float(n_docs), np.array([s2 for _, s2 in sums]) / float(n_docs)
    if not (np.array_equal(want_m.view(np.uint64), mean.view(np.uint64)) and np.array_equal(want_s.view(np.uint64), shift2.view(np.uint64))):
        raise SystemExit("%s: one substituted copy per cell and predict_partial differ in a mean or a shift" % name)
    few = cells[:: max(1, len(cells) // 4)][:4]              # the ICE scores of a few of (a)'s cells, their columns in one more call
    _, _, _, ice = model.predict_partial(rows, [cols[col_of[j]] for j in few], [flat[j:j + 1] for j in few], ice=True)
    if not np.array_equal(ice.view(np.uint32), res["a"][[cells.index(j) for j in few]].view(np.uint32)):
        raise SystemExit("%s: one substituted copy per cell and predict_partial differ in a score" % name)
    walk = statistics.median(w for w, _ in split[1:])
    red = statistics.median(r for _, r in split[1:])
    dX = torch.from_numpy(rows).cuda()
    dO = torch.empty(n_docs, dtype=torch.float32, device="cuda")
    pd = []
    for i in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.predict_device(dX.data_ptr(), n_docs, F + 1, dO.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            pd.append(e0.elapsed_time(e1))
    pdm = statistics.median(pd)
    sa, sb = spread(ms["a"]), spread(ms["b"])
    return dict(shape=name, docs=int(n_docs), features=F, trees=n_trees, leaves=n_leaves, grid=a.grid, cells=n_cells, batch=a.batch,
                batches=batches, repeats=a.repeat, a_cells_timed=len(cells), a_scaled=len(cells) != n_cells, a_ms=sa, b_ms=sb,
                a_over_b=round(sa["median"] / sb["median"], 2), b_faster=bool(sa["least"] > sb["largest"]), equal_bits=True,
                walk_ms=round(walk, 3), reduce_ms=round(red, 3), walk_ms_per_batch=round(walk / batches, 3), predict_device_ms=round(pdm, 4),
                predict_path=int(model.path()), cells_x_predict_ms=round((n_cells + 1) * pdm, 3),
                walk_over_product=round(walk / ((n_cells + 1) * pdm), 3), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--grid", type=int, default=20, help="order statistics per column")
    ap.add_argument("--batch", type=int, default=N.PARTIAL_BATCH, help="RL_PARTIAL_BATCH of the library under RLHIP_LIB, where it was built with another")
    ap.add_argument("--sample", type=int, default=-1, help="leg (a): time this many cells and scale (0: every cell; default: the shape's own)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial_bench.jsonl"))
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
