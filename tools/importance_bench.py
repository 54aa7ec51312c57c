"""Permutation importance (rl_model_eval_permuted) on one MI355X, on ranklib_amd/synth.py data, the two shapes of
tools/stages_bench.py:

    python tools/importance_bench.py                    # 12 000 x 136 with 100 trees, 720 000 x 136 with 1 000 trees of 31 leaves
    python tools/importance_bench.py --shapes small     # one shape

One JSON line per shape, printed and appended to --out (profiles/importance_bench.jsonl).  All 136 columns, --cell-repeats (5) donor
permutations, NDCG@10.  The rows are built once; the legs:
  (a) what exists without the entry point: per cell a permuted copy of the rows (made outside the clock), predict_rows, eval_lists.  With
      --sample n (the fold shape's default: 20) only n cells spread over the columns are timed and the sum is SCALED to all cells by
      n_cells / n: a_scaled says so;
  (b) one eval_permuted call for all cells -- the tool stops unless (a) and (b) agree bit for bit on the cells (a) made.
--repeat rounds after one warm-up round, the legs taking turns inside every round; host clock around the calls (uploads, launches,
copies back: what a caller waits for).  Reported: the median and least - largest of every leg, and b_faster = (a)'s least is above (b)'s
largest, i.e. the gap is more than either leg's own spread.
walk_ms / rank_ms: rl_debug_permuted_times of leg (b), medians.  predict_device_ms: rl_model_predict_device on the same rows resident on
the device, between two device events, median of 20 launches after 3; cells_x_predict_ms = (n_cells + 1) x that -- what a walk without
the path rule would need at the least -- and walk_over_product = walk_ms over it.  Clocks are whatever the device runs at: nothing here
reads or assumes a frequency."""
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
from ranklib_amd import importance as I       # noqa: E402
from ranklib_amd import synth                 # noqa: E402
import tree_models as T                       # noqa: E402  (the model text is built as the tests build it)

SHAPES = {"fold": (720000, 136, 1000, 31, 20), "small": (12000, 136, 100, 31, 0)}      # the last: leg (a)'s default sample (0 = every cell)


def model_text(n_features, n_trees, n_leaves):
    rng = np.random.default_rng(n_trees)
    g = T.Gen(rng, features=range(1, n_features + 1), thresholds=np.linspace(0.05, 0.95, 64).astype(np.float32))
    return T.model_text([T.random_tree(g, n_leaves) for _ in range(n_trees)], np.full(n_trees, 0.1, np.float32))


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves, sample = SHAPES[name]
    sample = a.sample if a.sample >= 0 else sample
    X, lab, qoff = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    qoff = np.ascontiguousarray(qoff, np.int32)
    lens = np.diff(qoff).astype(np.int64)
    metric, k = a.metric.split("@")[0], int(a.metric.split("@")[1]) if "@" in a.metric else 0
    model = N.Model(model_text(F, n_trees, n_leaves))
    cols = np.arange(1, F + 1, dtype=np.int32)
    R = a.cell_repeats
    donor = I.donor_maps(lens, R, seed=1)
    n_cells = F * R
    cells = list(range(n_cells)) if not sample or sample >= n_cells else sorted({int(v) for v in np.linspace(0, n_cells - 1, sample)})

    def leg_a():
        out, ms = np.zeros((len(cells), len(lens))), 0.0
        for i, g in enumerate(cells):
            c, r = divmod(g, R)
            perm = rows.copy()
            perm[:, cols[c]] = rows[donor[r], cols[c]]
            t0 = time.perf_counter()
            out[i] = N.eval_lists(model.predict_rows(perm).astype(np.float64), lab, qoff, metric, k)[0]
            ms += (time.perf_counter() - t0) * 1e3
        return out, ms * (n_cells / len(cells))

    split = []

    def leg_b():
        t0 = time.perf_counter()
        base, bnan, vals, nan, _ = model.eval_permuted(rows, lab, qoff, metric, k, cols, donor)
        ms = (time.perf_counter() - t0) * 1e3
        split.append(N.permuted_times())
        if nan.any() or bnan.any():
            raise SystemExit("%s: NaN cells in synthetic data" % name)
        return vals.reshape(n_cells, len(lens))[cells], ms

    legs = (("a", leg_a), ("b", leg_b))
    ms = {n: [] for n, _ in legs}
    res = {}
    for r in range(a.repeat + 1):                           # round 0 warms up
        for n, fn in legs:
            res[n], t = fn()
            if r:
                ms[n].append(t)
    if not np.array_equal(res["a"].view(np.uint64), np.ascontiguousarray(res["b"]).view(np.uint64)):
        raise SystemExit("%s: one permuted copy per cell and eval_permuted differ" % name)
    walk = statistics.median(w for w, _ in split[1:])
    rank = statistics.median(r for _, r in split[1:])
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
    return dict(shape=name, docs=int(n_docs), lists=len(lens), longest=int(lens.max()), features=F, trees=n_trees, leaves=n_leaves, metric=a.metric,
                cells=n_cells, cell_repeats=R, batch=N.PERMUTED_BATCH, repeats=a.repeat, a_cells_timed=len(cells), a_scaled=len(cells) != n_cells,
                a_ms=sa, b_ms=sb, a_over_b=round(sa["median"] / sb["median"], 2), b_faster=bool(sa["least"] > sb["largest"]), equal_bits=True,
                walk_ms=round(walk, 3), rank_ms=round(rank, 3), predict_device_ms=round(pdm, 4), predict_path=int(model.path()),
                cells_x_predict_ms=round((n_cells + 1) * pdm, 3), walk_over_product=round(walk / ((n_cells + 1) * pdm), 3), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--metric", default="NDCG@10")
    ap.add_argument("--cell-repeats", type=int, default=5, help="donor permutations per column")
    ap.add_argument("--sample", type=int, default=-1, help="leg (a): time this many cells and scale (0: every cell; default: the shape's own)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "importance_bench.jsonl"))
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
