"""Two-feature partial dependence (rl_model_predict_partial2) on one MI355X, on ranklib_amd/synth.py data, the two shapes of
tools/partial_bench.py:

    python tools/partial2_bench.py                    # 12 000 x 136 with 100 trees, 720 000 x 136 with 1 000 trees of 31 leaves
    python tools/partial2_bench.py --shapes small     # one shape

One JSON line per shape, printed and appended to --out (profiles/partial2_bench.jsonl).  --pairs (4) pairs of the model's most-used
columns (1st with 2nd, 3rd with 4th, ...), --grid (20) order statistics per axis: 400 cells a pair.  The rows are built once; the legs:
  (a) what exists without the entry point: per cell a copy of the rows with both columns substituted (made outside the clock) and
      predict_rows.  Only --sample (8) cells spread over the pairs are timed and the sum is SCALED to all cells: a_scaled says so;
  (b) one predict_partial2 call for all cells, ICE not asked for, walk and reduce split by rl_debug_partial2_times;
  (c) the yardstick: one predict_partial call with THE SAME NUMBER OF CELLS (cells / grid columns, the most-used first, --grid values
      each) in the same session: the one-column kernel's walk per cell (rl_debug_partial_times).
The tool stops unless (a) and (b) agree bit for bit on the means and shifts of the cells (a) made, and unless a second (b) call WITH the
ICE scores, on the pairs and values of a few of (a)'s cells, agrees with (a)'s scores.  --repeat rounds after one warm-up round, the legs
taking turns inside every round; host clock around the calls; median and least - largest of every leg.  walk_per_cell_over_c is (b)'s
walk per cell over (c)'s: below 1, the rectangle descent pays.  --tile names the RL_PARTIAL2_TILE_A / _B of an A/B library selected
with RLHIP_LIB.  Clocks are whatever the device runs at: nothing here reads or assumes a frequency."""
import argparse
import collections
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch                                  # (its HIP runtime has to be initialised before librlhip.so's: tests/conftest.py)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import partial as P          # noqa: E402
from ranklib_amd import synth                 # noqa: E402
from partial_bench import SHAPES, model_text, spread      # noqa: E402


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves, _ = SHAPES[name]
    X, _, _ = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    text = model_text(F, n_trees, n_leaves)
    model = N.Model(text)
    used = [int(f) for f, _ in collections.Counter(int(f) for f in re.findall(r"<feature>\s*(\d+)\s*</feature>", text)).most_common()]
    pairs = [(used[2 * p], used[2 * p + 1]) for p in range(a.pairs)]
    grid_of = {c: P.order_statistics(rows[:, c], a.grid) for c in used}
    grids = [(grid_of[x], grid_of[y]) for x, y in pairs]
    off = np.concatenate([[0], np.cumsum([len(ga) * len(gb) for ga, gb in grids])])
    n_cells = int(off[-1])
    cells = sorted({int(v) for v in np.linspace(0, n_cells - 1, a.sample)})
    where = []                                               # (pair, u, v) of (a)'s cells
    for j in cells:
        p = int(np.searchsorted(off, j, side="right")) - 1
        where.append((p, (j - int(off[p])) // len(grids[p][1]), (j - int(off[p])) % len(grids[p][1])))
    c_cols = used[:max(1, n_cells // a.grid)]
    c_grids = [grid_of[c] for c in c_cols]
    c_cells = sum(len(g) for g in c_grids)

    def leg_a():
        out, ms = np.zeros((len(cells), n_docs), np.float32), 0.0
        for i, (p, u, v) in enumerate(where):
            sub = rows.copy()
            sub[:, pairs[p][0]] = grids[p][0][u]
            sub[:, pairs[p][1]] = grids[p][1][v]
            t0 = time.perf_counter()
            out[i] = model.predict_rows(sub)
            ms += (time.perf_counter() - t0) * 1e3
        return out, ms * (n_cells / len(cells))

    split = {"b": [], "c": []}

    def leg_b():
        t0 = time.perf_counter()
        base, mean, shift2, _ = model.predict_partial2(rows, pairs, grids)
        ms = (time.perf_counter() - t0) * 1e3
        split["b"].append(N.partial2_times())
        return (base, mean[cells], shift2[cells]), ms

    def leg_c():
        t0 = time.perf_counter()
        model.predict_partial(rows, c_cols, c_grids)
        ms = (time.perf_counter() - t0) * 1e3
        split["c"].append(N.partial_times())
        return None, ms

    legs = (("a", leg_a), ("b", leg_b), ("c", leg_c))
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
        raise SystemExit("%s: one substituted copy per cell and predict_partial2 differ in a mean or a shift" % name)
    few = list(range(0, len(cells), max(1, len(cells) // 4)))[:4]      # the ICE scores of a few of (a)'s cells: one-cell pairs in one more call
    _, _, _, ice = model.predict_partial2(rows, [pairs[where[i][0]] for i in few],
                                          [(grids[where[i][0]][0][where[i][1]:where[i][1] + 1], grids[where[i][0]][1][where[i][2]:where[i][2] + 1]) for i in few], ice=True)
    if not np.array_equal(ice.view(np.uint32), res["a"][few].view(np.uint32)):
        raise SystemExit("%s: one substituted copy per cell and predict_partial2 differ in a score" % name)
    walk, red = statistics.median(w for w, _ in split["b"][1:]), statistics.median(r for _, r in split["b"][1:])
    c_walk = statistics.median(w for w, _ in split["c"][1:])
    sa, sb, sc = spread(ms["a"]), spread(ms["b"]), spread(ms["c"])
    return dict(shape=name, docs=int(n_docs), features=F, trees=n_trees, leaves=n_leaves, pairs=pairs, grid=a.grid, cells=n_cells, tile=a.tile,
                repeats=a.repeat, a_cells_timed=len(cells), a_scaled=True, a_ms=sa, b_ms=sb, c_ms=sc, c_cells=c_cells,
                a_over_b=round(sa["median"] / sb["median"], 2), b_faster=bool(sa["least"] > sb["largest"]), equal_bits=True,
                walk_ms=round(walk, 3), reduce_ms=round(red, 3), walk_ms_per_cell=round(walk / n_cells, 4), c_walk_ms=round(c_walk, 3),
                c_walk_ms_per_cell=round(c_walk / c_cells, 4), walk_per_cell_over_c=round((walk / n_cells) / (c_walk / c_cells), 3),
                clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--grid", type=int, default=20, help="order statistics per axis")
    ap.add_argument("--tile", default="%dx%d" % (N.PARTIAL2_TILE_A, N.PARTIAL2_TILE_B), help="the tile of the library under RLHIP_LIB, where it was built with another")
    ap.add_argument("--sample", type=int, default=8, help="leg (a): time this many cells and scale")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial2_bench.jsonl"))
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
