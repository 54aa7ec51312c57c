"""Staged evaluation (rl_model_eval_stages) on one MI355X, on ranklib_amd/synth.py data, the two shapes of
tools/eval_bench.py:

    python tools/stages_bench.py                    # 12 000 x 136 with 100 trees, 720 000 x 136 with 1 000 trees of 31 leaves
    python tools/stages_bench.py --shapes small     # one shape

One JSON line per shape, printed and appended to --out (profiles/stages_bench.jsonl).  The rows are built once; the legs:
  (a) what exists without the entry point: per stage a truncated Model (its text cut outside the clock), predict_rows, eval_lists,
      for the stages every --every trees;
  (b) one eval_stages call for the same stages -- the tool stops unless (a) and (b) agree bit for bit;
  (c) one eval_stages call for all T stages, with rl_debug_stage_times' walk / rank split and compares = T x sum of n^2 over the lists
      per second of rank time.
--repeat rounds after one warm-up round, the legs taking turns inside every round; host clock around the calls (uploads, launches,
copies back: what a caller waits for).  Reported: the median and least - largest of every leg, and b_faster = (a)'s least is above (b)'s
largest, i.e. the gap is more than either leg's own spread.  Clocks are whatever the device runs at: nothing here reads or assumes a
frequency."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402
from ranklib_amd.learning import truncate_model_text      # noqa: E402
import tree_models as T                       # noqa: E402  (the model text is built as the tests build it)

SHAPES = {"fold": (720000, 136, 1000, 31), "small": (12000, 136, 100, 31)}


def model_text(n_features, n_trees, n_leaves):
    rng = np.random.default_rng(n_trees)
    g = T.Gen(rng, features=range(1, n_features + 1), thresholds=np.linspace(0.05, 0.95, 64).astype(np.float32))
    return T.model_text([T.random_tree(g, n_leaves) for _ in range(n_trees)], np.full(n_trees, 0.1, np.float32))


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves = SHAPES[name]
    X, lab, qoff = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    qoff = np.ascontiguousarray(qoff, np.int32)
    lens = np.diff(qoff).astype(np.int64)
    metric, k = a.metric.split("@")[0], int(a.metric.split("@")[1]) if "@" in a.metric else 0
    text = model_text(F, n_trees, n_leaves)
    some = sorted(set(range(a.every, n_trees + 1, a.every)) | {n_trees})
    every = list(range(1, n_trees + 1))
    cuts = [truncate_model_text(text, t) for t in some]
    model = N.Model(text)

    def leg_a():
        out = np.zeros((len(some), len(lens)))
        for i, cut in enumerate(cuts):
            m = N.Model(cut)
            out[i] = N.eval_lists(m.predict_rows(rows).astype(np.float64), lab, qoff, metric, k)[0]
            m.close()
        return out

    def leg_b():
        return model.eval_stages(rows, lab, qoff, metric, k, some)[0]

    split = []

    def leg_c():
        out = model.eval_stages(rows, lab, qoff, metric, k, every)[0]
        split.append(N.stage_times())
        return out

    legs = (("a", leg_a), ("b", leg_b), ("c", leg_c))
    ms = {n: [] for n, _ in legs}
    res = {}
    for r in range(a.repeat + 1):                           # round 0 warms up
        for n, fn in legs:
            t0 = time.perf_counter()
            res[n] = fn()
            if r:
                ms[n].append((time.perf_counter() - t0) * 1e3)
    if not np.array_equal(res["a"].view(np.uint64), res["b"].view(np.uint64)):
        raise SystemExit("%s: one model per stage and eval_stages differ" % name)
    if not np.array_equal(res["c"][np.array(some) - 1].view(np.uint64), res["b"].view(np.uint64)):
        raise SystemExit("%s: the stages of the all-stages call differ from the same stages asked for alone" % name)
    walk = statistics.median(w for w, _ in split[1:])
    rank = statistics.median(r for _, r in split[1:])
    compares = int((lens * lens).sum()) * n_trees
    sa, sb = spread(ms["a"]), spread(ms["b"])
    return dict(shape=name, docs=int(n_docs), lists=len(lens), longest=int(lens.max()), features=F, trees=n_trees, leaves=n_leaves, metric=a.metric,
                stages_ab=len(some), repeats=a.repeat, a_ms=sa, b_ms=sb, c_ms=spread(ms["c"]),
                a_over_b=round(sa["median"] / sb["median"], 2), b_faster=bool(sa["least"] > sb["largest"]), equal_bits=True,
                c_walk_ms=round(walk, 3), c_rank_ms=round(rank, 3), c_compares=compares,
                c_tcompares_per_s=round(compares / (rank * 1e-3) / 1e12, 3), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--metric", default="NDCG@10")
    ap.add_argument("--every", type=int, default=50, help="legs (a) and (b): a stage every so many trees")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stages_bench.jsonl"))
    a = ap.parse_args()
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
