"""Interventional TreeSHAP against background rows (rl_model_predict_shap_background) beside path-dependent TreeSHAP
(rl_model_predict_shap) on one MI355X, on ranklib_amd/synth.py data and tools/shap_bench.py's models:

    python tools/interv_bench.py                  # 10 000 x 136 with 1 000 trees of 31 leaves, then 12 000 x 136 with 100 trees
    python tools/interv_bench.py --shapes small --background 100

One JSON line per shape, printed and appended to --out (profiles/interv_bench.jsonl).  The rows are built once; the background is the
first --background rows of the same generator's next rows, and the covers k_model_shap needs are counted on the documents once.  Per
round, in turn:
  interv           one predict_shap_background call on all rows for all of the model's features: mask_ms and walk_ms are
                   rl_debug_interv_times' device times of k_interv_masks + k_interv_bias and of k_model_interv
  shap             one predict_shap call on the same rows: shap_ms is the device time of k_model_shap
--repeat rounds after one warm-up round; the medians and least - largest are reported.  Counted on the model's path tables and the
first round's result: (row, z, leaf) triples -- rows x background rows x leaves, each one meet test --, and their rate at the median.
The first round is checked: every row's slots sum to rl_model_predict_leaf_sums' value within 1e-9 of the model's sum of |W out|, and
the bias is the same in every row (a loose sanity bound: the bit-for-bit checks are tests/test_gpu_interv.py).  Clocks are whatever the
device runs at: nothing here reads or assumes a frequency."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch                                  # (its HIP runtime has to be initialised before librlhip.so's: tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402
import tree_models as T                       # noqa: E402
from shap_bench import model_trees, spread    # noqa: E402

SHAPES = {"fold": (10000, 136, 1000, 31), "small": (12000, 136, 100, 31)}


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves = SHAPES[name]
    X, _, _ = synth.make_dataset(n_docs + a.background, F)
    rows = np.zeros((n_docs + a.background, F + 1), np.float32)          # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    rows, bg = rows[:n_docs], rows[n_docs:]
    trees, w = model_trees(F, n_trees, n_leaves)
    leaves = sum(int((t["feature"] == -1).sum()) for t in trees)
    model = N.Model(T.model_text(trees, w))
    model.cover(rows)
    mag = sum(abs(float(np.float64(wt)) * float(o)) for t, wt in zip(trees, w) for o, f in zip(t["output"], t["feature"]) if f == -1)
    mask, walk, shap, passes = [], [], [], 0
    for r in range(a.repeat + 1):                           # round 0 warms up
        got, ids = model.predict_shap_background(rows, bg)
        (k_ms, w_ms), passes = N.interv_times(), N.interv_passes()
        model.predict_shap(rows)
        s_ms = N.shap_times()
        print("%s round %d: masks %.3f ms, interv %.3f ms, shap %.3f ms" % (name, r, k_ms, w_ms, s_ms), file=sys.stderr, flush=True)
        if r:
            mask.append(k_ms); walk.append(w_ms); shap.append(s_ms)
        else:
            gap = float(np.abs(got.sum(axis=1) - model.leaf_sums(rows)).max())
            if not gap <= 1e-9 * mag or len(set(got[:, -1].view(np.uint64).tolist())) != 1:
                raise SystemExit("%s: the slots of a row are %g from its leaf sum, or the bias differs between rows" % (name, gap))
        del got
    sk, sw, ss = spread(mask), spread(walk), spread(shap)
    triples = n_docs * a.background * leaves
    return dict(shape=name, docs=int(n_docs), background=a.background, features=F, trees=n_trees, leaves=n_leaves, slots=len(ids) + 2,
                passes=passes, repeats=a.repeat, mask_ms=sk, walk_ms=sw, shap_ms=ss, interv_over_shap=round(sw["median"] / ss["median"], 2),
                interv_krows_per_s=round(n_docs / sw["median"], 2), row_z_leaf_triples=triples,
                gtriples_per_s=round(triples / (sw["median"] * 1e-3) / 1e9, 2), local_accuracy_gap=gap, lib=os.path.basename(N.LIB_PATH),
                clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="fold,small")
    ap.add_argument("--background", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interv_bench.jsonl"))
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
