"""Exact TreeSHAP contributions (rl_model_predict_shap) beside the Saabas walk (rl_model_predict_contribs) on
one MI355X, on ranklib_amd/synth.py data and tools/contrib_bench.py's models:

    python tools/shap_bench.py                    # 12 000 x 136 with 100 trees, then 1 000 000 x 136 with 1 000 trees of 31 leaves
    python tools/shap_bench.py --shapes small

One JSON line per shape, printed and appended to --out (profiles/shap_bench.jsonl).  The rows are built once and the covers counted once.
Per round, in turn:
  shap             one predict_shap call on all rows for all of the model's features: shap_ms is rl_debug_shap_times' device time of
                   k_model_shap over the call's chunks
  contribs         one predict_contribs call on the same rows: walk_ms is the device time of k_model_contribs
--repeat rounds after one warm-up round; the medians and least - largest are reported, rows per second from the medians and the ratio.
f64_ops_per_row_tree counts the rounded f64 operations of the computed form on the model's path tables, averaged over the trees: per leaf
of d elements 5 per extend step (d (d + 1) / 2 steps), 7 per unwind step as the kernel runs it (both arms in one loop, d steps per
element) and 6 per element behind it (the division, the term, the add); gops_per_s is that rate at the median.  The first round is
checked: the bias slot has the bits of the Saabas call's, and every row's slots sum to rl_model_predict_leaf_sums' value within 1e-9 of
the model's sum of |W out| (a loose sanity bound: the bit-for-bit checks are tests/test_gpu_shap.py).  Clocks are whatever the device
runs at: nothing here reads or assumes a frequency."""
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
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402
import shap_restatement as SR                 # noqa: E402  (the path elements are counted as the tests build them)
import tree_models as T                       # noqa: E402

SHAPES = {"fold": (1000000, 136, 1000, 31), "small": (12000, 136, 100, 31)}


def model_trees(n_features, n_trees, n_leaves):
    """tools/contrib_bench.py's model, by the same generator calls"""
    rng = np.random.default_rng(n_trees)
    g = T.Gen(rng, features=range(1, n_features + 1), thresholds=np.linspace(0.05, 0.95, 64).astype(np.float32))
    return [T.random_tree(g, n_leaves) for _ in range(n_trees)], np.full(n_trees, 0.1, np.float32)


def op_count(trees):
    """(f64 operations per (row, tree), mean elements per leaf, longest element list)"""
    ops, ds = 0, []
    for t in trees:
        for _, els in SR.leaf_elements(t, np.zeros(len(t["feature"]), np.uint64), SR.f64):
            d = len(els)
            ds.append(d)
            ops += 5 * d * (d + 1) // 2 + 7 * d * d + 6 * d
    return ops / len(trees), sum(ds) / len(ds), max(ds)


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves = SHAPES[name]
    X, _, _ = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    trees, w = model_trees(F, n_trees, n_leaves)
    ops, mean_d, max_d = op_count(trees)
    model = N.Model(T.model_text(trees, w))
    model.cover(rows)
    assert model.shap_limits() == (max_d, SR.P_LIMIT)
    mag = sum(abs(float(np.float64(wt)) * float(o)) for t, wt in zip(trees, w) for o, f in zip(t["output"], t["feature"]) if f == -1)
    shap, walk, passes = [], [], 0
    for r in range(a.repeat + 1):                           # round 0 warms up
        got, ids = model.predict_shap(rows)
        s_ms, passes = N.shap_times(), N.shap_passes()
        saabas, _ = model.predict_contribs(rows)
        w_ms = N.contrib_times()[1]
        print("%s round %d: shap %.3f ms, contribs %.3f ms" % (name, r, s_ms, w_ms), file=sys.stderr, flush=True)
        if r:
            shap.append(s_ms); walk.append(w_ms)
        else:
            if not np.array_equal(got[:, -1].view(np.uint64), saabas[:, -1].view(np.uint64)):
                raise SystemExit("%s: the bias slots of the two calls differ" % name)
            gap = float(np.abs(got.sum(axis=1) - model.leaf_sums(rows)).max())
            if not gap <= 1e-9 * mag:
                raise SystemExit("%s: the slots of a row are %g from its leaf sum" % (name, gap))
        del got, saabas
    ss, sw = spread(shap), spread(walk)
    per_s = lambda ms: round(n_docs / (ms * 1e-3) / 1e6, 4)      # noqa: E731
    return dict(shape=name, docs=int(n_docs), features=F, trees=n_trees, leaves=n_leaves, slots=len(ids) + 2, passes=passes, repeats=a.repeat,
                shap_ms=ss, walk_ms=sw, shap_mrows_per_s=per_s(ss["median"]), walk_mrows_per_s=per_s(sw["median"]),
                shap_over_walk=round(ss["median"] / sw["median"], 1), mean_elements_per_leaf=round(mean_d, 2), longest_path=max_d,
                f64_ops_per_row_tree=round(ops, 1), gops_per_s=round(ops * n_trees * n_docs / (ss["median"] * 1e-3) / 1e9, 1),
                local_accuracy_gap=gap, lib=os.path.basename(N.LIB_PATH), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_bench.jsonl"))
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
