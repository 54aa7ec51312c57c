"""SHAP interaction values (rl_model_predict_interactions) beside exact TreeSHAP (rl_model_predict_shap) on one
MI355X, on ranklib_amd/synth.py data and tools/shap_bench.py's models:

    python tools/interact_bench.py                    # the three shapes below
    python tools/interact_bench.py --shapes small

  small      12 000 x 136 with 100 trees of 31 leaves, columns = NULL (138 slots)
  cols20     100 000 x 136 with 1 000 trees of 31 leaves, 20 requested columns (22 slots)
  all        the same rows and model with columns = NULL, on as many rows as fit in 1 GiB of result

One JSON line per shape, printed and appended to --out (profiles/interact_bench.jsonl).  The rows are built once and the covers counted
once.  Per round, in turn:
  interactions     one predict_interactions call: interact_ms is rl_debug_interact_times' device time of k_model_interact and
                   k_interact_finish over the call's chunks (the k_model_shap launches inside the call are timed apart and reported as
                   inner_shap_ms)
  shap             one predict_shap call on the same rows and columns: shap_ms is rl_debug_shap_times' device time of k_model_shap
--repeat rounds after one warm-up round; the medians and least - largest are reported, rows per second from the medians and the ratio.
f64_ops_per_row_tree counts the rounded f64 operations of the computed form on the model's path tables as DESIGN.md 27.4 counts them,
averaged over the trees: per leaf of d >= 2 elements and per conditioned element whose slot is walked, 5 per extend step ((d - 1) d / 2
steps), 7 per unwind step as the kernel runs it (d - 1 steps per attributed element in another slot) and 8 per such element behind it
(the division, the four products, the add); gops_per_s is that rate at the median, vector_f64_share its share of 39.3e12 operations a
second (78.6 TFLOP/s counts an FMA as two, and this arithmetic may fuse nothing).  The first round is checked: every row of a matrix
sums to the SHAP value of the other call and the cells to rl_model_predict_leaf_sums' value within 1e-9 of the model's sum of |W out|
(a loose sanity bound: the bit-for-bit checks are tests/test_gpu_interact.py).  Clocks are whatever the device runs at: nothing here
reads or assumes a frequency."""
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
from shap_bench import model_trees            # noqa: E402

# rows, features, trees, leaves, requested columns (None: all), bytes of result at most (None: every row)
SHAPES = {"small": (12000, 136, 100, 31, None, None), "cols20": (100000, 136, 1000, 31, 20, None), "all": (100000, 136, 1000, 31, None, 1 << 30)}
VECTOR_F64_OPS = 39.3e12


def op_count(trees, columns):
    """(f64 operations of the interaction walk per (row, tree), of the SHAP walk, mean elements per leaf, longest element list).  A pair
    whose two features share a slot is not walked: with columns given, that is every pair inside rest"""
    slot = (lambda f: f) if columns is None else (lambda f: f if f in columns else -1)
    ops, shap_ops, ds = 0, 0, []
    for t in trees:
        for _, els in SR.leaf_elements(t, np.zeros(len(t["feature"]), np.uint64), SR.f64):
            d = len(els)
            ds.append(d)
            shap_ops += 5 * d * (d + 1) // 2 + 7 * d * d + 6 * d
            if d < 2:
                continue
            slots = [slot(e[0]) for e in els]
            for c in range(d):
                others = sum(1 for e in range(d) if e != c and slots[e] != slots[c])
                if others:                                   # (a leaf whose elements all share the conditioned slot is skipped whole)
                    ops += 5 * (d - 1) * d // 2 + others * (7 * (d - 1) + 8)
    return ops / len(trees), shap_ops / len(trees), sum(ds) / len(ds), max(ds)


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves, n_cols, result_bytes = SHAPES[name]
    trees, w = model_trees(F, n_trees, n_leaves)
    model = N.Model(T.model_text(trees, w))
    feats = [int(f) for f in model.features()]
    cols = None if n_cols is None else feats[::max(1, len(feats) // n_cols)][:n_cols]
    S = (len(feats) if cols is None else len(cols)) + 2
    X, _, _ = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    model.cover(rows)                                       # the covers of all rows, whatever part of them is explained
    if result_bytes is not None:
        rows = rows[:min(n_docs, result_bytes // (8 * S * S))]
    n = len(rows)
    ops, shap_ops, mean_d, max_d = op_count(trees, None if cols is None else set(cols))
    mag = sum(abs(float(np.float64(wt)) * float(o)) for t, wt in zip(trees, w) for o, f in zip(t["output"], t["feature"]) if f == -1)
    walk, inner, shap, passes = [], [], [], 0
    for r in range(a.repeat + 1):                           # round 0 warms up
        got, ids = model.predict_interactions(rows, cols)
        (i_ms, in_ms), passes = N.interact_times(), N.interact_passes()
        phi, _ = model.predict_shap(rows, cols)
        s_ms = N.shap_times()
        print("%s round %d: interactions %.3f ms (shap inside %.3f ms), shap %.3f ms" % (name, r, i_ms, in_ms, s_ms), file=sys.stderr, flush=True)
        if r:
            walk.append(i_ms); inner.append(in_ms); shap.append(s_ms)
        else:
            gap_row = float(np.abs(got.sum(axis=2) - phi).max())
            gap_all = float(np.abs(got.sum(axis=(1, 2)) - model.leaf_sums(rows)).max())
            asym = float(np.abs(got - got.transpose(0, 2, 1)).max())
            if not max(gap_row, gap_all, asym) <= 1e-9 * mag:
                raise SystemExit("%s: row sums %g from SHAP, cells %g from the leaf sum, asymmetry %g" % (name, gap_row, gap_all, asym))
        del got, phi
    si, sn, ss = spread(walk), spread(inner), spread(shap)
    per_s = lambda ms: round(n / (ms * 1e-3) / 1e6, 5)           # noqa: E731
    rate = ops * n_trees * n / (si["median"] * 1e-3)
    return dict(shape=name, docs=int(n), features=F, trees=n_trees, leaves=n_leaves, slots=S, passes=passes, repeats=a.repeat,
                interact_ms=si, inner_shap_ms=sn, shap_ms=ss, interact_mrows_per_s=per_s(si["median"]), shap_mrows_per_s=per_s(ss["median"]),
                interact_over_shap=round(si["median"] / ss["median"], 2), mean_elements_per_leaf=round(mean_d, 2), longest_path=max_d,
                f64_ops_per_row_tree=round(ops, 1), shap_f64_ops_per_row_tree=round(shap_ops, 1), ops_over_shap_ops=round(ops / shap_ops, 2),
                gops_per_s=round(rate / 1e9, 1), vector_f64_share=round(rate / VECTOR_F64_OPS, 4), row_sum_gap=gap_row, cells_sum_gap=gap_all,
                asymmetry=asym, lib=os.path.basename(N.LIB_PATH), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,cols20,all")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interact_bench.jsonl"))
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
