"""Feature contributions (rl_model_cover / rl_model_predict_contribs) on one MI355X, on ranklib_amd/synth.py data:

    python tools/contrib_bench.py                    # 1 000 000 x 136 with 1 000 trees of 31 leaves
    python tools/contrib_bench.py --shapes small     # 12 000 x 136 with 100 trees

One JSON line per shape, printed and appended to --out (profiles/contrib_bench.jsonl).  The rows are built once.  Per round, in turn:
  cover            one cover call on all rows: cover_ms is rl_debug_contrib_times' device time of k_model_cover over the call's chunks
  contribs         one predict_contribs call on all rows for all of the model's features: walk_ms is the device time of k_model_contribs
  predict          rl_model_predict_device on the same rows resident on the device, between two device events: the yardstick
--repeat rounds after one warm-up round; the medians and least - largest are reported, rows per second from the medians, and the two
ratios to predict.  The first round's contributions are checked: every row's slots must sum to predict's score within float rounding
of the float chain (a loose sanity bound, 1e-3 relative: the bit-for-bit checks are tests/test_gpu_contribs.py).  Clocks are whatever
the device runs at: nothing here reads or assumes a frequency."""
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
import tree_models as T                       # noqa: E402  (the model text is built as the tests build it)

SHAPES = {"fold": (1000000, 136, 1000, 31), "small": (12000, 136, 100, 31)}


def model_text(n_features, n_trees, n_leaves):
    rng = np.random.default_rng(n_trees)
    g = T.Gen(rng, features=range(1, n_features + 1), thresholds=np.linspace(0.05, 0.95, 64).astype(np.float32))
    return T.model_text([T.random_tree(g, n_leaves) for _ in range(n_trees)], np.full(n_trees, 0.1, np.float32))


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def run_shape(name, a):
    n_docs, F, n_trees, n_leaves = SHAPES[name]
    X, _, _ = synth.make_dataset(n_docs, F)
    rows = np.zeros((n_docs, F + 1), np.float32)            # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    model = N.Model(model_text(F, n_trees, n_leaves))
    d_rows = torch.from_numpy(rows).cuda()
    d_out = torch.zeros(n_docs, dtype=torch.float32, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cover, walk, pred, passes = [], [], [], 0
    for r in range(a.repeat + 1):                           # round 0 warms up
        model.cover(rows)
        c_ms = N.contrib_times()[0]
        got, ids = model.predict_contribs(rows)
        w_ms, passes = N.contrib_times()[1], N.contrib_passes()
        torch.cuda.synchronize()
        start.record()
        model.predict_device(d_rows.data_ptr(), n_docs, F + 1, d_out.data_ptr())
        stop.record()
        torch.cuda.synchronize()
        if r:
            cover.append(c_ms); walk.append(w_ms); pred.append(start.elapsed_time(stop))
        else:
            score = d_out.cpu().numpy().astype(np.float64)
            total = got.sum(axis=1)
            if not np.all(np.abs(total - score) <= 1e-3 * np.maximum(1.0, np.abs(score))):
                raise SystemExit("%s: the contributions of a row do not sum to its score" % name)
            counts, _ = model.cover_of(0)
            if int(counts[0]) != n_docs or model.cover_rows() != n_docs:
                raise SystemExit("%s: the root's cover is not the number of rows" % name)
    sc, sw, sp = spread(cover), spread(walk), spread(pred)
    per_s = lambda ms: round(n_docs / (ms * 1e-3) / 1e6, 3)      # noqa: E731
    return dict(shape=name, docs=int(n_docs), features=F, trees=n_trees, leaves=n_leaves, slots=len(ids) + 2, passes=passes, repeats=a.repeat,
                cover_ms=sc, walk_ms=sw, predict_ms=sp, cover_mrows_per_s=per_s(sc["median"]), walk_mrows_per_s=per_s(sw["median"]),
                predict_mrows_per_s=per_s(sp["median"]), cover_over_predict=round(sc["median"] / sp["median"], 2),
                walk_over_predict=round(sw["median"] / sp["median"], 2), predict_path=model.path(), lib=os.path.basename(N.LIB_PATH), clocks="not read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib_bench.jsonl"))
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
