"""Leaf indices (rl_model_predict_leaves) on one MI355X, on ranklib_amd/synth.py data:

    python tools/leaves_bench.py                     # 1 000 000 x 136 with 1 000 trees of 31 leaves, both layouts
    python tools/leaves_bench.py --docs 100000       # a smaller file

One JSON line, printed and appended to --out (profiles/leaves_bench.jsonl).  The rows are built once.  Per layout --repeat calls after
one warm-up call, the layouts taking turns inside every round:
  walk_ms          rl_debug_leaves_times: the time between device events around the kernel launches of the call, summed over its chunks
                   (the upload of a chunk's rows and the copy back of its leaf numbers are outside the events); median, least, largest
  call_ms          the host clock around the whole call: uploads, launches, copies back -- what a caller waits for
  store_gb_s       2 bytes x docs x trees over the median walk_ms: the rate at which the kernel's results reach memory
predict_device_ms: rl_model_predict_device on the same rows resident on the device, between two device events, median of 20 launches
after 3: ONE scoring pass of the same walk, the yardstick; walk_over_predict = walk_ms over it.
generic: one call per layout on a handle made under RLHIP_EVAL_GENERIC (k_model_leaves), for the record.
The tool stops unless the two layouts are each other's transpose, the generic kernel agrees with the tiled one, and the leaves of the
first rows reproduce rl_model_predict_leaf_sums bit for bit.  Clocks are whatever the device runs at: nothing here reads or assumes a
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
from ranklib_amd import synth                 # noqa: E402
import tree_models as T                       # noqa: E402  (the model text is built as the tests build it)


def model_trees(n_features, n_trees, n_leaves):
    rng = np.random.default_rng(n_trees)
    g = T.Gen(rng, features=range(1, n_features + 1), thresholds=np.linspace(0.05, 0.95, 64).astype(np.float32))
    return [T.random_tree(g, n_leaves) for _ in range(n_trees)]


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def timed(model, rows, by_tree):
    t0 = time.perf_counter()
    out = model.predict_leaves(rows, by_tree=by_tree)
    return out, (time.perf_counter() - t0) * 1e3, N.leaves_times()


def run(a):
    X, _, _ = synth.make_dataset(a.docs, a.features)
    rows = np.zeros((a.docs, a.features + 1), np.float32)   # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    del X
    trees = model_trees(a.features, a.trees, a.leaves)
    text = T.model_text(trees, np.full(a.trees, 0.1, np.float32))
    model = N.Model(text)
    legs = (("by_row", False), ("by_tree", True))
    walk, call, res = {n: [] for n, _ in legs}, {n: [] for n, _ in legs}, {}
    for r in range(a.repeat + 1):                           # round 0 warms up
        for n, by_tree in legs:
            res[n], c, w = timed(model, rows, by_tree)
            if r:
                walk[n].append(w)
                call[n].append(c)
    path = int(model.path())
    step = max(1, a.docs // 4096)                           # a transposed copy of 2 GB is the host's time: every step-th document
    if not np.array_equal(res["by_row"][::step], res["by_tree"][:, ::step].T):
        raise SystemExit("the two layouts are not each other's transpose")
    few = min(a.docs, 4096)
    outs = [t["output"][t["feature"] == -1].astype(np.float64) for t in trees]
    s = np.zeros(few, np.float64)
    for k in range(a.trees):
        s = s + np.float64(np.float32(0.1)) * outs[k][res["by_row"][:few, k]]
    if not np.array_equal(s.view(np.uint64), model.leaf_sums(rows[:few]).view(np.uint64)):
        raise SystemExit("the leaves do not reproduce rl_model_predict_leaf_sums")
    generic = {}
    if a.generic:
        os.environ["RLHIP_EVAL_GENERIC"] = "1"
        gm = N.Model(text)
        del os.environ["RLHIP_EVAL_GENERIC"]
        for n, by_tree in legs:
            out, _, w = timed(gm, rows, by_tree)
            if not np.array_equal(out[::step] if not by_tree else out[:, ::step], res[n][::step] if not by_tree else res[n][:, ::step]):
                raise SystemExit("k_model_leaves and k_model_leaves_tiled differ (%s)" % n)
            generic[n + "_walk_ms"] = round(w, 3)
        generic["path"] = int(gm.path())
        del out
    del res
    dX = torch.from_numpy(rows).cuda()
    dO = torch.empty(a.docs, dtype=torch.float32, device="cuda")
    pd = []
    for i in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.predict_device(dX.data_ptr(), a.docs, a.features + 1, dO.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            pd.append(e0.elapsed_time(e1))
    pdm = statistics.median(pd)
    nbytes = 2.0 * a.docs * a.trees
    line = dict(docs=a.docs, features=a.features, trees=a.trees, leaves=a.leaves, repeats=a.repeat, path=path, out_bytes=int(nbytes),
                predict_device_ms=round(pdm, 3), predict_path=int(model.path()), generic=generic, clocks="not read")
    for n, _ in legs:
        w = spread(walk[n])
        line[n] = dict(walk_ms=w, call_ms=spread(call[n]), store_gb_s=round(nbytes / w["median"] / 1e6, 1),
                       walk_over_predict=round(w["median"] / pdm, 3))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=136)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--leaves", type=int, default=31)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--generic", type=int, default=1, help="0: leave the generic kernel's calls out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leaves_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.init()
    try:
        line = json.dumps(run(a))
    except N.RankLibError as ex:
        print(json.dumps(dict(refused=str(ex))))
        return 1
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
