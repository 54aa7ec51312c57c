"""Neighbours in leaf space (rl_model_predict_neighbours) on one MI355X, on ranklib_amd/synth.py data:

    python tools/near_bench.py                                   # 10 000 queries x 1 000 000 references x 136, 1 000 trees of 31 leaves, k = 10
    python tools/near_bench.py --queries 1000 --refs 100000      # a smaller pair of files

One JSON line, printed and appended to --out (profiles/near_bench.jsonl).  The rows are built once.  --repeat calls after one warm-up call:
  walk_ms, match_ms    rl_debug_neighbours_times: the time between device events around the walks of both sets and around the k_near_match
                       and k_near_merge launches, summed over the call's chunks and bands (uploads are outside the events); median, least, largest
  call_ms              the host clock around the whole call: uploads, launches, the copy back of the lists
  compares_per_s       queries x references x trees over the median match_ms
  valu_share           1.5 vector instructions a compare (xor, packed min, packed add per word of two trees) over compute units x 64 lanes
                       x --clock-mhz, the peak clock the data sheet STATES (2 400 MHz; the clock the run had is not read): the fraction of peak
  predict_device_ms    rl_model_predict_device on the reference rows resident on the device, median of 10 launches after 2: ONE scoring
                       pass, the yardstick; match_over_predict = match_ms over it
parent: the route without this entry point, timed at --parent-queries x --parent-refs where it finishes: two predict_leaves calls, then per
query a NumPy compare of its leaves with every reference's and np.lexsort((index, -shared)).  parent.scaled_s is that time times
(queries x references) / (parent queries x parent references): SCALED, not measured.  The tool stops unless the GPU's lists at the
parent's size equal the parent's integers."""
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
from leaves_bench import model_trees, spread  # noqa: E402


def parent_route(model, q, r, k):
    t0 = time.perf_counter()
    lq, lr = model.predict_leaves(q), model.predict_leaves(r)
    index, shared, ar = np.zeros((len(q), k), np.int32), np.zeros((len(q), k), np.int32), np.arange(len(r))
    for i in range(len(q)):
        s = (lr == lq[i]).sum(1)
        order = np.lexsort((ar, -s))[:k]
        index[i], shared[i] = order, s[order]
    return index, shared, time.perf_counter() - t0


def run(a):
    X, _, _ = synth.make_dataset(a.refs + a.queries, a.features)
    rows = np.zeros((a.refs + a.queries, a.features + 1), np.float32)   # column 0 is unused, like DataPoint.fVals
    rows[:, 1:] = X
    del X
    ref, qry = rows[:a.refs], rows[a.refs:]
    model = N.Model(T.model_text(model_trees(a.features, a.trees, a.leaves), np.full(a.trees, 0.1, np.float32)))
    walk, match, call = [], [], []
    for r in range(a.repeat + 1):                           # round 0 warms up
        t0 = time.perf_counter()
        got = model.predict_neighbours(qry, ref, a.k)
        c = (time.perf_counter() - t0) * 1e3
        w, m = N.debug_neighbours_times()
        if r:
            walk.append(w); match.append(m); call.append(c)
    path = int(model.path())
    pq, pr = min(a.parent_queries, a.queries), min(a.parent_refs, a.refs)
    pi, ps, psec = parent_route(model, qry[:pq], ref[:pr], a.k)
    gi, gs = model.predict_neighbours(qry[:pq], ref[:pr], a.k)
    if not (np.array_equal(gi, pi) and np.array_equal(gs, ps)):
        raise SystemExit("rl_model_predict_neighbours and the parent's route differ")
    if pr == a.refs and not np.array_equal(got[0][:pq], pi):
        raise SystemExit("the full call and the parent's route differ")
    dX = torch.from_numpy(ref).cuda()
    dO = torch.empty(a.refs, dtype=torch.float32, device="cuda")
    pd = []
    for i in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.predict_device(dX.data_ptr(), a.refs, a.features + 1, dO.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            pd.append(e0.elapsed_time(e1))
    pdm = statistics.median(pd)
    prop = torch.cuda.get_device_properties(0)
    compares = float(a.queries) * a.refs * a.trees
    mm = statistics.median(match)
    rate = compares / (mm * 1e-3)
    peak = prop.multi_processor_count * 64 * a.clock_mhz * 1e6
    scaled = psec * (float(a.queries) * a.refs) / (float(pq) * pr)
    return dict(queries=a.queries, refs=a.refs, features=a.features, trees=a.trees, leaves=a.leaves, k=a.k, repeats=a.repeat, path=path,
                tiles=dict(query=N.NEAR_QUERY_TILE, ref=N.NEAR_REF_TILE, tree_chunk=N.NEAR_TREE_CHUNK, blocks=N.NEAR_BLOCKS),
                walk_ms=spread(walk), match_ms=spread(match), call_ms=spread(call), compares_per_s=float("%.4g" % rate),
                valu_share=round(1.5 * rate / peak, 3), compute_units=prop.multi_processor_count, stated_clock_mhz=a.clock_mhz,
                predict_device_ms=round(pdm, 3), match_over_predict=round(mm / pdm, 1),
                parent=dict(queries=pq, refs=pr, measured_s=round(psec, 3), scaled_s=round(scaled, 1), scaled=True,
                            scaled_over_call=round(scaled / (statistics.median(call) * 1e-3), 1), equal_integers=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--refs", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=136)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--leaves", type=int, default=31)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="the peak engine clock the data sheet states, for valu_share")
    ap.add_argument("--parent-queries", type=int, default=1000)
    ap.add_argument("--parent-refs", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_bench.jsonl"))
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
