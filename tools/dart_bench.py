"""DART (rl_set_dart) on one MI355X, on ranklib_amd/synth.py data, at the bench shapes c1 and c2 (1 000 trees of 31 leaves),
rate_drop 0.1, max_drop 50 and unlimited:

    python tools/dart_bench.py [--shapes c1,c2] [--parent-lib build_ab/librlhip_parent.so]

One JSON line per shape, printed and appended to --out (profiles/dart_bench.jsonl).  Per shape:
  plain        rl_boost_rounds_async + rl_sync of all rounds, host clock, rounds/s -- this tree's library with DART off; with --parent-lib also
               the parent commit's library in a child process of this tool (RLHIP_LIB), the two taking turns --repeat times: DART off must
               cost nothing
  dart_50, dart_all   the same run with DART on: rounds/s; then once more with RL_FLAG_TIMING for k_dart_drop's device time per round with
               k > 0 (rl_get_timing, both data sets' launches inside one event pair), its bytes (2 k N of history + 24 N of scores) per second
               and that as a fraction of the streaming-read rate rl_debug_membench measures on the same device
  walk         what taking the trees out by walking them would cost: rl_adopt_model_text's time per tree (k_replay_scores, the plain run's
               model) times the mean k
Trainers are created and initialised outside the clocks.  Clocks are whatever the device runs at: nothing here reads or assumes a frequency."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch                                 # noqa: F401  (its HIP runtime has to be initialised before librlhip.so's: tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402

RATE = 0.1


def run(data, n_trees, n_leaves, max_drop=None, timing=False):
    """-> (rounds/s, trainer)"""
    g = N.Trainer(n_trees=n_trees, n_leaves=n_leaves, flags=N.RL_FLAG_TIMING if timing else 0)
    g.set_train(*data)
    if max_drop is not None:
        g.set_dart(RATE, max_drop, 0)
    g.init()
    t0 = time.perf_counter()
    g.boost_rounds_async(n_trees)
    g.sync()
    return n_trees / (time.perf_counter() - t0), g


def plain_only(shape):
    n_docs, F, kind, n_trees, n_leaves = synth.SHAPES[shape]
    rps, g = run(synth.make_dataset(n_docs, F, kind), n_trees, n_leaves)
    g.close()
    print(json.dumps(dict(plain_rounds_per_s=rps)))


def run_shape(shape, a):
    n_docs, F, kind, n_trees, n_leaves = synth.SHAPES[shape]
    data = synth.make_dataset(n_docs, F, kind)
    rec = dict(shape=shape, n_docs=n_docs, n_trees=n_trees, n_leaves=n_leaves, rate_drop=RATE, plain=[], parent_plain=[])
    text = None
    for _ in range(a.repeat):
        rps, g = run(data, n_trees, n_leaves)
        rec["plain"].append(round(rps, 2))
        text = text or g.model_text()
        g.close()
        if a.parent_lib:
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--plain-only", shape], env=dict(os.environ, RLHIP_LIB=os.path.abspath(a.parent_lib)))
            rec["parent_plain"].append(round(json.loads(out.decode().strip().splitlines()[-1])["plain_rounds_per_s"], 2))
    g = N.Trainer(n_trees=n_trees, n_leaves=n_leaves)
    g.set_train(*data)
    g.init()
    t0 = time.perf_counter()
    g.adopt_model_text(text)
    walk_ms_per_tree = (time.perf_counter() - t0) * 1e3 / n_trees
    g.close()
    ms, nbytes = N.membench(1, 1 << 30)
    read_gbs = nbytes / ms / 1e6
    rec.update(walk_ms_per_tree=round(walk_ms_per_tree, 4), membench_read_GBps=round(read_gbs, 1))
    for name, max_drop in (("dart_50", 50), ("dart_all", 0)):
        rps, g = run(data, n_trees, n_leaves, max_drop)
        ks = [len(g.dart_dropped(m)) for m in range(n_trees)]
        g.close()
        _, g = run(data, n_trees, n_leaves, max_drop, timing=True)
        dms, launches, dbytes = g.timing("DART_DROP")
        g.close()
        gbs = dbytes / dms / 1e6
        rec[name] = dict(rounds_per_s=round(rps, 2), mean_k=round(statistics.mean(ks), 2), max_k=max(ks), rounds_with_drops=launches,
                         drop_ms_per_round=round(dms / max(launches, 1), 4), drop_GBps=round(gbs, 1), fraction_of_read_rate=round(gbs / read_gbs, 3),
                         walk_ms_per_round=round(walk_ms_per_tree * statistics.mean(k for k in ks if k), 3))
    line = json.dumps(rec)
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--plain-only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dart_bench.jsonl"))
    a = ap.parse_args()
    if a.plain_only:
        plain_only(a.plain_only)
    else:
        for s in a.shapes.split(","):
            run_shape(s, a)
