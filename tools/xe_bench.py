"""The XE-NDCG objective (rl_set_objective, k_lambda_xe) on one MI355X, on ranklib_amd/synth.py data, at the bench shapes c1 and c2
(trees of 31 leaves):

    python tools/xe_bench.py [--shapes c1,c2] [--rounds 300] [--parent-lib build_ab/librlhip_parent.so]

One JSON line per shape, printed and appended to --out (profiles/xe_bench.jsonl).  Per shape, with the objective off ("lambda") and on ("xendcg"):
  rounds_per_s   rl_boost_rounds_async + rl_sync of --rounds rounds, host clock; the two objectives take turns --repeat times, and with
                 --parent-lib the parent commit's library runs the off leg in a child process of this tool (RLHIP_LIB) in the same turns: the
                 objective switched off must cost nothing
  lambda_ms      one more run each with RL_FLAG_TIMING: the device time of the launches under RL_KERNEL_LAMBDA per round (rl_get_timing; the
                 pairwise objective's several launches inside one event pair, k_lambda_xe alone)
  xe_GBps        k_lambda_xe's bytes -- 28 a document: score, label, (lambda, w) -- per second, and that as a fraction of the streaming-read
                 rate rl_debug_membench measures on the same device
  quality        train and held-out (synth.make_heldout) NDCG@10 of both objectives after --rounds trees with a validation set, early stopping
                 out of reach.  Reported, not compared: they are different losses
Trainers are created and initialised outside the clocks.  Clocks are whatever the device runs at: nothing here reads or assumes a frequency."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch                                 # noqa: F401  (its HIP runtime has to be initialised before librlhip.so's: tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402

OBJECTIVES = ("lambda", "xendcg")


def trainer(data, rounds, n_leaves, objective, flags=0, valid=None):
    g = N.Trainer(n_trees=rounds, n_leaves=n_leaves, flags=flags, early_stop_rounds=rounds + 1)
    g.set_train(*data)
    if valid is not None:
        g.set_validation(*valid)
    if objective != "lambda":
        g.set_objective(objective, 0)
    g.init()
    return g


def run(data, rounds, n_leaves, objective, flags=0):
    """-> (rounds/s, trainer)"""
    g = trainer(data, rounds, n_leaves, objective, flags)
    t0 = time.perf_counter()
    g.boost_rounds_async(rounds)
    g.sync()
    return rounds / (time.perf_counter() - t0), g


def plain_only(shape, rounds):
    """the child process of the parent library's leg"""
    n_docs, F, kind, _, n_leaves = synth.SHAPES[shape]
    rps, g = run(synth.make_dataset(n_docs, F, kind), rounds, n_leaves, "lambda")
    g.close()
    print(json.dumps(dict(plain_rounds_per_s=rps)))


def note(*what):
    print(*what, file=sys.stderr, flush=True)


def run_shape(shape, a):
    n_docs, F, kind, _, n_leaves = synth.SHAPES[shape]
    data = synth.make_dataset(n_docs, F, kind)
    note(shape, "data made")
    rec = dict(shape=shape, n_docs=n_docs, rounds=a.rounds, n_leaves=n_leaves, rounds_per_s={o: [] for o in OBJECTIVES}, parent_rounds_per_s=[])
    for _ in range(a.repeat):
        for o in OBJECTIVES:
            rps, g = run(data, a.rounds, n_leaves, o)
            g.close()
            rec["rounds_per_s"][o].append(round(rps, 2))
            note(shape, o, "%.1f rounds/s" % rps)
        if a.parent_lib:
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--plain-only", shape, "--rounds", str(a.rounds)],
                                          env=dict(os.environ, RLHIP_LIB=os.path.abspath(a.parent_lib)))
            rec["parent_rounds_per_s"].append(round(json.loads(out.decode().strip().splitlines()[-1])["plain_rounds_per_s"], 2))
    ms, nbytes = N.membench(1, 1 << 30)
    read_gbs = nbytes / ms / 1e6
    rec["membench_read_GBps"] = round(read_gbs, 1)
    rec["lambda_ms"] = {}
    for o in OBJECTIVES:
        _, g = run(data, a.rounds, n_leaves, o, flags=N.RL_FLAG_TIMING)
        lms, launches, lbytes = g.timing("LAMBDA")
        g.close()
        rec["lambda_ms"][o] = round(lms / max(launches, 1), 4)
        note(shape, o, "lambda kernels %.4f ms a round" % rec["lambda_ms"][o])
        if o == "xendcg":
            gbs = lbytes / lms / 1e6
            rec.update(xe_GBps=round(gbs, 1), xe_fraction_of_read_rate=round(gbs / read_gbs, 3))
    valid = synth.make_heldout(shape)
    rec["quality"] = {}
    for o in OBJECTIVES:
        g = trainer(data, a.rounds, n_leaves, o, valid=valid)
        for _ in range(a.rounds):
            g.boost_round(want_tree=False)
        tm, vm = g.round_metrics(a.rounds - 1)
        g.close()
        rec["quality"][o] = dict(train_ndcg10=round(float(tm), 5), heldout_ndcg10=round(float(vm), 5))
    line = json.dumps(rec)
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--plain-only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xe_bench.jsonl"))
    a = ap.parse_args()
    if a.plain_only:
        plain_only(a.plain_only, a.rounds)
    else:
        for s in a.shapes.split(","):
            run_shape(s, a)
