"""Refit (rl_refit_model_text) on one MI355X, on ranklib_amd/synth.py data, at the bench shapes c1 and c2 (MSLR-WEB10K /
WEB30K sizes, 1 000 trees of 31 leaves):

    python tools/refit_bench.py                    # c1 and c2
    python tools/refit_bench.py --shapes c1        # one shape

One JSON line per shape, printed and appended to --out (profiles/refit_bench.jsonl).  Per shape, the whole model of n_trees trees:
  train   the trees grown by the trainer: rl_boost_rounds_async + rl_sync, no validation set -- without a refit the only way to get
          n_trees trees whose leaf values are fitted to the data;
  adopt   a fresh, initialised trainer adopts the model text (rl_adopt_model_text): the floor, walks and metrics without any leaf work;
  tiled   a fresh, initialised trainer refits the model text with decay 0 (k_refit_route from an LDS tile);
  direct  the same with RLHIP_REFIT_DIRECT (rows read from global memory).
The model text is taken from the trained run (outside every clock), trainers are created and initialised outside the clock.  The tool stops
unless the refit on the training data reproduces the model bit for bit -- every leaf output through the model text, the scores and the round
metrics -- under both arms.  --repeat rounds after one warm-up round, the legs taking turns inside every round; host clock around the calls
(what a caller waits for).  Reported: median and least - largest of every leg, the legs' cost per round, and refit_over_train =
median refit / median train.  Clocks are whatever the device runs at: nothing here reads or assumes a frequency."""
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
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402

LEGS = ("train", "adopt", "tiled", "direct")


def spread(ms):
    return dict(median=round(statistics.median(ms), 2), least=round(min(ms), 2), largest=round(max(ms), 2))


def trainer(data, n_trees, n_leaves, direct=False):
    if direct:
        os.environ["RLHIP_REFIT_DIRECT"] = "1"            # a trainer reads its knobs when it is created
    else:
        os.environ.pop("RLHIP_REFIT_DIRECT", None)
    g = N.Trainer(n_trees=n_trees, n_leaves=n_leaves)
    g.set_train(*data)
    g.init()
    os.environ.pop("RLHIP_REFIT_DIRECT", None)
    return g


def state(g, rounds):
    return g.array("SCORE").view(np.uint64), np.array([g.round_metrics(r)[0] for r in range(rounds)], np.float32).view(np.uint32)


def run_shape(name, a):
    n_docs, F, kind, n_trees, n_leaves = synth.SHAPES[name]
    if a.trees:
        n_trees = a.trees
    data = synth.make_dataset(n_docs, F, kind)
    ms = {leg: [] for leg in LEGS}
    for r in range(a.repeat + 1):                          # round 0 warms up
        g = trainer(data, n_trees, n_leaves)
        t0 = time.perf_counter()
        g.boost_rounds_async(n_trees)
        g.sync()
        t = (time.perf_counter() - t0) * 1e3
        if r:
            ms["train"].append(t)
        text, want = g.model_text(), state(g, n_trees)
        g.close()
        for leg in LEGS[1:]:
            c = trainer(data, n_trees, n_leaves, leg == "direct")
            t0 = time.perf_counter()
            if leg == "adopt":
                c.adopt_model_text(text)
            else:
                c.refit_model_text(text, 0.0)
            t = (time.perf_counter() - t0) * 1e3
            if r:
                ms[leg].append(t)
            got, stats = state(c, n_trees), c.refit_stats()
            same_text = leg == "adopt" or c.model_text() == text
            c.close()
            if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_text):
                raise SystemExit("%s: the %s leg does not reproduce the trained model bit for bit" % (name, leg))
            if leg != "adopt" and stats != ((n_trees, 0, 0) if leg == "tiled" else (0, n_trees, 0)):
                raise SystemExit("%s: the %s leg took the other arm or kept a leaf: %r" % (name, leg, stats))
        print("[refit_bench] %s: round %d of %d done" % (name, r, a.repeat), file=sys.stderr, flush=True)
    out = dict(shape=name, docs=int(n_docs), lists=len(data[2]) - 1, features=F, trees=n_trees, leaves=n_leaves, repeats=a.repeat, validation=False,
               equal_bits=True, clocks="not read")
    for leg in LEGS:
        out[leg + "_ms"] = spread(ms[leg])
        out[leg + "_ms_per_round"] = round(out[leg + "_ms"]["median"] / n_trees, 4)
    best = min(("tiled", "direct"), key=lambda leg: out[leg + "_ms"]["median"])
    out["faster_arm"] = best
    out["refit_over_train"] = round(out[best + "_ms"]["median"] / out["train_ms"]["median"], 3)
    out["refit_under_half_a_training_round"] = bool(2 * out[best + "_ms"]["largest"] < out["train_ms"]["least"])
    out["direct_over_tiled"] = round(out["direct_ms"]["median"] / out["tiled_ms"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--trees", type=int, default=0, help="fewer trees than the shape's (a trial run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_bench.jsonl"))
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
