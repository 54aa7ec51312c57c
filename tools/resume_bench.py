"""Resume (rl_adopt_model_text) on one MI355X, on ranklib_amd/synth.py data, at the bench shapes c1 and c2 (MSLR-WEB10K /
WEB30K sizes, 1 000 trees of 31 leaves):

    python tools/resume_bench.py                    # c1 and c2
    python tools/resume_bench.py --shapes c1        # one shape

One JSON line per shape, printed and appended to --out (profiles/resume_bench.jsonl).  Per shape, for T0 = 500 and T0 = 1 000:
  train   rounds 0 .. T0 - 1 grown by the trainer: rl_boost_rounds_async + rl_sync, no validation set -- the fastest way the trainer has to
          reach the state after T0 rounds, and without rl_adopt_model_text the only one;
  tiled   a fresh, initialised trainer adopts the T0-tree model text (k_replay_scores from an LDS tile);
  direct  the same with RLHIP_REPLAY_DIRECT (rows read from global memory).
The model text is taken from the trained run (outside every clock), trainers are created and initialised outside the clock.  The tool
stops unless the adopted trainer's scores and round metrics equal the trained one's bit for bit, under both arms.  --repeat rounds after
one warm-up round, the legs taking turns inside every round; host clock around the calls (what a caller waits for).  Reported: median and
least - largest of every leg; tiled_faster_than_direct / adopt_faster_than_train = the slower leg's least is above the faster leg's
largest, i.e. the gap is more than either leg's own spread.  Clocks are whatever the device runs at: nothing here reads or assumes a
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
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402

STAGES = (500, 1000)


def spread(ms):
    return dict(median=round(statistics.median(ms), 2), least=round(min(ms), 2), largest=round(max(ms), 2))


def trainer(data, n_trees, n_leaves, direct):
    if direct:
        os.environ["RLHIP_REPLAY_DIRECT"] = "1"           # a trainer reads its knobs when it is created
    else:
        os.environ.pop("RLHIP_REPLAY_DIRECT", None)
    g = N.Trainer(n_trees=n_trees, n_leaves=n_leaves)
    g.set_train(*data)
    g.init()
    os.environ.pop("RLHIP_REPLAY_DIRECT", None)
    return g


def state(g, rounds):
    return g.array("SCORE").view(np.uint64), np.array([g.round_metrics(r)[0] for r in range(rounds)], np.float32).view(np.uint32)


def run_shape(name, a):
    n_docs, F, kind, n_trees, n_leaves = synth.SHAPES[name]
    stages = [s for s in STAGES if s <= n_trees]
    data = synth.make_dataset(n_docs, F, kind)
    ms = {(leg, s): [] for leg in ("train", "tiled", "direct") for s in stages}
    for r in range(a.repeat + 1):                          # round 0 warms up
        g = trainer(data, n_trees, n_leaves, False)
        texts, want, done, t_train = {}, {}, 0, 0.0
        for s in stages:
            t0 = time.perf_counter()
            g.boost_rounds_async(s - done)
            g.sync()
            t_train += (time.perf_counter() - t0) * 1e3
            done = s
            if r:
                ms[("train", s)].append(t_train)
            texts[s], want[s] = g.model_text(), state(g, s)
        g.close()
        for s in stages:
            for leg in ("tiled", "direct"):
                c = trainer(data, n_trees, n_leaves, leg == "direct")
                t0 = time.perf_counter()
                c.adopt_model_text(texts[s])
                t = (time.perf_counter() - t0) * 1e3
                if r:
                    ms[(leg, s)].append(t)
                got = state(c, s)
                arms = c.array("LAUNCH_ARMS")
                c.close()
                if not (np.array_equal(got[0], want[s][0]) and np.array_equal(got[1], want[s][1])):
                    raise SystemExit("%s: the %s replay of %d trees differs from the trained state" % (name, leg, s))
                if (arms[N.ARM["REPLAY_TILED"]] > 0) != (leg == "tiled") or (arms[N.ARM["REPLAY_DIRECT"]] > 0) != (leg == "direct"):
                    raise SystemExit("%s: the %s leg took the other arm" % (name, leg))
        print("[resume_bench] %s: round %d of %d done" % (name, r, a.repeat), file=sys.stderr, flush=True)
    out = dict(shape=name, docs=int(n_docs), lists=len(data[2]) - 1, features=F, trees=n_trees, leaves=n_leaves, repeats=a.repeat, validation=False,
               equal_bits=True, clocks="not read")
    for s in stages:
        tr, ti, di = spread(ms[("train", s)]), spread(ms[("tiled", s)]), spread(ms[("direct", s)])
        best = ti if ti["median"] <= di["median"] else di
        out["T0_%d" % s] = dict(train_ms=tr, adopt_tiled_ms=ti, adopt_direct_ms=di, train_over_tiled=round(tr["median"] / ti["median"], 2),
                                direct_over_tiled=round(di["median"] / ti["median"], 2), tiled_faster_than_direct=bool(di["least"] > ti["largest"]),
                                direct_faster_than_tiled=bool(ti["least"] > di["largest"]), adopt_faster_than_train=bool(tr["least"] > best["largest"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume_bench.jsonl"))
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
