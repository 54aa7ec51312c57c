"""The lambda kernels of the tree trainer per train metric on one MI355X, at a shape of bench.py (default c2):

    python tools/lambda_metric_bench.py                       # NDCG@10, P@10, RR@10 fused, and P@10, RR@10 through the pair-term matrix
    python tools/lambda_metric_bench.py --shape c1 --repeat 7

One JSON line per run and one summary line per configuration, printed and written to --out (profiles/pr_lambda_bench.jsonl).
  A run is a fresh trainer on the shape's data: --warmup rounds (default 5), rl_reset_timing, then --rounds rounds (default 20: rounds 6 .. 25) with
  RL_FLAG_TIMING; lambda_ms_per_round is RL_KERNEL_LAMBDA of rl_get_timing over those rounds, device events around everything enqueue_lambdas
  launches (all length classes, side streams joined), divided by the rounds.  round_ms is the host clock around the same rounds, enqueue to sync.
  The configurations take turns inside every repeat (a, b, c, a, b, c, ..), so a drift of the machine reaches all of them alike; the summary gives
  the median, the least and the largest run, and spread = (largest - least) / median of that configuration's own repeats.
  "unfused" runs set RLHIP_LAMBDA_UNFUSED for the trainer they create and remove it afterwards.
Clocks are whatever the device runs at: nothing here assumes a frequency."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402

CONFIGS = [("NDCG", "fused"), ("P", "fused"), ("RR", "fused"), ("P", "unfused"), ("RR", "unfused")]


def one_run(data, leaves, metric, path, warmup, rounds):
    X, lab, qoff = data
    if path == "unfused":
        os.environ["RLHIP_LAMBDA_UNFUSED"] = "1"
    try:
        g = N.Trainer(n_trees=warmup + rounds, n_leaves=leaves, metric=metric, metric_k=10, flags=N.RL_FLAG_TIMING)
    finally:
        os.environ.pop("RLHIP_LAMBDA_UNFUSED", None)
    try:
        g.set_train(X, lab, qoff)
        g.init()
        g.boost_rounds_async(warmup)
        g.sync()
        g.reset_timing()
        t0 = time.perf_counter()
        g.boost_rounds_async(rounds)
        g.sync()
        host_ms = (time.perf_counter() - t0) * 1e3
        ms, launches, _ = g.timing("LAMBDA")
        arms = g.array("LAUNCH_ARMS")
        took_unfused = int(arms[N.ARM["LAM_UNFUSED"]]) > 0
        if took_unfused != (path == "unfused") or launches != rounds:
            raise SystemExit("%s %s: the trainer took another path than asked for (unfused launches %d, timed rounds %d)" % (metric, path, arms[N.ARM["LAM_UNFUSED"]], launches))
        return dict(lambda_ms_per_round=ms / rounds, round_ms=host_ms / rounds, train_metric=float(g.round_metrics(warmup + rounds - 1)[0]))
    finally:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2", help="a shape of ranklib_amd.synth.SHAPES")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_lambda_bench.jsonl"))
    a = ap.parse_args()
    if N.device_count() < 1:
        print(json.dumps(dict(refused="no gfx950 device visible")))
        return 1
    n_docs, n_feat, kind, _, leaves = synth.SHAPES[a.shape]
    X, lab, qoff, _ = synth.make_shard(n_docs, n_feat, kind, 0, 1)
    shape = dict(shape=a.shape, docs=int(n_docs), features=int(n_feat), lists=len(qoff) - 1, leaves=int(leaves), k=10, rounds="%d..%d" % (a.warmup + 1, a.warmup + a.rounds))
    runs = {c: [] for c in CONFIGS}
    with open(a.out, "w", encoding="ascii") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for rep in range(a.repeat):
            for c in CONFIGS:
                r = one_run((X, lab, qoff), leaves, c[0], c[1], a.warmup, a.rounds)
                runs[c].append(r)
                emit(dict(shape, what="run", metric=c[0] + "@10", path=c[1], repeat=rep, lambda_ms_per_round=round(r["lambda_ms_per_round"], 5),
                          round_ms=round(r["round_ms"], 4), train_metric=r["train_metric"]))
        for c in CONFIGS:
            v = sorted(r["lambda_ms_per_round"] for r in runs[c])
            med = statistics.median(v)
            emit(dict(shape, what="summary", metric=c[0] + "@10", path=c[1], repeats=len(v), lambda_ms_median=round(med, 5), lambda_ms_min=round(v[0], 5),
                      lambda_ms_max=round(v[-1], 5), spread=round((v[-1] - v[0]) / med, 4),
                      round_ms_median=round(statistics.median(r["round_ms"] for r in runs[c]), 4)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
