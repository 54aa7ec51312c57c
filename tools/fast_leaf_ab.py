"""RL_FLAG_FAST_LEAF beside the default leaves on one MI355X: what the flag buys a round, and what it changes in a run.

    python tools/fast_leaf_ab.py speed     [--shape c2] [--rounds 40] [--repeat 7] [--warmup 10]
    python tools/fast_leaf_ab.py deviation [--shape c1] [--rounds 100]

speed: ONE process, ONE synthetic data set of the shape, four trainers on it -- default, FAST_LEAF, FIRST_TIE, FAST_LEAF | FIRST_TIE -- warmed up, then
taken in turns: every repeat gives every trainer the same `rounds` further rounds (rl_boost_rounds_async + rl_sync, a host clock around both: the
sync ends in a device synchronise).  One JSON line per setting: rounds/s as the median of the repeats, the repeats themselves, and the spread.  The
settings grow their own models (a leaf value that differs feeds the next round), so equal round numbers are not equal trees: the figure is the pace
of the boosting loop, the thing a user waits for.

deviation: the default trainer is the reference.  Both train `rounds` rounds on the shape with its held-out set (synth.make_heldout) passed as
validation data, early stopping off.  While both have grown the same splits so far, the leaf values of a round are comparable: max |fast - default|
over those leaves; the first round whose tree stores a different split ends that comparison.  Then NDCG@10 on the training and the held-out set of
both final models (rl_finish).  One JSON line.

Nothing here sets a threshold: DESIGN.md 14 quotes what this printed.  Without a gfx950 device both modes fail in rl_create.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import synth                 # noqa: E402


def note(msg):
    print("[fast_leaf_ab] " + msg, file=sys.stderr, flush=True)


SETTINGS = [("default", 0), ("fast_leaf", N.RL_FLAG_FAST_LEAF), ("first_tie", N.RL_FLAG_FIRST_TIE),
            ("fast_leaf+first_tie", N.RL_FLAG_FAST_LEAF | N.RL_FLAG_FIRST_TIE)]


def speed(a):
    n_docs, n_feat, kind, _, leaves = synth.SHAPES[a.shape]
    t_gen = time.perf_counter()
    X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    note("%s: %d x %d generated in %.1f s" % (a.shape, n_docs, n_feat, time.perf_counter() - t_gen))
    total = a.warmup + a.rounds * a.repeat
    trainers = []
    for name, flags in SETTINGS:
        t = N.Trainer(n_trees=total, n_leaves=leaves, flags=flags)
        t.set_train(X, lab, qoff)
        t.init()
        t.boost_rounds_async(a.warmup)
        t.sync()
        note("%s: initialised and warmed up" % name)
        trainers.append((name, flags, t, []))
    for rep in range(a.repeat):
        order = trainers if rep % 2 == 0 else trainers[::-1]       # alternate the order too: whoever runs first meets the coolest chip
        for name, flags, t, times in order:
            t0 = time.perf_counter()
            t.boost_rounds_async(a.rounds)
            t.sync()
            times.append(time.perf_counter() - t0)
    base = None
    for name, flags, t, times in trainers:
        rps = [a.rounds / s for s in times]
        med = statistics.median(rps)
        base = med if base is None else base
        tm, _ = t.round_metrics(total - 1)
        print(json.dumps(dict(mode="speed", shape=a.shape, n_docs=n_docs, n_features=n_feat, leaves=leaves, setting=name, flags=flags, warmup_rounds=a.warmup,
                              rounds_per_repeat=a.rounds, repeats=a.repeat, rounds_per_s_median=round(med, 2), rounds_per_s_min=round(min(rps), 2),
                              rounds_per_s_max=round(max(rps), 2), rounds_per_s=[round(v, 2) for v in rps], vs_default=round(med / base, 4),
                              train_ndcg_last_round=float(tm))), flush=True)
        t.close()
    return 0


def same_splits(x, y):
    return (x.n_nodes == y.n_nodes and np.array_equal(x.feature[:x.n_nodes], y.feature[:y.n_nodes]) and
            np.array_equal(x.threshold[:x.n_nodes].view(np.uint32), y.threshold[:y.n_nodes].view(np.uint32)) and
            np.array_equal(x.left[:x.n_nodes], y.left[:y.n_nodes]) and np.array_equal(x.right[:x.n_nodes], y.right[:y.n_nodes]))


def deviation(a):
    n_docs, n_feat, kind, _, leaves = synth.SHAPES[a.shape]
    X, lab, qoff = synth.make_dataset(n_docs, n_feat, kind)
    Xv, labv, qv = synth.make_heldout(a.shape)
    note("%s: %d training and %d held-out documents generated" % (a.shape, n_docs, len(labv)))
    pair = []
    for flags in (0, N.RL_FLAG_FAST_LEAF):
        t = N.Trainer(n_trees=a.rounds, n_leaves=leaves, flags=flags, early_stop_rounds=1 << 30)
        t.set_train(X, lab, qoff)
        t.set_validation(Xv, labv, qv)
        t.init()
        pair.append(t)
    ref, fast = pair
    first_other_split, max_dev, leaves_compared, leaves_other_bits, largest_leaf = None, 0.0, 0, 0, 0
    worst = dict(round=None, count=None)
    tm_ref = tm_fast = vm_ref = vm_fast = 0.0
    for r in range(a.rounds):
        tr, tm_ref, vm_ref, _ = ref.boost_round()
        tf, tm_fast, vm_fast, _ = fast.boost_round()
        if first_other_split is None:
            if not same_splits(tr, tf):
                first_other_split = r + 1
            else:
                lf = tr.feature[:tr.n_nodes] == -1
                d = np.abs(tr.output[:tr.n_nodes][lf].astype(np.float64) - tf.output[:tf.n_nodes][lf].astype(np.float64))
                leaves_compared += int(lf.sum())
                leaves_other_bits += int((tr.output[:tr.n_nodes][lf].view(np.uint32) != tf.output[:tf.n_nodes][lf].view(np.uint32)).sum())
                largest_leaf = max(largest_leaf, int(tr.count[:tr.n_nodes][lf].max()))
                if d.max() > max_dev:
                    max_dev = float(d.max())
                    worst = dict(round=r + 1, count=int(tr.count[:tr.n_nodes][lf][int(d.argmax())]))
    note("%d rounds trained twice" % a.rounds)
    ts_ref, vs_ref = ref.finish()
    ts_fast, vs_fast = fast.finish()
    print(json.dumps(dict(mode="deviation", shape=a.shape, n_docs=n_docs, n_features=n_feat, leaves=leaves, rounds=a.rounds, heldout_docs=int(len(labv)),
                          first_round_with_another_split=first_other_split, rounds_with_the_same_splits=(first_other_split or a.rounds + 1) - 1,
                          leaves_compared=leaves_compared, leaves_with_other_bits=leaves_other_bits, largest_leaf_compared=largest_leaf,
                          max_abs_leaf_value_deviation=max_dev, worst_leaf=worst,
                          ndcg10_train_default=ts_ref, ndcg10_train_fast=ts_fast, ndcg10_train_diff=ts_fast - ts_ref,
                          ndcg10_heldout_default=vs_ref, ndcg10_heldout_fast=vs_fast, ndcg10_heldout_diff=vs_fast - vs_ref,
                          last_round_float_metric=dict(train_default=float(tm_ref), train_fast=float(tm_fast), heldout_default=float(vm_ref),
                                                       heldout_fast=float(vm_fast)))), flush=True)
    ref.close(); fast.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["speed", "deviation"])
    ap.add_argument("--shape", default=None, help="a ranklib_amd.synth.SHAPES entry (speed: c2, deviation: c1)")
    ap.add_argument("--rounds", type=int, default=None, help="speed: rounds per repeat (40); deviation: rounds trained (100)")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    a.shape = a.shape or ("c2" if a.mode == "speed" else "c1")
    a.rounds = a.rounds or (40 if a.mode == "speed" else 100)
    try:
        return speed(a) if a.mode == "speed" else deviation(a)
    except N.RankLibError as ex:
        print(json.dumps(dict(mode=a.mode, shape=a.shape, refused=str(ex))))
        return 1


if __name__ == "__main__":
    sys.exit(main())
