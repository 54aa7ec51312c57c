"""Writing LETOR text (FeatureManager.save): the native writer (rl_letor_format, at most 16 host threads) against the Python
writer (DataPoint.toString) on synth.py data.  Host only: no device is touched.

    python tools/letor_write_bench.py [--docs 100000] [--features 136] [--repeat 3]

Prints one JSON line per writer -- lines/s and MB/s of the best repeat, the threads the native writer may use -- and one for the pair;
it stops if the two files differ by a byte."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                           # noqa: E402

from ranklib_amd import _native as N                         # noqa: E402
from ranklib_amd import synth                                # noqa: E402
from ranklib_amd.features import FeatureManager              # noqa: E402
from ranklib_amd.learning import DataPoint, RankList         # noqa: E402


def lists_of(n_docs, n_features):
    X, lab, qoff = synth.make_dataset(n_docs, n_features, "mslr")
    rows = np.full((n_docs, n_features + 1), np.nan, np.float32)         # column 0 unused, as in DataPoint.fVals
    rows[:, 1:] = X
    out = []
    for q in range(len(qoff) - 1):
        out.append(RankList([DataPoint.from_parsed(float(lab[i]), "q%d" % q, "#docid = %d" % i, rows[i]) for i in range(qoff[q], qoff[q + 1])]))
    return out


def timed(samples, path, native, repeat):
    FeatureManager.native = native
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        FeatureManager.save(samples, path)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--features", type=int, default=136)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    if not hasattr(N.lib(), "rl_letor_format"):
        sys.exit("this librlhip.so has no rl_letor_format")
    samples = lists_of(a.docs, a.features)
    threads = min(16, os.cpu_count() or 1, a.docs // 2048 + 1)      # thread_count of rl_letor.cpp
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for name, native in (("native", True), ("python", False)):
            path = os.path.join(d, name + ".txt")
            dt = timed(samples, path, native, a.repeat if native else 1)
            size = os.path.getsize(path)
            res[name] = dict(writer=name, docs=a.docs, features=a.features, seconds=round(dt, 3), lines_per_s=round(a.docs / dt), mb_per_s=round(size / dt / 1e6, 1),
                             bytes=size, threads=threads if native else 1)
            print(json.dumps(res[name]), flush=True)
        with open(os.path.join(d, "native.txt"), "rb") as f, open(os.path.join(d, "python.txt"), "rb") as g:
            if f.read() != g.read():
                sys.exit("the two writers' files differ")
    print(json.dumps(dict(byte_equal=True, native_over_python=round(res["python"]["seconds"] / res["native"]["seconds"], 1))))


if __name__ == "__main__":
    main()
