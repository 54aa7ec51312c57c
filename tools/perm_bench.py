"""The Analyzer's randomisation test (rl_perm_test) on one MI355X: the call's time beside a serial-chain model and the
Java's loop on one host thread.

    python tools/perm_bench.py                               # n = 2 000 and 10 000, -np 10^4 and 10^6, 1 and 8 targets
    python tools/perm_bench.py --n 61 --np 10000 --targets 3 # one shape

One JSON line per shape.  call_ms is the best of --repeat calls of rl_perm_test on the host clock: the upload of the arrays, the launch
and the copy of the counts, what a caller waits for.  add_ns is measured here, not taken from a datasheet: one wavefront runs one
dependent chain of f64 adds at two lengths between device events (rl_debug_perm_calib), the difference divided by the adds.  model_ms =
ceil(wavefronts / SIMDs) * n * add_ns: a lane's two sums are independent chains that overlap, so an element costs one dependent add,
and wavefronts beyond one per SIMD are priced as if they queued (they interleave instead, so the model is an upper estimate there and
ratio = call_ms / model_ms falls below 1).  host_ms_per_perm is RandomPermutationTest.test's loop as written (digit strings, copies
into pb / pt, two serial means) in C++ on one host thread over --host-perms permutations, and host_ms that figure times -np; the counts
of those permutations from the host and from the GPU must agree or the tool stops.  There is no parent-commit number: the capability
is new."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ranklib_amd import _native as N          # noqa: E402

WAVE = 64


def run(n, np_, targets, seed, repeat, host_perms, add_ns, n_simd):
    rng = np.random.default_rng(n + targets)
    b = rng.random(n)
    t = np.clip(b[None, :] + rng.standard_normal((targets, n)) * 0.1, 0.0, 1.0)
    best, count = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        count, _, _ = N.perm_test(b, t, seed, 0, np_)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    hp = min(host_perms, np_)
    _, host_ms, host_count = N.perm_calib(1 << 16, b, t[0], seed, hp)
    gpu_head, _, _ = N.perm_test(b, t[:1], seed, 0, hp)
    if int(gpu_head[0]) != host_count:
        raise SystemExit("host loop and GPU disagree on the first %d permutations: %d vs %d" % (hp, host_count, int(gpu_head[0])))
    waves = -(-np_ // WAVE) * targets
    model = -(-waves // n_simd) * n * add_ns * 1e-6
    return dict(n=n, np=np_, targets=targets, call_ms=round(best, 4), add_ns=round(add_ns, 3), wavefronts=waves, simds=n_simd,
                model_ms=round(model, 4), ratio=round(best / model, 3), host_perms=hp, host_ms_per_perm=round(host_ms / hp, 6),
                host_ms=round(host_ms / hp * np_ * targets, 2), speedup_vs_host=round(host_ms / hp * np_ * targets / best, 1),
                p=[float(c) / np_ for c in count])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="2000,10000")
    ap.add_argument("--np", default="10000,1000000")
    ap.add_argument("--targets", default="1,8")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-perms", type=int, default=2000)
    ap.add_argument("--simds", type=int, default=256 * 4, help="SIMDs of the device (MI355X: 256 CUs of 4)")
    ap.add_argument("--chain", type=int, default=1 << 22, help="f64 adds of the calibration chain")
    a = ap.parse_args()
    try:
        N.perm_calib(1 << 16)                                                   # warm-up
        add_ns = float(np.median([N.perm_calib(a.chain)[0] for _ in range(5)]))
        n_simd = a.simds
        for n in [int(v) for v in a.n.split(",")]:
            for np_ in [int(v) for v in a.np.split(",")]:
                for k in [int(v) for v in a.targets.split(",")]:
                    print(json.dumps(run(n, np_, k, a.seed, a.repeat, a.host_perms, add_ns, n_simd)), flush=True)
    except N.RankLibError as ex:
        print(json.dumps(dict(refused=str(ex))))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
