"""Feature normalisation (rl_normalize_lists) on one MI355X, on ranklib_amd/synth.py data:

    python tools/norm_bench.py                     # the fold shape (720 000 documents, 136 features) and a small one
    python tools/norm_bench.py --shapes small      # one shape
    python tools/norm_bench.py --parts kernel,flow # without the -kcv legs (the list by list one is 25 passes over the file)

One JSON line per measurement, printed and written to --out (profiles/norm_bench.jsonl).
  "kernel": N.normalize_lists alone on the file's row matrix, for each kind: call_ms is the best of --repeat calls on the host clock (upload,
      launch, copy back: what a caller waits for), kernel_ms the launch alone between device events (rl_debug_normalize_times).  bytes is
      what the kind must move -- its passes over the requested cells (sum and linear read them twice, zscore three times) plus the write,
      4 bytes a cell -- and hbm_fraction is bytes / kernel_ms over the HBM peak (--hbm-tbs, a datasheet figure, not measured here).
  "flow": Normalizer.normalizeAll on the same in-memory ranked lists with Normalizer.batch = True ("batch") against False ("lists": the parent
      commit's code, list by list), for rows that are views of one matrix as the readers make them ("views") and for rows that each own
      their memory ("copied").  Every leg starts from a fresh copy of the rows; best and worst of --repeat-flow runs each.  The tool stops
      if the two legs' rows differ by a bit.
  "kcv": the normalisation of `-kcv 5 -norm sum` both ways: the loop of Evaluator.evaluate_kcv over all folds, once per fold, list by list,
      against one call with times = 25.  The list by list leg is run --repeat-kcv times (it is 25 passes over the file).
Clocks are whatever the device runs at: nothing here assumes a frequency."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ranklib_amd import _native as N          # noqa: E402
from ranklib_amd import normalizer as NM      # noqa: E402
from ranklib_amd import synth                 # noqa: E402
from ranklib_amd.features import FeatureManager          # noqa: E402
from ranklib_amd.learning import DataPoint, RankList     # noqa: E402

SHAPES = {"fold": (720000, 136), "small": (12000, 136)}
KINDS = ("sum", "zscore", "linear")
PASSES = {"sum": 2, "zscore": 3, "linear": 2}                # reads of every requested cell; one write on top


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def make_samples(rows, qoff, views):
    """ranked lists over a fresh copy of `rows`: row views of that copy (what _read_native makes), or one owned array per DataPoint"""
    M = rows.copy()
    fv = list(M) if views else [r.copy() for r in M]
    pts = [DataPoint.from_parsed(0.0, "", "", v) for v in fv]
    return [RankList(pts[qoff[q]:qoff[q + 1]]) for q in range(len(qoff) - 1)], pts


def bits_of(pts):
    return np.stack([p.fVals for p in pts]).view(np.uint32)


def run_shape(name, a, emit):
    n_docs, F = SHAPES[name]
    X, _, qoff = synth.make_dataset(n_docs, F)
    rows = np.full((n_docs, F + 1), np.nan, np.float32)       # fVals[0] is unused
    rows[:, 1:] = X
    cols = list(range(1, F + 1))
    lens = np.diff(qoff)
    shape = dict(shape=name, docs=int(n_docs), lists=len(lens), features=F, longest=int(lens.max()))
    for kind in KINDS if "kernel" in a.parts else ():
        N.normalize_lists(rows.copy(), qoff, cols, kind)                     # warm-up
        call, kern = [], []
        for _ in range(a.repeat):
            G = rows.copy()
            call.append(timed(lambda: N.normalize_lists(G, qoff, cols, kind)))
            kern.append(N.normalize_kernel_ms())
        nbytes = (PASSES[kind] + 1) * n_docs * F * 4
        emit(dict(shape, what="kernel", kind=kind, call_ms=round(min(call), 3), kernel_ms=round(min(kern), 4), bytes=nbytes,
                  tb_per_s=round(nbytes / (min(kern) * 1e-3) / 1e12, 3), hbm_fraction=round(nbytes / (min(kern) * 1e-3) / (a.hbm_tbs * 1e12), 4)))
    for views in (True, False) if "flow" in a.parts else ():
        for kind in KINDS:
            nm = NM.create(kind)
            ms, out = {True: [], False: []}, {}
            for batch in (True, False):
                NM.Normalizer.batch = batch
                try:
                    for _ in range(a.repeat_flow + (1 if batch else 0)):     # the batch leg's first run is its warm-up
                        samples, pts = make_samples(rows, qoff, views)
                        ms[batch].append(timed(lambda: nm.normalizeAll(samples, cols)))
                    out[batch] = bits_of(pts)
                finally:
                    NM.Normalizer.batch = True
            if not np.array_equal(out[True], out[False]):
                raise SystemExit("%s %s: the rows of the batch and the list by list leg differ" % (name, kind))
            b, l = ms[True][1:], ms[False]
            emit(dict(shape, what="flow", rows="views" if views else "copied", kind=kind, batch_ms=round(min(b), 2), batch_worst_ms=round(max(b), 2),
                      lists_ms=round(min(l), 2), lists_worst_ms=round(max(l), 2), ratio=round(min(l) / min(b), 2), bits_equal=True))
    if "kcv" not in a.parts:
        return
    nm, nFold = NM.create("sum"), 5
    ms, out = {True: [], False: []}, {}
    for batch in (True, False):
        NM.Normalizer.batch = batch
        try:
            for _ in range(a.repeat_flow if batch else a.repeat_kcv):
                samples, pts = make_samples(rows, qoff, True)
                groups = FeatureManager.prepareCV(samples, nFold)

                def kcv():                                                   # Evaluator.evaluate_kcv's normalisation
                    if nm.normalizeBatch(samples, cols, times=nFold * nFold):
                        return
                    for _ in range(nFold):
                        print("kcv: one pass over all folds, list by list ...", file=sys.stderr, flush=True)
                        for group in groups:
                            for fold in group:
                                nm.normalizeAll(fold, cols)
                ms[batch].append(timed(kcv))
            out[batch] = bits_of(pts)
        finally:
            NM.Normalizer.batch = True
    if not np.array_equal(out[True], out[False]):
        raise SystemExit("%s: the rows of the -kcv normalisation differ between the batch and the list by list leg" % name)
    emit(dict(shape, what="kcv", kind="sum", folds=nFold, times=nFold * nFold, batch_ms=round(min(ms[True]), 2), batch_worst_ms=round(max(ms[True]), 2),
              lists_ms=round(min(ms[False]), 2), lists_worst_ms=round(max(ms[False]), 2), ratio=round(min(ms[False]) / min(ms[True]), 2),
              bits_equal=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,fold")
    ap.add_argument("--parts", default="kernel,flow,kcv", help="which measurements to take")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--repeat-flow", type=int, default=3)
    ap.add_argument("--repeat-kcv", type=int, default=1)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s the byte rate is taken against (MI355X datasheet: 8)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_bench.jsonl"))
    a = ap.parse_args()
    a.parts = a.parts.split(",")
    import logging
    logging.getLogger("ranklib_amd").setLevel(logging.WARNING)
    if N.device_count() < 1:
        print(json.dumps(dict(refused="no gfx950 device visible: the batch leg would be the list by list path")))
        return 1
    with open(a.out, "w", encoding="ascii") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        try:
            for name in [s for s in a.shapes.split(",") if s]:
                run_shape(name, a, emit)
        except N.RankLibError as ex:
            emit(dict(refused=str(ex)))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
