"""Scoring with a RankNet / LambdaRank / ListNet model on one MI355X: rl_net_predict_device on rows that are resident on the device.

    python tools/net_bench.py                              # c2's rows (3.77 M x 136, row stride 137), hidden [] and [10]
    python tools/net_bench.py --hidden ";10;33" --repeats 30 --lin-score-ms 0.41
    rocprofv3 --kernel-trace --stats ... -- python tools/net_bench.py --profile-pass      # the kernels' own times, k_lin_score's among them

One JSON line per network.  ms is one launch between two device events: after --warmup launches, --repeats (>= 20) launches are timed one
by one and the median, the extremes and the 10th / 90th percentile are reported.  Beside the time stand two floors computed from the
shape:

    hbm_floor_ms   the bytes of X (n_docs x row_stride floats) over the rate k_lin_score reaches reading the same rows in the same session:
                   --lin-score-ms is that kernel's time from the --profile-pass run (rl_lr_predict on a host copy of the rows; its kernel
                   reads every row once).  Without it the floor uses 6.29 TB/s, the streaming rate measured for this chip, and says so.
    f64_floor_ms   the f64 multiplies and adds, 2 * sum n_l * (n_{l-1} + 1) per document, over 39.3 T operations/s: one wave64
                   v_mul_f64 / v_add_f64 per 4 cycles and SIMD, 4 SIMDs on each of 256 CUs at 2.4 GHz (the issue cost the kernels of this
                   library have been measured against; the activations' exp and divisions are not counted)

and which of the two is nearer to the measured time (the larger one), with the ratio to it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ranklib_amd import _native as N          # noqa: E402  (after torch: one HIP runtime in the process, as bench.py)

F64_OPS_PER_S = 256 * 4 * 64 / 4 * 2.4e9
HBM_STREAM = 6.29e12


def device_rows(n, stride, seed=20240601):
    """bench.py's inference rows: the column kinds of ranklib_amd.synth (feature id f = column f), generated on the device"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    dX = torch.empty((n, stride), dtype=torch.float32, device="cuda")
    chunk = 1 << 20
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        u = torch.rand((b - a, stride), generator=gen, device="cuda")
        k = torch.arange(stride, device="cuda") % 4
        cnt = torch.floor(u * 21.0)
        heavy = torch.exp(4.0 * u)
        sparse = torch.where(torch.rand((b - a, stride), generator=gen, device="cuda") < 0.7, torch.zeros_like(u), u)
        dX[a:b] = torch.where(k == 1, cnt, torch.where(k == 2, u, torch.where(k == 3, heavy, sparse)))
        dX[a:b, 0] = 0
    return dX


def make_net(F, hidden, rng):
    dims = [F] + hidden + [1]
    w = np.concatenate([rng.standard_normal(dims[l] * (dims[l - 1] + 1)) * (0.5 / np.sqrt(dims[l - 1] * 8.0)) for l in range(1, len(dims))])
    return N.NetModel(list(range(1, F + 1)), hidden, w), dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=3_770_000)
    ap.add_argument("--features", type=int, default=136)
    ap.add_argument("--hidden", default=";10", help="networks separated by ';', each a comma-separated list of hidden sizes ('' = none)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--lin-score-ms", type=float, default=0.0, help="k_lin_score's time on the same rows (from the --profile-pass run)")
    ap.add_argument("--profile-pass", action="store_true", help="few launches and one rl_lr_predict on the same rows, for rocprofv3")
    a = ap.parse_args()
    if not a.profile_pass and a.repeats < 20:
        ap.error("--repeats must be at least 20")
    torch.cuda.init()
    n, F, stride = a.docs, a.features, a.features + 1
    dX = device_rows(n, stride)
    dO = torch.empty(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    bytes_x = n * stride * 4
    rate, src = (bytes_x / (a.lin_score_ms * 1e-3), "k_lin_score on the same rows") if a.lin_score_ms > 0 else (HBM_STREAM, "6.29 TB/s, not k_lin_score")
    if a.profile_pass:                 # k_lin_score<false, true> over every row once: 136 terms and the bias
        rows = dX.cpu().numpy()
        N.lr_predict(list(range(1, F + 1)), rng.standard_normal(F + 1), rows)
        del rows
    for spec in a.hidden.split(";"):
        hidden = [int(v) for v in spec.split(",") if v.strip()]
        m, dims = make_net(F, hidden, rng)
        for _ in range(a.warmup):
            m.predict_device(dX.data_ptr(), n, stride, dO.data_ptr())
        torch.cuda.synchronize()
        ms = []
        for _ in range(3 if a.profile_pass else a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.predict_device(dX.data_ptr(), n, stride, dO.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.sort(np.array(ms))
        ops = 2 * sum(dims[l] * (dims[l - 1] + 1) for l in range(1, len(dims)))
        hbm_ms, f64_ms = bytes_x / rate * 1e3, n * ops / F64_OPS_PER_S * 1e3
        near = "hbm" if hbm_ms >= f64_ms else "f64"
        med = float(np.median(ms))
        out = dict(shape="%d x %d" % (n, F), row_stride=stride, hidden=hidden, variant={1: "lds", 2: "global"}[m.path()],
                   repeats=len(ms), ms_median=round(med, 4), ms_min=round(float(ms[0]), 4), ms_max=round(float(ms[-1]), 4),
                   ms_p10=round(float(np.percentile(ms, 10)), 4), ms_p90=round(float(np.percentile(ms, 90)), 4),
                   docs_per_s=round(n / (med * 1e-3)), bytes_x=bytes_x, hbm_rate_tb_s=round(rate / 1e12, 3), hbm_rate_source=src,
                   hbm_floor_ms=round(hbm_ms, 4), f64_ops_per_doc=ops, f64_floor_ms=round(f64_ms, 4), nearer_floor=near,
                   times_nearer_floor=round(med / max(hbm_ms, f64_ms), 2), score_mean=float(dO.mean().item()), profile_pass=a.profile_pass)
        print(json.dumps(out), flush=True)
        m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
