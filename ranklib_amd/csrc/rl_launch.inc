// rl_launch.inc -- the two launchers that choose a kernel instantiation from the shape of the data: launch_rank (K1's ranking and K8's per-query
// metric, MergeSorter.java:134-189 / LambdaMART.java:442-483; the k_rank_* kernels of rl_k_rank.inc) and launch_hist<ROOT> (K2/K3,
// FeatureHistogram.java:126-146,166-195; the k_hist instantiations of rl_k_hist.inc).  Included by rl_trainer.hip behind `struct rl_trainer` and
// `struct DataSet`; needs them, Ctx, Knobs and RL_HIP.  Both count what they launched in RL_ARR_LAUNCH_ARMS (include/rlhip.h).
//
// launch_rank: the tiny lists (k_rank_tiny) first; then k_rank_mixed for wave-sized and block-sized lists in one launch, unless the rank_split
// knob is set or one of the two classes is empty, in which case k_rank_wave (long lists, then short ones) and k_rank_block; k_rank_huge last.
//
// launch_hist looks for an arm in this order, the order of the RL_HARM_* values, and launches the first that fits:
//   1. child pass from compact rows (sparse data)                                      RL_HARM_COMPACT
//   2. child pass, a group's features spread over 16 / sub_child blocks of 256 threads RL_HARM_SUB8 | RL_HARM_SUB4
//   3. child pass, blocks wider than kThreads (hist_nt)                                RL_HARM_NT1024 | RL_HARM_NT512
//   4. root pass that quantises the lambdas itself (fq)                                RL_HARM_FQ_PACKED | RL_HARM_FQ_ROWS16
//   5. 16 features a block and at most kHistLdsStride bins a feature: packed or 16-bit rows, with or without run folding
//                                                                                      RL_HARM_PACKED_RUNS | _PACKED | RL_HARM_ROWS16_RUNS | _ROWS16
//   6. everything else: the LDS row stride known at run time only, by features a block RL_HARM_STRIDE
// 1 .. 4 also require 16 features a block, at most kHistLdsStride bins a feature and no run folding; 2 and 3 no packed child rows (p8 > 1).

namespace rl {

// ---- per-query kernels on a data set -------------------------------------------------------------
// rank every query by `scores` (stable, descending) and leave NDCG@k per query in `out`; with `ranked` the
// ranked-order arrays of the data set are refreshed too (they feed the next round's lambdas)
static int launch_rank(rl_trainer *t, DataSet &d, const double *scores, double *out, bool ranked)
{
    RankArgs a{scores, d.d_labels, d.d_qoff, d.d_ideal1, t->ctx.disc,
               ranked ? d.d_ss : nullptr, ranked ? d.d_sl : nullptr, ranked ? d.d_srel : nullptr, ranked ? d.d_sidx : nullptr,
               out, t->p.metric_k, t->p.metric, ranked ? d.d_aux_i : nullptr, ranked ? d.d_aux_a : nullptr, ranked ? d.d_aux_b : nullptr, t->err_max,
               d.d_ext_rd};
    if (d.n_tiny > 0) {
        t->arms[RL_ARM_RANK_TINY]++;
        hipLaunchKernelGGL(k_rank_tiny, dim3((d.n_tiny + kRankTinyGroups - 1) / kRankTinyGroups), dim3(kRankTinyDocs * kRankTinyGroups), 0, t->stream, a,
                           (const int *)d.d_qtiny, d.n_tiny);
    }
    if (!t->knobs.rank_split && d.n_big > 0 && d.n_small > 0) {
        const int wpb = kRankBlockThreads / 64;
        const size_t lds = std::max((size_t)d.max_big, (size_t)wpb * kLambdaWaveCap) * kRankLdsPerDoc;
        t->arms[RL_ARM_RANK_MIXED]++; t->arms[RL_ARM_RANK_HUGE] += d.n_huge > 0 ? 1 : 0;
        hipLaunchKernelGGL(k_rank_mixed, dim3(d.n_big + (d.n_small + wpb - 1) / wpb), dim3(kRankBlockThreads), lds, t->stream, a, (const int *)d.d_qbig, d.n_big, d.max_big,
                           (const int *)d.d_qsmall, d.n_small, kLambdaWaveCap);
        if (d.n_huge > 0)
            hipLaunchKernelGGL(k_rank_huge, dim3(d.n_huge), dim3(kRankBlockThreads), 0, t->stream, a, (const int *)d.d_qhuge, d.n_huge, d.d_relscratch);
        RL_HIP(hipGetLastError());
        return RL_OK;
    }
    t->arms[RL_ARM_RANK_WAVE_LONG] += d.n_small_long > 0 ? 1 : 0; t->arms[RL_ARM_RANK_WAVE_SHORT] += d.n_small > d.n_small_long ? 1 : 0;
    t->arms[RL_ARM_RANK_BLOCK] += d.n_big > 0 ? 1 : 0; t->arms[RL_ARM_RANK_HUGE] += d.n_huge > 0 ? 1 : 0;
    if (d.n_small_long > 0)       // (d_qsmall: longest first)
        hipLaunchKernelGGL(k_rank_wave, dim3((d.n_small_long + 3) / 4), dim3(kThreads), 4 * kLambdaWaveCap * kRankLdsPerDoc, t->stream, a,
                           (const int *)d.d_qsmall, d.n_small_long, kLambdaWaveCap);
    if (d.n_small > d.n_small_long)
        hipLaunchKernelGGL(k_rank_wave, dim3((d.n_small - d.n_small_long + 3) / 4), dim3(kThreads), 4 * kRankShort * kRankLdsPerDoc, t->stream, a,
                           (const int *)d.d_qsmall + d.n_small_long, d.n_small - d.n_small_long, kRankShort);
    if (d.n_big > 0)
        hipLaunchKernelGGL(k_rank_block, dim3(d.n_big), dim3(kRankBlockThreads), (size_t)d.max_big * kRankLdsPerDoc, t->stream, a, d.d_qbig, d.n_big, d.max_big);
    if (d.n_huge > 0)
        hipLaunchKernelGGL(k_rank_huge, dim3(d.n_huge), dim3(kRankBlockThreads), 0, t->stream, a, (const int *)d.d_qhuge, d.n_huge, d.d_relscratch);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

template <bool ROOT>
static void launch_hist(const Ctx &c, const Knobs &kn, int64_t *arms, int gx, int gy, size_t lds, hipStream_t s, bool fq = false)
{
    // RL_ARR_LAUNCH_ARMS: one increment per launch, root and child passes apart; of a child pass also the grid and the LDS it was given
    const auto took = [&](int arm, const dim3 &grid, size_t lds_bytes) {
        arms[(ROOT ? RL_ARM_HIST_ROOT : RL_ARM_HIST_CHILD) + arm]++;
        if (!ROOT) { arms[RL_ARM_CHILD_GRID_X] = grid.x; arms[RL_ARM_CHILD_GRID_Y] = grid.y; arms[RL_ARM_CHILD_LDS] = (int64_t)lds_bytes; }
    };
    // the XCD-aware block map of k_hist wants a multiple of 8 chunks (the extra blocks exit); child passes: a bounded grid whose blocks walk the
    // step's chunks (k_hist), about one resident set of blocks (3 per CU)
    const int grid_blocks = kn.hist_grid.or_else(1024);
    // (balanced steps -- balance_slots -- want exactly balance_target rows: block row r then works through the chunks r, r + balance_target, ..)
    const bool grid_env = kn.hist_grid.set;
    const auto bounded = [&](int gxx) { return ROOT ? ((gy + 7) & ~7) : (c.balance && (!c.sharded || c.cum_cnt_loc) && !grid_env) ? std::min((gy + 7) & ~7, c.balance_target)
                                                                      : std::min((gy + 7) & ~7, std::max(8, ((grid_blocks + gxx - 1) / gxx + 7) & ~7)); };
    if (!ROOT) lds += kn.hist_ldspad;
    const dim3 g(gx, bounded(gx)), b(kThreads);
    if (!ROOT && c.crows && c.sub == 16 && c.TS <= kHistLdsStride && !c.any_runs) {      // sparse data: compact rows (k_compact_rows)
        took(RL_HARM_COMPACT, g, lds);
        hipLaunchKernelGGL((k_hist<false, 16, kHistLdsStride, false, false, kThreads, true>), g, b, lds, s, c);
        return;
    }
    if (!ROOT && c.sub == 16 && c.TS <= kHistLdsStride && !c.any_runs && !(c.p8 > 1) && c.sub_child < 16) {
        // child passes, features of a group spread over 16 / sub_child blocks: a step of a few chunks leaves most CUs idle while every block is bound by
        // the LDS atomics of ITS CU -- the same atomics on more CUs (the rows are read once per sub-block, from L2)
        const dim3 g2(gx * (16 / c.sub_child), bounded(gx * (16 / c.sub_child)));
        const size_t lds2 = (size_t)c.sub_child * kHistLdsStride * 12;
        took(c.sub_child == 8 ? RL_HARM_SUB8 : RL_HARM_SUB4, g2, lds2);
        if (c.sub_child == 8) hipLaunchKernelGGL((k_hist<false, 8, kHistLdsStride, false, false, 256>), g2, dim3(256), lds2, s, c);
        else hipLaunchKernelGGL((k_hist<false, 4, kHistLdsStride, false, false, 256>), g2, dim3(256), lds2, s, c);
        return;
    }
    if (!ROOT && c.sub == 16 && c.TS <= kHistLdsStride && !c.any_runs && !(c.p8 > 1) && c.hist_nt > kThreads) {
        // child passes: a step has few chunks (~12 per node), so the chip is mostly idle and every block is a chain of dependent row gathers --
        // larger blocks keep more of them in flight per chunk
        took(c.hist_nt >= 1024 ? RL_HARM_NT1024 : RL_HARM_NT512, g, lds);
        if (c.hist_nt >= 1024) hipLaunchKernelGGL((k_hist<false, 16, kHistLdsStride, false, false, 1024>), g, dim3(1024), lds, s, c);
        else hipLaunchKernelGGL((k_hist<false, 16, kHistLdsStride, false, false, 512>), g, dim3(512), lds, s, c);
        return;
    }
    if constexpr (ROOT) {
        if (fq && c.sub == 16 && c.TS <= kHistLdsStride && !c.any_runs) {      // root pass that quantises the lambdas itself (root_quant_fused)
            took(c.p8 ? RL_HARM_FQ_PACKED : RL_HARM_FQ_ROWS16, g, lds);
            if (c.p8) hipLaunchKernelGGL((k_hist<true, 16, kHistLdsStride, false, true, kThreads, false, true>), g, b, lds, s, c);
            else hipLaunchKernelGGL((k_hist<true, 16, kHistLdsStride, false, false, kThreads, false, true>), g, b, lds, s, c);
            return;
        }
    }
    if (c.sub == 16 && c.TS <= kHistLdsStride) {
        // packed rows for the root pass only (measured at c2: 43 % fewer bytes buy the root pass 9 % -- it is bound by LDS atomics, not by HBM --
        // and the child passes nothing: their extra bit-field work costs what the two 128-byte lines per document instead of three save)
        took((c.p8 && (ROOT || c.p8 > 1)) ? (c.any_runs ? RL_HARM_PACKED_RUNS : RL_HARM_PACKED) : (c.any_runs ? RL_HARM_ROWS16_RUNS : RL_HARM_ROWS16), g, lds);
        if (c.p8 && (ROOT || c.p8 > 1)) {
            if (c.any_runs) hipLaunchKernelGGL((k_hist<ROOT, 16, kHistLdsStride, true, true>), g, b, lds, s, c);
            else hipLaunchKernelGGL((k_hist<ROOT, 16, kHistLdsStride, false, true>), g, b, lds, s, c);
        } else if (c.any_runs) hipLaunchKernelGGL((k_hist<ROOT, 16, kHistLdsStride, true>), g, b, lds, s, c);
        else hipLaunchKernelGGL((k_hist<ROOT, 16, kHistLdsStride>), g, b, lds, s, c);
        return;
    }
    took(RL_HARM_STRIDE, g, lds);
    switch (c.sub) {
    case 16: hipLaunchKernelGGL((k_hist<ROOT, 16, 0>), g, b, lds, s, c); break;
    case 8: hipLaunchKernelGGL((k_hist<ROOT, 8, 0>), g, b, lds, s, c); break;
    case 4: hipLaunchKernelGGL((k_hist<ROOT, 4, 0>), g, b, lds, s, c); break;
    case 2: hipLaunchKernelGGL((k_hist<ROOT, 2, 0>), g, b, lds, s, c); break;
    default: hipLaunchKernelGGL((k_hist<ROOT, 1, 0>), g, b, lds, s, c); break;
    }
}

}  // namespace rl
