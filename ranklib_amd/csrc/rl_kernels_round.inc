// rl_kernels_round.inc -- gfx950 kernels of one boosting round (included by rl_trainer.hip): one rl_k_*.inc piece per stage, each a namespace rl
// block of its own, included in dependency order.  This file itself holds only what more than one piece shares: the small helpers below and the
// trace block (kTraceBlocks .. RL_TR_END) between the includes.
//
// K1  k_rank_*                                                  rl_k_rank.inc     MergeSorter.java:134-189
//      per-query stable rank, the metric of that ranking (K8)
//     k_lambda_fused / k_pair_terms + k_lambda_acc / k_lambda_tiny, k_mart_residual, k_max_reduce
//      pairwise swap change x sigmoid                           rl_k_lambda.inc   LambdaMART.java:361-396, MART.java:47-51
// K1b k_quantize        lambda -> order-independent fixed point rl_k_quant.inc    (DESIGN.md 3 "exact sums")
// K2/3 k_hist<ROOT>     LDS-staged per-chunk histograms         rl_k_hist.inc     FeatureHistogram.java:126-146,166-195
// K4/5 k_hist_finish    chunk reduction, prefix over thresholds, sibling = parent - built child, per-feature gain scan
//      rl_k_finish.inc (its helpers and k_hist_reduce: rl_k_reduce.inc; the per-feature best-split exchange: rl_k_best.inc)
//                                                                                 FeatureHistogram.java:141-145,189-194,222-264
//      select_step      (last block of k_hist_finish) best-first growth bookkeeping, speculative slots
//      rl_k_select.inc                                                            RegressionTree.java:58-87,147-157
// K6  k_part_scatter<LOOKBACK> (+ k_part_count when sharded)  stable partition    FeatureHistogram.java:328-341
//      rl_k_partition.inc
// K7  k_leaf_table, k_leaf_output, k_score_update (+ rl_chain.inc)   rl_k_leaf.inc   LambdaMART.java:398-415, 203-210
// K8  per-query metric in k_rank_* (rl_k_rank.inc), float mean via rl_chain.inc / k_float_mean (rl_k_leaf.inc)   LambdaMART.java:442-483
// K10 k_ensemble_eval, k_valid_update (k_model_eval* live in rl_model_eval.inc)   rl_k_ensemble.inc   Ensemble.java:110-116, Split.java:115-125

namespace rl {

// ------------------------------------------------------------------------------------------------
// small helpers: 128-bit integers in halves and across lanes (the growth step; rl_step2.inc and rl_tie.inc behind this file), the Java's gain 2^label - 1 (rank, lambdas)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ i128 shfl_up_i128(i128 v, int d)
{
    uint32_t w0 = (uint32_t)(u128)v, w1 = (uint32_t)((u128)v >> 32), w2 = (uint32_t)((u128)v >> 64),
             w3 = (uint32_t)((u128)v >> 96);
    w0 = __shfl_up(w0, d); w1 = __shfl_up(w1, d); w2 = __shfl_up(w2, d); w3 = __shfl_up(w3, d);
    return (i128)(((u128)w3 << 96) | ((u128)w2 << 64) | ((u128)w1 << 32) | (u128)w0);
}

__device__ __forceinline__ i128 make_i128(long long hi, unsigned long long lo) { return (i128)(((u128)(unsigned long long)hi << 64) | (u128)lo); }
__device__ __forceinline__ long long hi_of(i128 v) { return (long long)(v >> 64); }
__device__ __forceinline__ unsigned long long lo_of(i128 v) { return (unsigned long long)(u128)v; }

// DCGScorer.java:28-31,137-139: (1 << i) - 1 in Java int arithmetic -- the shift count is taken mod 32 and the subtraction wraps, so labels
// above 30 give 2^31 - 1 (31), 0 (32), 1 (33), ..: reproduced, not rejected
__device__ __forceinline__ int java_pow2m1(int rel) { return (int)(((unsigned)1 << (rel & 31)) - 1u); }
__device__ __forceinline__ double gain_of(int rel) { return (double)java_pow2m1(rel); }

}  // namespace rl

// K1 and K1b: what a round does before its tree grows
#include "rl_k_rank.inc"
#include "rl_k_lambda.inc"
#include "rl_k_quant.inc"

namespace rl {

// Block-level timeline of the growth steps of ONE tree (builds with -DRL_PHASE_CLOCKS, tools/step_trace.py): every working block of the partition
// (kernel 0), child-histogram (1) and finish (2) kernels stores its entry / exit wall-clock stamps at trace[step][kernel][block] -- plain stores to
// distinct addresses (folding them with atomics on a few words made the measurement the bottleneck).  Ctx::trace_tree selects the tree.
constexpr int kTraceBlocks = 2048, kTraceStamps = 8;
#ifdef RL_PHASE_CLOCKS
// a stamp that cannot move: every memory operation the wavefront has issued is complete when the clock is read, and nothing later starts before it
__device__ __forceinline__ long long strict_clock()
{
    unsigned long long t;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    return (long long)t;
}
// where the block runs: HW_ID (wave / SIMD / CU / SH / SE fields) and the XCD number, kept in stamp 6 (no kernel uses it as a time; tools/block_place.py)
__device__ __forceinline__ long long hw_place()
{
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return (long long)(((unsigned long long)(xcc & 0xfu) << 32) | hw);
}
#define RL_TR_BEGIN() long long tr_t_[kTraceStamps] = {0, 0, 0, 0, 0, 0, 0, 0}; tr_t_[0] = strict_clock(); tr_t_[6] = hw_place()
#define RL_TR_MARK(k) do { tr_t_[k] = strict_clock(); } while (0)
#define RL_TR_END(kern, idx) do { if (threadIdx.x == 0 && c.trace && c.st->tree_seq == c.trace_tree && (int)(idx) < kTraceBlocks) { \
        long long *o_ = c.trace + ((((size_t)(c.st->step & 63) * 3 + (kern)) * kTraceBlocks + (size_t)(idx)) * kTraceStamps); \
        tr_t_[kTraceStamps - 1] = strict_clock(); \
        for (int q_ = 0; q_ < kTraceStamps; q_++) o_[q_] = tr_t_[q_]; } } while (0)
#else
#define RL_TR_BEGIN() do { } while (0)
#define RL_TR_MARK(k) do { } while (0)
#define RL_TR_END(kern, idx) do { } while (0)
#endif

}  // namespace rl

// K2/K3, then the growth step of a tree (K4/K5 and K6), then what ends the round (K7, K8, K10)
#include "rl_k_hist.inc"
#include "rl_k_reduce.inc"
#include "rl_k_best.inc"
#include "rl_k_select.inc"
#include "rl_k_finish.inc"
#include "rl_k_partition.inc"
#include "rl_k_leaf.inc"
#include "rl_k_ensemble.inc"
