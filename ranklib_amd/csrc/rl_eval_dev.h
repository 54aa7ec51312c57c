// rl_eval_dev.h -- the device code that every kernel ranking and scoring a list shares, whatever translation unit it is built in:
// ca_pow2m1 and ca_sync (k_ca_trials and its kin, rl_ca.hip), the length classes, EvArgs and ev_metric (k_eval_lists, rl_eval.inc;
// k_stage_eval, rl_stage.inc).  The scorers are stated once, here.
#pragma once
#include "rl_internal.h"

namespace rl {

__device__ __forceinline__ int ca_pow2m1(int rel) { return (int)(((unsigned)1 << (rel & 31)) - 1u); }   // DCGScorer.java:137-139, Java int arithmetic

template <int G>
__device__ __forceinline__ void ca_sync()
{
    if (G > kWave) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
}

constexpr int kEvTiny = 16, kEvWave = 256, kEvBlock = 6144;

struct EvArgs {
    const double *sc; const float *labels; const int32_t *qoff; const double *ideal; const int32_t *rd_ext; const double *disc;
    const int32_t *qlist; int32_t nq;                           // the lists of this length class
    float *glab;                                               // longest class: ranked labels, [n_docs] (list q at qoff[q])
    double *out; int32_t *pos;                                  // pos may be null
    int32_t metric, k;
    double err_max;
};

// The scorer's value of one ranked list (lab: its labels in ranked order), by one thread
__device__ inline double ev_metric(const EvArgs &a, int q, int n, const float *lab)
{
    int size = a.k;
    if (a.k > n || a.k <= 0) size = n;
    switch (a.metric) {
    case RL_METRIC_NDCG: {                                  // NDCGScorer.score :103-129
        const double ideal = a.ideal[q];
        if (!(ideal > 0.0)) return 0.0;
        double dcg = 0;
        for (int i = 0; i < size; i++) dcg += (double)ca_pow2m1((int)lab[i]) * a.disc[i];
        return dcg / ideal;
    }
    case RL_METRIC_DCG: {                                   // DCGScorer.score :58-71
        double dcg = 0;
        for (int i = 0; i < size; i++) dcg += (double)ca_pow2m1((int)lab[i]) * a.disc[i];
        return dcg;
    }
    case RL_METRIC_MAP: {                                   // APScorer.score :73-100, the whole list
        double ap = 0.0; int count = 0;
        for (int i = 0; i < n; i++)
            if (lab[i] > 0.f) { count++; ap += ((double)count) / (i + 1); }
        const int rdc = a.rd_ext ? a.rd_ext[q] : count;
        return (rdc == 0) ? 0.0 : ap / rdc;
    }
    case RL_METRIC_ERR: {                                   // ERRScorer.score :45-64
        double s = 0.0, p = 1.0;
        for (int i = 1; i <= size; i++) { const double R = (double)ca_pow2m1((int)lab[i - 1]) / a.err_max; s += p * R / i; p *= (1.0 - R); }
        return s;
    }
    case RL_METRIC_P: {                                     // PrecisionScorer.score :28-40
        int count = 0;
        for (int i = 0; i < size; i++) count += lab[i] > 0.f ? 1 : 0;
        return ((double)count) / size;
    }
    case RL_METRIC_RR: {                                    // ReciprocalRankScorer.score :24-35: (double) (1.0f / firstRank); k = 0 scores 0
        const int rsize = (n > a.k) ? a.k : n;
        for (int i = 0; i < rsize; i++)
            if (lab[i] > 0.f) return (double)(1.0f / (float)(i + 1));
        return 0.0;
    }
    default: {                                              // RL_METRIC_BEST, BestAtKScorer.score :28-56: the first maximum of positions 0 .. size
        int bsize = a.k - 1;
        if (bsize < 0 || bsize > n - 1) bsize = n - 1;
        double mx = -1.0; int mi = 0;
        for (int i = 0; i <= bsize; i++)
            if (mx < (double)lab[i]) { mx = (double)lab[i]; mi = i; }
        return (double)lab[mi];
    }
    }
}

}  // namespace rl
