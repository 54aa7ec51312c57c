// rl_ca.hip -- Coordinate Ascent (-ranker 4, learning/CoorAscent.java) on gfx950.
//
// The Java's training loop is thousands of `scorer.score(rank(samples))` evaluations.  Every trial of one search direction depends only
// on the cached scores at the start of the direction, the feature's column and the step list (CoorAscent.java:127-149: all
// nMaxIteration trials run, only the sign loop breaks), so a direction is ONE pass here:
//
//   k_ca_trials<G, PER>  a group of G threads owns one (list, chunk of trials): it rebuilds the Java's chain of cached-score updates
//                        ((c0 + s0 x) + s1 x) + ... in registers, ranks the list by counting after every trial (stable, descending:
//                        MergeSorter.sort(double[], false)) and writes the list's metric of every trial, m[q][t].  The group that holds a
//                        direction's last trial writes the chain's final value: the cache the Java leaves behind.  The last block to
//                        finish sums every trial's metrics in list order (MetricScorer.java:47-52: f64, serial) -> sums[t] / Q.
//                        Length classes: <= 16 documents (G = 16, 16 lists per block), <= 384 (one wavefront), <= 5000 (one block,
//                        LDS), longer (one block, global scratch).
//   k_ca_apply           cached = cached + wc * x, then optionally cached = cached / sum (updateCached / scaleCached :315-335)
//   k_lin_score          cached = 0.0 + w[0] x0 + w[1] x1 + ...  (rank() with current_feature == -1, :207-213; also CoorAscent.eval): the
//                        scoring kernel of all four linear rankers (rl_linear.inc)
//
// The host side runs CoorAscent.learn() (:67-202) literally: weights, the keep / restore decisions, the -reg penalty and the shuffle.
// Built with -ffp-contract=off like the rest of the library: no fused multiply-adds, plain IEEE divisions.  There is no CPU fallback.
//
// The sets on the device, the scorer's tables, the stream and the entry points' common bodies are the ranking context's (LinCtx,
// rl_linear.inc), which AdaRank, RankBoost and Linear Regression (included at the end of this file) use as well; k_ca_trials ranks for all.
#include "rl_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>

#include "rl_lists_host.h" // the host side of a set of ranked lists: list rules, ideal DCGs (no HIP in it)
#include "rl_linear.inc"   // LinCtx and everything the four linear rankers share
#include "rl_eval_dev.h"   // ca_pow2m1, ca_sync and the scorers of k_eval_lists: shared with the tree models' unit (rl_stage.inc)

namespace rl {

constexpr int kCaStage = 2048;        // doubles of LDS the last block stages the per-list metrics through (32 rows of kCaSteps trials)

struct CaArgs {
    const double *cache; double *cache_out; const float *x;    // x: the direction's column [N] (null when no step is applied)
    const float *labels; const int32_t *qoff; const double *ideal; const int32_t *rd_ext; const double *disc;
    const int32_t *qlist; int32_t nq;                           // the lists of this length class
    double *hsc; int32_t *hrel; const int64_t *hoff; int64_t nh;   // longest class: per chunk, global scratch at hoff[slot]
    double *m; double *sums; uint32_t *done; int32_t blocks_total;
    int32_t Q, T, first, tchunk, nchunk, metric, k;
    double err_max;
    double steps[kCaSteps];
};

// ca_pow2m1 and ca_sync: rl_eval_dev.h

// rel view of the labels: (int)label for NDCG / DCG / ERR, label > 0 for MAP / P / RR
__device__ __forceinline__ int ca_rel(const CaArgs &a, float l)
{
    return (a.metric == RL_METRIC_MAP || a.metric == RL_METRIC_P || a.metric == RL_METRIC_RR) ? (l > 0.f ? 1 : 0) : (int)l;
}

// The scorer's value of one ranked list, by one thread (metric/{NDCG,DCG,AP,ERR,Precision,ReciprocalRank}Scorer.java)
__device__ double ca_metric(const CaArgs &a, int q, int n, const int *rel)
{
    int size = a.k;
    if (a.k > n || a.k <= 0) size = n;
    if (a.metric == RL_METRIC_NDCG) {                       // NDCGScorer.score :103-129
        const double ideal = a.ideal[q];
        if (!(ideal > 0.0)) return 0.0;
        double dcg = 0;
        for (int i = 0; i < size; i++) dcg += (double)ca_pow2m1(rel[i]) * a.disc[i];
        return dcg / ideal;
    }
    if (a.metric == RL_METRIC_DCG) {                        // DCGScorer.score :58-71
        double dcg = 0;
        for (int i = 0; i < size; i++) dcg += (double)ca_pow2m1(rel[i]) * a.disc[i];
        return dcg;
    }
    if (a.metric == RL_METRIC_MAP) {                        // APScorer.score :73-100
        double ap = 0.0; int count = 0;
        for (int i = 0; i < n; i++)
            if (rel[i]) { count++; ap += ((double)count) / (i + 1); }
        const int rdc = a.rd_ext ? a.rd_ext[q] : count;
        return (rdc == 0) ? 0.0 : ap / rdc;
    }
    if (a.metric == RL_METRIC_ERR) {                        // ERRScorer.score :45-64
        double sc = 0.0, p = 1.0;
        for (int i = 1; i <= size; i++) { const double R = (double)ca_pow2m1(rel[i - 1]) / a.err_max; sc += p * R / i; p *= (1.0 - R); }
        return sc;
    }
    if (a.metric == RL_METRIC_P) {                          // PrecisionScorer.score :28-40
        int count = 0;
        for (int i = 0; i < size; i++) count += rel[i];
        return ((double)count) / size;
    }
    const int rsize = (n > a.k) ? a.k : n;                  // ReciprocalRankScorer.score :24-35: (double) (1.0f / firstRank)
    for (int i = 0; i < rsize; i++)
        if (rel[i]) return (double)(1.0f / (float)(i + 1));
    return 0.0;
}

// the last block of a direction: every trial's list-order f64 sum / Q.  The metrics are staged through LDS in coalesced rounds (stage:
// the kernel's own LDS, cap doubles), then lane t adds row after row of column t: the Java's serial chain, its loads already on chip.
__device__ void ca_finish(const CaArgs &a, double *stage, int cap)
{
    __shared__ int s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const uint32_t prev = atomicAdd(a.done, 1u);
        s_last = (prev == (uint32_t)a.blocks_total - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const int T = a.T, rows = cap / T, tid = threadIdx.x;
    double s = 0.0;
    for (int q0 = 0; q0 < a.Q; q0 += rows) {
        const int nr = min(rows, a.Q - q0);
        for (int e = tid; e < nr * T; e += blockDim.x) stage[e] = a.m[(size_t)q0 * T + e];
        __syncthreads();
        if (tid < T) {
#pragma unroll 16
            for (int r = 0; r < nr; r++) s += stage[r * T + tid];
        }
        __syncthreads();
    }
    if (tid < T) a.sums[tid] = s / a.Q;
    if (tid == 0) atomicExch(a.done, 0u);                   // ready for the next direction
}

// PER > 0: a group keeps its list (<= G * PER documents) in registers and LDS; PER == 0: global scratch (any length)
template <int G, int PER>
__device__ void ca_group(const CaArgs &a, int slot, int chunk, int tid, double *s_sc, int *s_rel)
{
    const int q = a.qlist[slot];
    const int cur = a.qoff[q], n = a.qoff[q + 1] - cur;
    const int t0 = chunk * a.tchunk, t1 = min(a.T, t0 + a.tchunk);
    int applied = 0;
    if (PER > 0) {
        double c[PER > 0 ? PER : 1]; float x[PER > 0 ? PER : 1]; int rv[PER > 0 ? PER : 1];
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int i = tid + u * G;
            c[u] = 0.0; x[u] = 0.f; rv[u] = 0;
            if (i < n) { c[u] = a.cache[cur + i]; if (a.x) x[u] = a.x[cur + i]; rv[u] = ca_rel(a, a.labels[cur + i]); }
        }
        for (int t = t0; t < t1; t++) {
            for (; applied < t + a.first; applied++) {
                const double s = a.steps[applied];
#pragma unroll
                for (int u = 0; u < PER; u++) c[u] = c[u] + s * (double)x[u];
            }
#pragma unroll
            for (int u = 0; u < PER; u++) { const int i = tid + u * G; if (i < n) s_sc[i] = c[u]; }
            ca_sync<G>();
#pragma unroll
            for (int u = 0; u < PER; u++) {
                const int i = tid + u * G;
                if (i < n) {
                    const double v = c[u];
                    int p = 0;
                    for (int j = 0; j < n; j++) { const double y = s_sc[j]; p += ((y > v) || (y == v && j < i)) ? 1 : 0; }
                    s_rel[p] = rv[u];
                }
            }
            ca_sync<G>();
            if (tid == 0) a.m[(size_t)q * a.T + t] = ca_metric(a, q, n, s_rel);
        }
        if (t1 == a.T && a.first) {
#pragma unroll
            for (int u = 0; u < PER; u++) { const int i = tid + u * G; if (i < n) a.cache_out[cur + i] = c[u]; }
        }
        ca_sync<G>();          // the next list of this group reuses the LDS
    } else {
        double *sc = a.hsc + (size_t)chunk * a.nh + a.hoff[slot];
        int *rel = a.hrel + (size_t)chunk * a.nh + a.hoff[slot];
        for (int i = tid; i < n; i += G) sc[i] = a.cache[cur + i];
        for (int t = t0; t < t1; t++) {
            for (; applied < t + a.first; applied++) {
                const double s = a.steps[applied];
                for (int i = tid; i < n; i += G) sc[i] = sc[i] + s * (double)a.x[cur + i];
            }
            __syncthreads();
            for (int i = tid; i < n; i += G) {
                const double v = sc[i];
                int p = 0;
                for (int j = 0; j < n; j++) { const double y = sc[j]; p += ((y > v) || (y == v && j < i)) ? 1 : 0; }
                rel[p] = ca_rel(a, a.labels[cur + i]);
            }
            __syncthreads();
            if (tid == 0) a.m[(size_t)q * a.T + t] = ca_metric(a, q, n, rel);
            __syncthreads();
        }
        if (t1 == a.T && a.first)
            for (int i = tid; i < n; i += G) a.cache_out[cur + i] = sc[i];
        __syncthreads();
    }
}

template <int G, int CAP>
__global__ __launch_bounds__(kThreads) void k_ca_trials(const CaArgs a)
{
    constexpr int GPB = kThreads / G;                 // groups per block
    constexpr int PER = CAP > 0 ? (CAP + G - 1) / G : 0;
    constexpr int LDS = CAP > 0 ? CAP : 1;
    constexpr int SC = GPB * LDS > kCaStage ? GPB * LDS : kCaStage;      // the groups' scores, then ca_finish's staging area
    __shared__ double s_sc[SC];
    __shared__ int s_rel[GPB][LDS];
    const int grp = threadIdx.x / G, tid = threadIdx.x % G;
    const int64_t g = (int64_t)blockIdx.x * GPB + grp;
    if (g < (int64_t)a.nq * a.nchunk) {
        const int slot = (int)(g % a.nq), chunk = (int)(g / a.nq);
        ca_group<G, PER>(a, slot, chunk, tid, s_sc + grp * LDS, s_rel[grp]);
    }
    ca_finish(a, s_sc, SC);
}

__global__ void k_ca_apply(double *cache, const float *x, int64_t n, double wc, int scale, double sum)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = cache[i] + wc * (double)x[i];
    if (scale) v = v / sum;
    cache[i] = v;
}

}  // namespace rl

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------

using namespace rl;

struct rl_ca {
    rl_ca_params p;
    LinCtx ctx;
    std::vector<double> weight;
    std::vector<rl_ca_trace_rec> trace;
};

namespace rl {

// java.util.Random (the javadoc's LCG) and Collections.shuffle (java/util/Collections.java: for i = size; i > 1; i--: swap(i-1, nextInt(i)))
struct JavaRandom {
    uint64_t seed;
    explicit JavaRandom(int64_t s) : seed(((uint64_t)s ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1)) {}
    int32_t next(int bits)
    {
        seed = (seed * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int32_t)(int64_t)(seed >> (48 - bits));
    }
    int32_t nextInt(int32_t bound)
    {
        int32_t r = next(31);
        const int32_t m = bound - 1;
        if ((bound & m) == 0) return (int32_t)(((int64_t)bound * (int64_t)r) >> 31);
        for (int32_t u = r; (int32_t)((uint32_t)u - (uint32_t)(r = u % bound) + (uint32_t)m) < 0; u = next(31)) {}
        return r;
    }
};

// Evaluates trials [0, T) of one direction on set d (steps[t] = the weight change of trial t; first = 0: T == 1, the cache as it is) and
// copies sums[0..T) (= scorer.score(rank(samples)) after each trial) into out.  first = 1 leaves the chain's final value in d.d_cache.
static int ca_trials(LinCtx *c, CaSet &d, const float *xcol, const double *steps, int T, int first, double *out)
{
    CaArgs a;
    memset(&a, 0, sizeof(a));
    a.cache = d.d_cache; a.cache_out = d.d_cache2; a.x = xcol;
    a.labels = d.d_labels; a.qoff = d.d_qoff; a.ideal = d.d_ideal; a.rd_ext = d.d_rd; a.disc = c->d_disc;
    a.m = c->d_m; a.sums = c->d_sums; a.done = c->d_done;
    a.Q = d.Q; a.T = T; a.first = first; a.metric = c->metric; a.k = c->metric_k; a.err_max = c->err_max;
    for (int t = 0; t < T; t++) a.steps[t] = steps ? steps[t] : 0.0;
    static const int G[4] = {kCaTiny, kWave, kThreads, kThreads};
    // a group per (list, chunk of trials): few lists get the trial dimension spread over more groups (~2048 wavefronts of work)
    int grid[4] = {0, 0, 0, 0}, tchunk[4], nchunk[4], total = 0;
    for (int k = 0; k < 4; k++) {
        const CaClass &cl = d.cls[k];
        if (!cl.nq) continue;
        const int64_t target = (int64_t)2048 * kWave / G[k];
        int nc = (int)std::min<int64_t>(T, std::max<int64_t>(1, (target + cl.nq - 1) / cl.nq));
        if (k == 3) nc = std::min(nc, d.hchunks);
        tchunk[k] = (T + nc - 1) / nc;
        nchunk[k] = (T + tchunk[k] - 1) / tchunk[k];
        const int gpb = kThreads / G[k];
        grid[k] = (int)(((int64_t)cl.nq * nchunk[k] + gpb - 1) / gpb);
        total += grid[k];
    }
    a.blocks_total = total;
    for (int k = 0; k < 4; k++) {
        if (!grid[k]) continue;
        const CaClass &cl = d.cls[k];
        a.qlist = cl.d_qlist; a.nq = cl.nq; a.tchunk = tchunk[k]; a.nchunk = nchunk[k];
        a.hsc = d.d_hsc; a.hrel = d.d_hrel; a.hoff = cl.d_hoff; a.nh = cl.nh;
        if (k == 0) hipLaunchKernelGGL((k_ca_trials<kCaTiny, kCaTiny>), dim3(grid[k]), dim3(kThreads), 0, c->stream, a);
        else if (k == 1) hipLaunchKernelGGL((k_ca_trials<kWave, kCaWave>), dim3(grid[k]), dim3(kThreads), 0, c->stream, a);
        else if (k == 2) hipLaunchKernelGGL((k_ca_trials<kThreads, kCaBlock>), dim3(grid[k]), dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL((k_ca_trials<kThreads, 0>), dim3(grid[k]), dim3(kThreads), 0, c->stream, a);
        RL_HIP(hipGetLastError());
    }
    RL_HIP(hipMemcpyAsync(c->h_sums, c->d_sums, T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RL_HIP(hipStreamSynchronize(c->stream));
    for (int t = 0; t < T; t++) out[t] = c->h_sums[t];
    if (first) std::swap(d.d_cache, d.d_cache2);
    return RL_OK;
}

// all trials of one direction (in launches of up to kCaSteps trials: each continues the previous one's chain)
static int ca_direction(LinCtx *c, int f, const std::vector<double> &steps, std::vector<double> &scores)
{
    const int T = (int)steps.size();
    scores.resize(T);
    const float *x = c->tr.d_xc + (size_t)f * c->tr.N;
    for (int t0 = 0; t0 < T; t0 += kCaSteps) {
        const int n = std::min(kCaSteps, T - t0);
        int rc = ca_trials(c, c->tr, x, steps.data() + t0, n, 1, scores.data() + t0);
        if (rc) return rc;
    }
    return RL_OK;
}

static int ca_apply(LinCtx *c, int f, double wc, bool scale, double sum)
{
    CaSet &d = c->tr;
    const int64_t n = d.N;
    hipLaunchKernelGGL(k_ca_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d.d_cache, d.d_xc + (size_t)f * n, n, wc,
                       scale ? 1 : 0, sum);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

static double ca_distance(const std::vector<double> &w1, const std::vector<double> &w2)
{   // CoorAscent.getDistance :350-364
    double s1 = 0.0, s2 = 0.0;
    for (size_t i = 0; i < w1.size(); i++) { s1 += std::fabs(w1[i]); s2 += std::fabs(w2[i]); }
    double dist = 0.0;
    for (size_t i = 0; i < w1.size(); i++) { const double t = w1[i] / s1 - w2[i] / s2; dist += t * t; }
    return std::sqrt(dist);
}

static double ca_normalize(std::vector<double> &w)
{   // CoorAscent.normalize :366-382
    double sum = 0.0;
    for (double v : w) sum += std::fabs(v);
    if (sum > 0) { for (double &v : w) v /= sum; }
    else { sum = 1; for (double &v : w) v = 1.0 / (double)w.size(); }
    return sum;
}

static int ca_learn(rl_ca *h)
{
    LinCtx *c = &h->ctx;
    const rl_ca_params &P = h->p;
    const int F = c->F;
    auto rec = [&](int kind, int r, int f, int dir, int j, int imp, double w, double s) {
        rl_ca_trace_rec t; t.kind = kind; t.restart = r; t.feature = f; t.dir = dir; t.j = j; t.improved = imp; t.weight = w; t.score = s;
        h->trace.push_back(t);
    };
    auto model = [&](const std::vector<double> &w) { LinModel m; m.w = w.data(); m.nt = m.nw = F; return m; };      // column t, weight w[t]
    h->trace.clear();
    std::vector<double> weight((size_t)F), regVector((size_t)F, 1.0 / F);      // init() :62-63, copied at :68-69
    std::vector<double> bestModel; double bestModelScore = 0.0;
    const int sign[3] = {1, -1, 0};
    JavaRandom rnd(P.seed);
    std::vector<double> steps, tw, ts, scores;
    for (int r = 0; r < P.n_restart; r++) {
        int consecutive_fails = 0;
        for (int i = 0; i < F; i++) weight[i] = (double)(1.0f / (float)F);       // :87-89, a float division
        double startScore;
        int rc = lin_score_model(c, c->tr, model(weight), &startScore);
        if (rc) return rc;
        rec(RL_CA_RESTART, r, -1, 0, 0, 0, 0.0, startScore);
        double bestScore = startScore;
        std::vector<double> bestWeight = weight;
        int pass = 0;
        while ((F > 1 && consecutive_fails < F - 1) || (F == 1 && consecutive_fails == 0)) {
            rec(RL_CA_PASS, r, -1, 0, pass++, 0, 0.0, bestScore);
            std::vector<int> fids((size_t)F);
            for (int i = 0; i < F; i++) fids[i] = i;
            for (int i = F; i > 1; i--) std::swap(fids[i - 1], fids[rnd.nextInt(i)]);   // Collections.shuffle(l, rnd)
            for (int i = 0; i < F; i++) {
                const int f = fids[i];
                const double origWeight = weight[f];
                double totalStep = 0, bestTotalStep = 0;
                bool succeeds = false;
                for (int s = 0; s < 3; s++) {
                    const int dir = sign[s];
                    double step = 0.001 * dir;
                    if (origWeight != 0.0 && std::fabs(step) > 0.5 * std::fabs(origWeight)) step = P.step_base * std::fabs(origWeight);
                    totalStep = step;
                    int numIter = P.n_max_iteration;
                    if (dir == 0) { numIter = 1; totalStep = -origWeight; }
                    steps.clear(); tw.clear(); ts.clear();
                    for (int j = 0; j < numIter; j++) {
                        tw.push_back(origWeight + totalStep); steps.push_back(step); ts.push_back(totalStep);
                        if (j < P.n_max_iteration - 1) { step *= P.step_scale; totalStep += step; }
                    }
                    if (numIter > 0) {
                        rc = ca_direction(c, f, steps, scores);
                        if (rc) return rc;
                    }
                    for (int j = 0; j < numIter; j++) {
                        weight[f] = tw[j];
                        double score = scores[j];
                        if (P.regularized) score -= P.slack * ca_distance(weight, regVector);
                        const bool imp = score > bestScore;
                        if (imp) { bestScore = score; bestTotalStep = ts[j]; succeeds = true; }
                        rec(RL_CA_TRIAL, r, f, dir, j, imp ? 1 : 0, tw[j], score);
                    }
                    if (succeeds) break;
                    else if (s < 2) {
                        if ((rc = ca_apply(c, f, -totalStep, false, 0.0))) return rc;
                        weight[f] = origWeight;
                    }
                }
                if (succeeds) {
                    weight[f] = origWeight + bestTotalStep;
                    consecutive_fails = 0;
                    const double sum = ca_normalize(weight);
                    // updateCached() with bestTotalStep - totalStep, then scaleCached(sum): two roundings per document, one launch
                    if ((rc = ca_apply(c, f, bestTotalStep - totalStep, true, sum))) return rc;
                    bestWeight = weight;
                    rec(RL_CA_SUCCESS, r, f, 0, 0, 0, weight[f], bestScore);
                } else {
                    consecutive_fails++;
                    if ((rc = ca_apply(c, f, -totalStep, false, 0.0))) return rc;
                    weight[f] = origWeight;
                }
            }
            if (bestScore - startScore < P.tolerance) break;
        }
        if (c->has_valid) {
            int rc2 = lin_score_model(c, c->va, model(weight), &bestScore);
            if (rc2) return rc2;
            rec(RL_CA_VALID, r, -1, 0, 0, 0, 0.0, bestScore);
        }
        if (bestModel.empty() || bestScore > bestModelScore) { bestModelScore = bestScore; bestModel = bestWeight; }
    }
    h->weight = bestModel;
    return lin_finish(c, model(h->weight));
}

}  // namespace rl

extern "C" {

void rl_ca_params_default(rl_ca_params *p)
{   // learning/CoorAscent.java:37-43
    if (!p) return;
    p->n_restart = 5; p->n_max_iteration = 25; p->step_base = 0.05; p->step_scale = 2.0; p->tolerance = 0.001;
    p->regularized = 0; p->slack = 0.001; p->metric = RL_METRIC_NDCG; p->metric_k = 10; p->device = 0; p->seed = 0;
    p->err_max = 16.0;
}

int rl_ca_create(const rl_ca_params *p, rl_ca **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    if (p->n_restart < 1) return fail(RL_ERR_INVALID, "n_restart must be >= 1 (the Java ends in a NullPointerException)");
    std::unique_ptr<rl_ca> c(new rl_ca());
    c->p = *p;
    int rc = lin_create(&c->ctx, "Coordinate Ascent", p->metric, p->metric_k, p->device, p->err_max);
    if (rc) return rc;
    *out = c.release();
    return RL_OK;
}

void rl_ca_destroy(rl_ca *c) { lin_destroy(c); }

int rl_ca_set_train(rl_ca *c, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                    int32_t n_queries, const int32_t *qkey)
{
    return lin_set_train(lin_ctx(c), "rl_ca_", X, n_docs, n_features, labels, qoff, n_queries, qkey);
}

int rl_ca_set_validation(rl_ca *c, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                         const int32_t *qkey)
{
    return lin_set_validation(lin_ctx(c), "rl_ca_", X, n_docs, labels, qoff, n_queries, qkey);
}

int rl_ca_set_external_judgments(rl_ca *c, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    return lin_set_external_judgments(lin_ctx(c), "rl_ca_", validation, ideal_dcg, rel_doc_count);
}

int rl_ca_learn(rl_ca *c)
{
    int rc = lin_begin_learn(lin_ctx(c), "rl_ca_");
    if (rc) return rc;
    if ((rc = ca_prepare(&c->ctx))) return rc;
    return ca_learn(c);
}

int rl_ca_get_weights(const rl_ca *c, double *w, int32_t cap)
{
    if (!c || !w) return fail(RL_ERR_INVALID, "null argument");
    if (!c->ctx.learned) return fail(RL_ERR_STATE, "rl_ca_learn has not run");
    if (cap < c->ctx.F) return fail(RL_ERR_INVALID, "weight buffer too small");
    std::copy(c->weight.begin(), c->weight.end(), w);
    return RL_OK;
}

int rl_ca_scores(const rl_ca *c, double *train, double *valid) { return lin_scores(lin_ctx(c), "rl_ca_", train, valid); }

int rl_ca_trace(const rl_ca *c, rl_ca_trace_rec *out, int64_t cap, int64_t *n) { return lin_trace(c ? &c->trace : nullptr, out, cap, n); }

int rl_ca_predict(int32_t device, const int32_t *feature_ids, const double *weights, int32_t n_weights, const float *X, int64_t n_docs,
                  int32_t row_stride, double *out)
{
    if (!feature_ids || !weights || !out || (n_docs > 0 && !X)) return fail(RL_ERR_INVALID, "null argument");
    if (n_weights < 0 || n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad sizes");
    LinModel m;
    m.col = feature_ids; m.w = weights; m.nt = m.nw = n_weights;
    return lin_predict(device, m, X, n_docs, row_stride, out);
}

}  // extern "C"

// The other three linear rankers: the same translation unit, so each handle's LinCtx is ranked by k_ca_trials and scored by ca_metric
#include "rl_ada.inc"      // AdaRank (-ranker 3): k_ada_weak shares ca_metric and the sets' length classes
#include "rl_rb.inc"       // RankBoost (-ranker 2): its training lists sorted into getCorrectRanking() order in the context's set
#include "rl_lr.inc"       // Linear Regression (-ranker 9): k_lr_gram reads the context's column-major training set
// not a linear ranker, but it shares this unit's build
#include "rl_net.inc"      // RankNet / LambdaRank / ListNet models (-ranker 1 / 5 / 7): the forward pass, scoring only
#include "rl_ln.inc"       // ListNet training (-ranker 7): k_ln_epoch walks the context's training lists, k_ca_trials ranks
#include "rl_rn.inc"       // RankNet training (-ranker 1): k_rn_epoch walks the lists and their documents, net_layer scores, k_ca_trials ranks
#include "rl_perm.inc"     // the Analyzer's randomisation test: k_perm_test draws its sign vectors from this unit's JavaRandom stream
#include "rl_eval.inc"     // test-time evaluation: k_eval_lists ranks and scores every list of a file (shares ca_pow2m1, ca_sync)
#include "rl_norm.inc"     // -norm: k_normalize_lists normalises every list of a file in place
