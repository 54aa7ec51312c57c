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
//   k_ca_recompute       cached = 0.0 + w[0] x0 + w[1] x1 + ...  (rank() with current_feature == -1, :207-213; also CoorAscent.eval)
//
// The host side runs CoorAscent.learn() (:67-202) literally: weights, the keep / restore decisions, the -reg penalty and the shuffle.
// Built with -ffp-contract=off like the rest of the library: no fused multiply-adds, plain IEEE divisions.  There is no CPU fallback.
#include "rl_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>

namespace rl {

constexpr int kCaSteps = 64;          // trials per launch (a direction of more trials is evaluated in pieces of 64: same chain)
constexpr int kCaTiny = 16, kCaWave = 384, kCaBlock = 5000;
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

__device__ __forceinline__ int ca_pow2m1(int rel) { return (int)(((unsigned)1 << (rel & 31)) - 1u); }   // DCGScorer.java:137-139, Java int arithmetic

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

template <int G>
__device__ __forceinline__ void ca_sync()
{
    if (G > kWave) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
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

// column-major X (xc[f * n + i]) or rows (x[i * stride + fid[f]], fid >= stride reads 0)
__global__ void k_ca_recompute(double *out, const float *xc, const float *rows, int64_t stride, const int32_t *fid, const double *w, int32_t F,
                               int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int f = 0; f < F; f++) {
        float v;
        if (xc) v = xc[(int64_t)f * n + i];
        else v = (fid[f] >= 0 && fid[f] < stride) ? rows[i * stride + fid[f]] : 0.f;
        s += w[f] * (double)v;
    }
    out[i] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------
struct CaBuf {                         // device allocations of one handle, freed together
    std::vector<void *> ptrs;
    template <class T> hipError_t alloc(T **p, size_t count)
    {
        hipError_t e = hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    ~CaBuf() { for (void *p : ptrs) (void)hipFree(p); }
};

struct CaClass {
    int32_t nq = 0; int32_t *d_qlist = nullptr;
    int64_t nh = 0; int64_t *d_hoff = nullptr;        // longest class only
};

struct CaSet {
    int64_t N = 0; int32_t Q = 0, maxq = 0;
    std::vector<float> X;              // [N][F] as given
    std::vector<float> labels; std::vector<int32_t> qoff, qkey; bool has_key = false;
    std::vector<double> ext_ideal; std::vector<int32_t> ext_rd;
    float *d_xc = nullptr, *d_labels = nullptr; int32_t *d_qoff = nullptr, *d_rd = nullptr;
    double *d_ideal = nullptr, *d_cache = nullptr, *d_cache2 = nullptr;
    CaClass cls[4];
    double *d_hsc = nullptr; int32_t *d_hrel = nullptr; int32_t hchunks = 0;
};

}  // namespace rl

using namespace rl;

struct rl_ca {
    rl_ca_params p;
    int32_t F = 0;
    bool has_train = false, has_valid = false, learned = false, uploaded = false;
    CaSet tr, va;
    double err_max = 16.0;
    hipStream_t stream = nullptr;
    CaBuf buf;
    double *d_disc = nullptr, *d_m = nullptr, *d_sums = nullptr, *d_w = nullptr; uint32_t *d_done = nullptr;
    double *h_sums = nullptr;
    std::vector<double> weight; double train_score = 0, valid_score = 0;
    std::vector<rl_ca_trace_rec> trace;
    ~rl_ca()
    {
        if (h_sums) (void)hipHostFree(h_sums);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace rl {

static double ca_discount(int i) { return 1.0 / (std::log((double)(i + 2)) / std::log(2.0)); }   // DCGScorer.java:26

static double ca_ideal_dcg(const float *labels, int n, int topk, const std::vector<double> &disc)
{   // NDCGScorer.getIdealDCG (:167-174)
    std::vector<int> rel(n);
    for (int i = 0; i < n; i++) rel[i] = (int)labels[i];
    std::sort(rel.begin(), rel.end(), [](int a, int b) { return a > b; });
    double dcg = 0;
    for (int i = 0; i < topk; i++) dcg += (double)(int32_t)(((uint32_t)1 << (rel[i] & 31)) - 1u) * disc[i];
    return dcg;
}

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

static int ca_check_set(const float *X, int64_t n, int32_t F, const float *labels, const int32_t *qoff, int32_t Q)
{
    if (!X || !labels || !qoff) return fail(RL_ERR_INVALID, "null data pointer");
    if (n <= 0 || Q <= 0 || F <= 0) return fail(RL_ERR_INVALID, "There are no training samples / features");
    if (n >= (int64_t)2147483647 - 4096) return fail(RL_ERR_UNSUPPORTED, "more than 2^31 documents per GPU");
    if (qoff[0] != 0 || (int64_t)qoff[Q] != n) return fail(RL_ERR_INVALID, "qoff must start at 0 and end at n_docs");
    for (int32_t q = 0; q < Q; q++)
        if (qoff[q + 1] <= qoff[q]) return fail(RL_ERR_INVALID, "qoff must be strictly increasing (empty ranked list)");
    for (int64_t i = 0; i < n; i++) {
        if (!(labels[i] >= 0)) return fail(RL_ERR_INVALID, "Relevance label cannot be negative. System will now exit.");
        if (labels[i] >= 16777216.f) return fail(RL_ERR_UNSUPPORTED, "relevance label of 2^24 or more");
    }
    for (int64_t i = 0; i < n * F; i++) {
        if (std::isnan(X[i])) return fail(RL_ERR_INVALID, "NaN in X (a missing feature must be passed as 0)");
        if (std::isinf(X[i])) return fail(RL_ERR_UNSUPPORTED, "+-Infinity feature value: the Java's cached scores turn NaN (0 * Infinity), not reproduced (DESIGN.md 7)");
    }
    return RL_OK;
}

static void ca_store(CaSet &d, const float *X, int64_t n, int32_t F, const float *labels, const int32_t *qoff, int32_t Q, const int32_t *qkey)
{
    d.N = n; d.Q = Q;
    d.X.assign(X, X + n * F);
    d.labels.assign(labels, labels + n);
    d.qoff.assign(qoff, qoff + Q + 1);
    d.has_key = qkey != nullptr;
    if (qkey) d.qkey.assign(qkey, qkey + Q); else d.qkey.clear();
    d.maxq = 0;
    for (int32_t q = 0; q < Q; q++) d.maxq = std::max(d.maxq, qoff[q + 1] - qoff[q]);
    d.ext_ideal.clear(); d.ext_rd.clear();
}

static int ca_upload(rl_ca *c, CaSet &d, const std::vector<double> &ideal)
{
    const int64_t N = d.N; const int32_t F = c->F;
    std::vector<float> xc((size_t)N * F);
    for (int64_t i = 0; i < N; i++)
        for (int32_t f = 0; f < F; f++) xc[(size_t)f * N + i] = d.X[(size_t)i * F + f];
    std::vector<float>().swap(d.X);                  // the rows are not needed on the host any more
    RL_HIP(c->buf.alloc(&d.d_xc, xc.size()));
    RL_HIP(hipMemcpy(d.d_xc, xc.data(), xc.size() * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(c->buf.alloc(&d.d_labels, (size_t)N));
    RL_HIP(hipMemcpy(d.d_labels, d.labels.data(), N * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(c->buf.alloc(&d.d_qoff, (size_t)d.Q + 1));
    RL_HIP(hipMemcpy(d.d_qoff, d.qoff.data(), ((size_t)d.Q + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(c->buf.alloc(&d.d_ideal, (size_t)d.Q));
    RL_HIP(hipMemcpy(d.d_ideal, ideal.data(), d.Q * sizeof(double), hipMemcpyHostToDevice));
    if (!d.ext_rd.empty()) {
        RL_HIP(c->buf.alloc(&d.d_rd, (size_t)d.Q));
        RL_HIP(hipMemcpy(d.d_rd, d.ext_rd.data(), d.Q * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    RL_HIP(c->buf.alloc(&d.d_cache, (size_t)N));
    RL_HIP(c->buf.alloc(&d.d_cache2, (size_t)N));
    std::vector<int32_t> lists[4];
    std::vector<int64_t> hoff;
    int64_t nh = 0;
    for (int32_t q = 0; q < d.Q; q++) {
        const int n = d.qoff[q + 1] - d.qoff[q];
        const int k = n <= kCaTiny ? 0 : n <= kCaWave ? 1 : n <= kCaBlock ? 2 : 3;
        lists[k].push_back(q);
        if (k == 3) { hoff.push_back(nh); nh += n; }
    }
    for (int k = 0; k < 4; k++) {
        CaClass &cl = d.cls[k];
        cl.nq = (int32_t)lists[k].size();
        if (!cl.nq) continue;
        RL_HIP(c->buf.alloc(&cl.d_qlist, lists[k].size()));
        RL_HIP(hipMemcpy(cl.d_qlist, lists[k].data(), lists[k].size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (d.cls[3].nq) {
        CaClass &cl = d.cls[3];
        cl.nh = nh;
        RL_HIP(c->buf.alloc(&cl.d_hoff, hoff.size()));
        RL_HIP(hipMemcpy(cl.d_hoff, hoff.data(), hoff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        d.hchunks = std::max(1, std::min(kCaSteps, 1024 / cl.nq));     // chunks of the trials of one launch (sizes the scratch)
        RL_HIP(c->buf.alloc(&d.d_hsc, (size_t)d.hchunks * nh));
        RL_HIP(c->buf.alloc(&d.d_hrel, (size_t)d.hchunks * nh));
    }
    return RL_OK;
}

// ideal DCGs with the qid-keyed cache quirk (NDCGScorer.java:114-122,134-143), -qrel entries first: as rl_trainer.hip builds them
static int ca_prepare(rl_ca *c)
{
    const int maxq = std::max(c->tr.maxq, c->has_valid ? c->va.maxq : 0);
    std::vector<double> disc((size_t)maxq + 2);
    for (size_t i = 0; i < disc.size(); i++) disc[i] = ca_discount((int)i);
    RL_HIP(c->buf.alloc(&c->d_disc, disc.size()));
    RL_HIP(hipMemcpy(c->d_disc, disc.data(), disc.size() * sizeof(double), hipMemcpyHostToDevice));
    std::map<int64_t, double> cache;
    auto preload = [&](CaSet &d, int64_t anon_base) {
        for (int q = 0; q < d.Q && !d.ext_ideal.empty(); q++)
            if (d.ext_ideal[q] == d.ext_ideal[q]) cache[d.has_key ? (int64_t)d.qkey[q] : anon_base + q] = d.ext_ideal[q];
    };
    preload(c->tr, (int64_t)1 << 40);
    if (c->has_valid) preload(c->va, (int64_t)1 << 41);
    const std::map<int64_t, double> external = cache;
    auto run = [&](CaSet &d, int64_t anon_base, std::vector<double> &cached) {
        cached.resize(d.Q);
        for (int q = 0; q < d.Q; q++) {
            const int n = d.qoff[q + 1] - d.qoff[q];
            const int size = (c->p.metric_k > n || c->p.metric_k <= 0) ? n : c->p.metric_k;
            const int64_t key = d.has_key ? (int64_t)d.qkey[q] : anon_base + q;
            { auto pre = external.find(key); if (pre != external.end()) { cached[q] = pre->second; continue; } }
            auto it = cache.find(key);
            if (it == cache.end()) it = cache.emplace(key, ca_ideal_dcg(d.labels.data() + d.qoff[q], n, size, disc)).first;
            cached[q] = it->second;
        }
    };
    std::vector<double> ideal;
    run(c->tr, (int64_t)1 << 40, ideal);
    int rc = ca_upload(c, c->tr, ideal);
    if (rc) return rc;
    if (c->has_valid) {
        run(c->va, (int64_t)1 << 41, ideal);
        rc = ca_upload(c, c->va, ideal);
        if (rc) return rc;
    }
    RL_HIP(c->buf.alloc(&c->d_m, (size_t)std::max(c->tr.Q, c->has_valid ? c->va.Q : 0) * kCaSteps));
    RL_HIP(c->buf.alloc(&c->d_sums, (size_t)kCaSteps));
    RL_HIP(c->buf.alloc(&c->d_done, 1));
    RL_HIP(hipMemset(c->d_done, 0, sizeof(uint32_t)));
    RL_HIP(c->buf.alloc(&c->d_w, (size_t)c->F));
    RL_HIP(hipHostMalloc((void **)&c->h_sums, kCaSteps * sizeof(double), hipHostMallocDefault));
    c->uploaded = true;
    return RL_OK;
}

// Evaluates trials [0, T) of one direction on set d (steps[t] = the weight change of trial t; first = 0: T == 1, the cache as it is) and
// copies sums[0..T) (= scorer.score(rank(samples)) after each trial) into out.  first = 1 leaves the chain's final value in d.d_cache.
static int ca_trials(rl_ca *c, CaSet &d, const float *xcol, const double *steps, int T, int first, double *out)
{
    CaArgs a;
    memset(&a, 0, sizeof(a));
    a.cache = d.d_cache; a.cache_out = d.d_cache2; a.x = xcol;
    a.labels = d.d_labels; a.qoff = d.d_qoff; a.ideal = d.d_ideal; a.rd_ext = d.d_rd; a.disc = c->d_disc;
    a.m = c->d_m; a.sums = c->d_sums; a.done = c->d_done;
    a.Q = d.Q; a.T = T; a.first = first; a.metric = c->p.metric; a.k = c->p.metric_k; a.err_max = c->err_max;
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
static int ca_direction(rl_ca *c, int f, const std::vector<double> &steps, std::vector<double> &scores)
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

static int ca_apply(rl_ca *c, int f, double wc, bool scale, double sum)
{
    CaSet &d = c->tr;
    const int64_t n = d.N;
    hipLaunchKernelGGL(k_ca_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d.d_cache, d.d_xc + (size_t)f * n, n, wc,
                       scale ? 1 : 0, sum);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// scorer.score(rank(set)) with current_feature == -1: the cache recomputed from the weights
static int ca_score_weights(rl_ca *c, CaSet &d, const std::vector<double> &w, double *score)
{
    RL_HIP(hipMemcpyAsync(c->d_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_ca_recompute, dim3((unsigned)((d.N + 255) / 256)), dim3(256), 0, c->stream, d.d_cache, d.d_xc, (const float *)nullptr,
                       (int64_t)0, (const int32_t *)nullptr, c->d_w, c->F, d.N);
    RL_HIP(hipGetLastError());
    return ca_trials(c, d, nullptr, nullptr, 1, 0, score);
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

static int ca_learn(rl_ca *c)
{
    const rl_ca_params &P = c->p;
    const int F = c->F;
    auto rec = [&](int kind, int r, int f, int dir, int j, int imp, double w, double s) {
        rl_ca_trace_rec t; t.kind = kind; t.restart = r; t.feature = f; t.dir = dir; t.j = j; t.improved = imp; t.weight = w; t.score = s;
        c->trace.push_back(t);
    };
    c->trace.clear();
    std::vector<double> weight((size_t)F), regVector((size_t)F, 1.0 / F);      // init() :62-63, copied at :68-69
    std::vector<double> bestModel; double bestModelScore = 0.0;
    const int sign[3] = {1, -1, 0};
    JavaRandom rnd(P.seed);
    std::vector<double> steps, tw, ts, scores;
    for (int r = 0; r < P.n_restart; r++) {
        int consecutive_fails = 0;
        for (int i = 0; i < F; i++) weight[i] = (double)(1.0f / (float)F);       // :87-89, a float division
        double startScore;
        int rc = ca_score_weights(c, c->tr, weight, &startScore);
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
            int rc2 = ca_score_weights(c, c->va, weight, &bestScore);
            if (rc2) return rc2;
            rec(RL_CA_VALID, r, -1, 0, 0, 0, 0.0, bestScore);
        }
        if (bestModel.empty() || bestScore > bestModelScore) { bestModelScore = bestScore; bestModel = bestWeight; }
    }
    c->weight = bestModel;
    int rc = ca_score_weights(c, c->tr, c->weight, &c->train_score);
    if (rc) return rc;
    c->valid_score = 0;
    if (c->has_valid && (rc = ca_score_weights(c, c->va, c->weight, &c->valid_score))) return rc;
    c->learned = true;
    return RL_OK;
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
    if (p->metric < RL_METRIC_NDCG || p->metric > RL_METRIC_RR)
        return fail(RL_ERR_UNSUPPORTED, "Coordinate Ascent train metric must be NDCG, DCG, MAP, ERR, P or RR (BEST is not built for training)");
    if (p->n_restart < 1) return fail(RL_ERR_INVALID, "n_restart must be >= 1 (the Java ends in a NullPointerException)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(RL_ERR_NO_DEVICE, "no HIP device visible: librlhip has no CPU fallback");
    if (p->device < 0 || p->device >= ndev) return fail(RL_ERR_INVALID, "device ordinal out of range");
    RL_HIP(hipSetDevice(p->device));
    hipDeviceProp_t prop;
    RL_HIP(hipGetDeviceProperties(&prop, p->device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(RL_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", librlhip is built for gfx950 only");
    std::unique_ptr<rl_ca> c(new rl_ca());
    c->p = *p;
    if (!(p->err_max > 0.0) || !std::isfinite(p->err_max)) return fail(RL_ERR_INVALID, "err_max (ERRScorer.MAX) must be positive and finite");
    c->err_max = p->err_max;
    RL_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    *out = c.release();
    return RL_OK;
}

void rl_ca_destroy(rl_ca *c)
{
    if (!c) return;
    (void)hipSetDevice(c->p.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

int rl_ca_set_train(rl_ca *c, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                    int32_t n_queries, const int32_t *qkey)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (c->uploaded) return fail(RL_ERR_STATE, "rl_ca_set_train after rl_ca_learn");
    int rc = ca_check_set(X, n_docs, n_features, labels, qoff, n_queries);
    if (rc) return rc;
    c->F = n_features;
    ca_store(c->tr, X, n_docs, n_features, labels, qoff, n_queries, qkey);
    c->has_train = true;
    return RL_OK;
}

int rl_ca_set_validation(rl_ca *c, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                         const int32_t *qkey)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (!c->has_train) return fail(RL_ERR_STATE, "set the training data first");
    if (c->uploaded) return fail(RL_ERR_STATE, "rl_ca_set_validation after rl_ca_learn");
    int rc = ca_check_set(X, n_docs, c->F, labels, qoff, n_queries);
    if (rc) return rc;
    ca_store(c->va, X, n_docs, c->F, labels, qoff, n_queries, qkey);
    c->has_valid = true;
    return RL_OK;
}

int rl_ca_set_external_judgments(rl_ca *c, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (c->uploaded) return fail(RL_ERR_STATE, "rl_ca_set_external_judgments after rl_ca_learn");
    if (validation ? !c->has_valid : !c->has_train) return fail(RL_ERR_STATE, "set the data first");
    CaSet &d = validation ? c->va : c->tr;
    d.ext_ideal.clear(); d.ext_rd.clear();
    if (ideal_dcg) d.ext_ideal.assign(ideal_dcg, ideal_dcg + d.Q);
    if (rel_doc_count) {
        for (int q = 0; q < d.Q; q++) if (rel_doc_count[q] < 0) return fail(RL_ERR_INVALID, "negative relevant-document count");
        d.ext_rd.assign(rel_doc_count, rel_doc_count + d.Q);
    }
    return RL_OK;
}

int rl_ca_learn(rl_ca *c)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (!c->has_train) return fail(RL_ERR_STATE, "set the training data first");
    if (c->uploaded) return fail(RL_ERR_STATE, "rl_ca_learn runs once per handle");
    RL_HIP(hipSetDevice(c->p.device));
    int rc = ca_prepare(c);
    if (rc) return rc;
    return ca_learn(c);
}

int rl_ca_get_weights(const rl_ca *c, double *w, int32_t cap)
{
    if (!c || !w) return fail(RL_ERR_INVALID, "null argument");
    if (!c->learned) return fail(RL_ERR_STATE, "rl_ca_learn has not run");
    if (cap < c->F) return fail(RL_ERR_INVALID, "weight buffer too small");
    std::copy(c->weight.begin(), c->weight.end(), w);
    return RL_OK;
}

int rl_ca_scores(const rl_ca *c, double *train, double *valid)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (!c->learned) return fail(RL_ERR_STATE, "rl_ca_learn has not run");
    if (train) *train = c->train_score;
    if (valid) *valid = c->valid_score;
    return RL_OK;
}

int rl_ca_trace(const rl_ca *c, rl_ca_trace_rec *out, int64_t cap, int64_t *n)
{
    if (!c || !n) return fail(RL_ERR_INVALID, "null argument");
    *n = (int64_t)c->trace.size();
    if (out) std::copy(c->trace.begin(), c->trace.begin() + std::min<int64_t>(cap, *n), out);
    return RL_OK;
}

int rl_ca_predict(int32_t device, const int32_t *feature_ids, const double *weights, int32_t n_weights, const float *X, int64_t n_docs,
                  int32_t row_stride, double *out)
{
    if (!feature_ids || !weights || !out || (n_docs > 0 && !X)) return fail(RL_ERR_INVALID, "null argument");
    if (n_weights < 0 || n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad sizes");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(RL_ERR_NO_DEVICE, "no HIP device visible: librlhip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(RL_ERR_INVALID, "device ordinal out of range");
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(device));
    CaBuf buf;
    float *dX = nullptr; int32_t *dF = nullptr; double *dW = nullptr, *dO = nullptr;
    RL_HIP(buf.alloc(&dX, (size_t)n_docs * row_stride));
    RL_HIP(buf.alloc(&dF, (size_t)n_weights));
    RL_HIP(buf.alloc(&dW, (size_t)n_weights));
    RL_HIP(buf.alloc(&dO, (size_t)n_docs));
    RL_HIP(hipMemcpy(dX, X, (size_t)n_docs * row_stride * sizeof(float), hipMemcpyHostToDevice));
    if (n_weights) {
        RL_HIP(hipMemcpy(dF, feature_ids, n_weights * sizeof(int32_t), hipMemcpyHostToDevice));
        RL_HIP(hipMemcpy(dW, weights, n_weights * sizeof(double), hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_ca_recompute, dim3((unsigned)((n_docs + 255) / 256)), dim3(256), 0, 0, dO, (const float *)nullptr, dX, (int64_t)row_stride,
                       dF, dW, n_weights, n_docs);
    RL_HIP(hipGetLastError());
    RL_HIP(hipMemcpy(out, dO, n_docs * sizeof(double), hipMemcpyDeviceToHost));
    return RL_OK;
}

}  // extern "C"

#include "rl_ada.inc"      // AdaRank (-ranker 3): the same translation unit, so its kernels share ca_metric and k_ca_trials
#include "rl_rb.inc"       // RankBoost (-ranker 2): the device sets, ca_metric and the ranking kernel again
#include "rl_lr.inc"       // Linear Regression (-ranker 9): the same
