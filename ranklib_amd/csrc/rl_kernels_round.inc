// rl_kernels_round.inc -- gfx950 kernels of one boosting round (included by rl_trainer.hip).
//
// K1  k_rank_*, k_lambda_fused / k_pair_terms + k_lambda_acc, k_mart_residual, k_max_reduce
//                       per-query stable rank + pairwise swap change x sigmoid   LambdaMART.java:361-396, MART.java:47-51
// K1b k_quantize        lambda -> order-independent fixed point                   (DESIGN.md 3 "exact sums")
// K2/3 k_hist<ROOT>     LDS-staged per-chunk histograms                           FeatureHistogram.java:126-146,166-195
// K4/5 k_hist_finish    chunk reduction, prefix over thresholds, sibling = parent - built child, per-feature gain scan
//                                                                                 FeatureHistogram.java:141-145,189-194,222-264
//      select_step      (last block of k_hist_finish) best-first growth bookkeeping, speculative slots
//                                                                                 RegressionTree.java:58-87,147-157
// K6  k_part_scatter<LOOKBACK> (+ k_part_count when sharded)  stable partition    FeatureHistogram.java:328-341
// K7  k_leaf_table, k_leaf_output, k_score_update (+ rl_chain.inc)                LambdaMART.java:398-415, 203-210
// K8  per-query metric in k_rank_*, float mean via rl_chain.inc / k_float_mean    LambdaMART.java:442-483
// K10 k_ensemble_eval, k_valid_update (k_model_eval* live in rl_trainer.hip)      Ensemble.java:110-116, Split.java:115-125

namespace rl {

// ------------------------------------------------------------------------------------------------
// small helpers
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

// ------------------------------------------------------------------------------------------------
// K1: lambdas.  G threads (one wavefront, or the whole block for long queries) own one query.
//   1. stage score/label in LDS                     2. stable descending rank by counting
//   3. each sorted position accumulates ITS lambda and weight in exactly the order the Java loop
//      touches pseudoResponses[idx[p]] (j outer, k inner), so the f64 results are bit-identical and no
//      atomics are needed.  Every pair's rho is therefore evaluated from both ends.
// ------------------------------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ void group_sync()
{
    if (G > kWave) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
}

// ------------------------------------------------------------------------------------------------
// K1 (three kernels): lambdas without serial exp/div chains.
//   k_rank_*      per query: stable descending rank (MergeSorter.sort, utilities/MergeSorter.java:134-189) ->
//                 score / label / original slot in ranked order, plus NDCG@k of that ranking (the sort of round
//                 m+1's lambdas is the sort round m's training metric needs: it is done once).
//   k_pair_terms  one thread per ranked document b: the swap terms of the pairs (a, b), a < min(b, k): the
//                 expensive part (|dNDCG|, exp, three f64 divisions) is embarrassingly parallel.
//   k_lambda_acc  one thread per ranked document: adds ITS terms in exactly the order the Java loop visits them
//                 (LambdaMART.java:371-393: j outer, k inner), so lambda and weight are bit-identical f64 sums.
// T layout: T[(cur + b) * K + a] = (lambda term, weight term) of pair (a, b); lambda term < 0 marks "inactive".
// ------------------------------------------------------------------------------------------------
constexpr int kRankLdsPerDoc = 20;      // LDS bytes per document of the rank kernels: score, int label, label, original slot
struct RankArgs {
    const double *scores; const float *labels; const int *qoff; const double *ideal; const double *disc;
    double *ss; float *sl; int *srel; int *sidx;     // ranked order (may be null for metric-only use)
    double *ndcg; int k;
    int metric;                  // RL_METRIC_*
    int *aux_i; double *aux_a, *aux_b;   // ranked-order per-query tables for the swap changes of MAP / ERR, RR: aux_i[2 q], [2 q + 1] = firstRank, secondRank (may be null)
    double err_max;              // ERRScorer.MAX = 2^gmax (metric/ERRScorer.java:25, set by -gmax: eval/Evaluator.java:241-242)
    const int *rd_ext;           // MAP with -qrel: relDocCount of every list's qid (0 = not in the file), null = the list's own count (APScorer.java:86-94)
};

__device__ __forceinline__ double err_R(int rel, double mx) { return (double)java_pow2m1(rel) / mx; }    // ERRScorer.java:71-73

// The scorer's value of one ranked list + the ranked-order tables its swapChange needs, by ONE thread.  s_rel: int view of the ranked
// labels (NDCG / DCG / ERR: (int)label of the top `size`, MAP / P / RR: label > 0 of all n positions).
__device__ __forceinline__ bool metric_binary_view(int metric) { return metric == RL_METRIC_MAP || metric == RL_METRIC_P || metric == RL_METRIC_RR; }
__device__ void rank_metric(const RankArgs &a, int qi, int cur, int n, int size, const int *s_rel)
{
    const bool is_map = a.metric == RL_METRIC_MAP;
    {
        double res = 0.0;
        if (a.metric == RL_METRIC_NDCG) {
            const double ideal = a.ideal[qi];
            if (n > 0 && ideal > 0.0) {                                        // NDCGScorer.score :103-129
                double dcg = 0;
                for (int i = 0; i < size; i++) dcg += gain_of(s_rel[i]) * a.disc[i];   // DCGScorer.java:97-103
                res = dcg / ideal;
            }
        } else if (a.metric == RL_METRIC_DCG) {                                 // DCGScorer.score :58-71
            for (int i = 0; i < size; i++) res += gain_of(s_rel[i]) * a.disc[i];
        } else if (is_map) {                                                    // APScorer.score :73-100 (whole list)
            double ap = 0.0; int count = 0;
            for (int i = 0; i < n; i++) {
                if (s_rel[i]) { count++; ap += ((double)count) / (i + 1); }
                if (a.aux_i) a.aux_i[cur + i] = count;                          // relCount[] of swapChange :111-122
            }
            const int rdc = a.rd_ext ? a.rd_ext[qi] : count;
            res = (rdc == 0) ? 0.0 : ap / rdc;
        } else if (a.metric == RL_METRIC_P) {                                   // PrecisionScorer.score :30-44
            int count = 0;
            for (int i = 0; i < size; i++) count += s_rel[i];
            res = ((double)count) / size;
        } else if (a.metric == RL_METRIC_RR) {                                  // ReciprocalRankScorer.score :26-35, and firstRank / secondRank of swapChange :49-61
            const int rsize = (n > a.k) ? a.k : n;
            int first = -1, second = -1;
            for (int i = 0; i < rsize && second < 0; i++)
                if (s_rel[i]) { if (first < 0) first = i; else second = i; }
            res = (first < 0) ? 0.0 : (double)(1.0f / (float)(first + 1));      // a float division, widened
            if (a.aux_i) { a.aux_i[2 * qi] = first; a.aux_i[2 * qi + 1] = second; }
        } else {                                                                // ERRScorer.score :45-64
            double sc = 0.0, p = 1.0;
            for (int i = 1; i <= size; i++) { const double R = err_R(s_rel[i - 1], a.err_max); sc += p * R / i; p *= (1.0 - R); }
            res = sc;
            if (a.aux_a) {          // R[] and np[] of swapChange :78-88: filled for i < min(k, n) only, the rest stays 0 (zeroed once by rl_init)
                const int ssize = (n > a.k) ? a.k : n;
                double pp = 1.0;
                for (int i = 0; i < ssize; i++) {
                    const double R = err_R(s_rel[i], a.err_max), np = pp * (1.0 - R);
                    pp *= np;
                    a.aux_a[cur + i] = R; a.aux_b[cur + i] = np;
                }
            }
        }
        a.ndcg[qi] = res;
    }
}

// s_rel: int view of the ranked labels (NDCG / DCG / ERR: (int)label, MAP / P / RR: label > 0), all n positions for MAP and
// for the aux tables, else the top `size`.
template <int G, int CAP>
__device__ void rank_query(const RankArgs &a, int qi, int tid, double *s_raw, int *s_rel, float *s_lab, int *s_idx)
{
    int cur = a.qoff[qi], n = a.qoff[qi + 1] - cur;
    if (G >= kWave) {       // one list per wavefront: say so -- loops whose bounds sit in vector registers are compiled as divergent loops (no unrolling, one
        cur = __builtin_amdgcn_readfirstlane(cur); n = __builtin_amdgcn_readfirstlane(n);       // LDS round trip per iteration)
    }
    for (int i = tid; i < n; i += G) s_raw[i] = a.scores[cur + i];
    group_sync<G>();
    int size = a.k;
    if (a.k > n || a.k <= 0) size = n;
    const bool is_map = a.metric == RL_METRIC_MAP, bin_view = metric_binary_view(a.metric);
    // The ranked order is assembled in LDS and leaves in rows: written straight to ss[cur + pos] .. the 4- and 8-byte stores of a wavefront land
    // on as many memory sectors as it has lanes (four arrays: 15 M partial-sector writes a round at c2, the whole cost of these kernels).
    constexpr int PER = (CAP + G - 1) / G;
    double v[PER]; float l[PER]; int pos[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int r = tid + u * G;
        pos[u] = 0; v[u] = 0.0; l[u] = 0.f;
        if (G >= kWave) {
            // The count is bound by instruction issue (n x n/64 wavefront iterations of two f64 compares, an index compare and their glue: 0.1 ms a
            // round at c2).  A wavefront's documents are 64 consecutive slots [rb, rb + 64): every j below rb precedes all of them (count x >= v),
            // every j from rb + 64 on follows all of them (count x > v) -- one compare and an add-with-carry; only the 64 slots in between need
            // the index.
            const int rb = __builtin_amdgcn_readfirstlane(r);
            if (rb >= n) break;                              // (wave-uniform)
            v[u] = (r < n) ? s_raw[r] : 0.0;
            const int j0 = rb, j1 = min(rb + 64, n);
            int p = 0;
#pragma unroll 8
            for (int j = 0; j < j0; j++) p += (s_raw[j] >= v[u]) ? 1 : 0;
#pragma unroll 8
            for (int j = j0; j < j1; j++) { const double x = s_raw[j]; p += ((x > v[u]) || (x == v[u] && j < r)) ? 1 : 0; }
#pragma unroll 8
            for (int j = j1; j < n; j++) p += (s_raw[j] > v[u]) ? 1 : 0;
            pos[u] = p;
            if (r < n) l[u] = a.labels[cur + r];
        } else if (r < n) {
            v[u] = s_raw[r];
            int p = 0;
            for (int j = 0; j < n; j++) { const double x = s_raw[j]; p += (x > v[u]) || (x == v[u] && j < r); }
            pos[u] = p; l[u] = a.labels[cur + r];
        }
    }
    group_sync<G>();            // every rank is counted: the raw scores may go
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int r = tid + u * G;
        if (r < n) {
            s_raw[pos[u]] = v[u]; s_rel[pos[u]] = bin_view ? (l[u] > 0.f ? 1 : 0) : (int)l[u];
            if (a.ss) { s_lab[pos[u]] = l[u]; s_idx[pos[u]] = r; }
        }
    }
    group_sync<G>();
    if (a.ss)
        for (int i = tid; i < n; i += G) { const float lv = s_lab[i]; a.ss[cur + i] = s_raw[i]; a.sl[cur + i] = lv; a.srel[cur + i] = (int)lv; a.sidx[cur + i] = s_idx[i]; }
    group_sync<G>();
    if (is_map) {
        // APScorer.score / relCount[] (metric/APScorer.java:73-100,111-122) by the whole group: the counts are integers (one thread's
        // running count, cheap), the quotients count / (i + 1) are independent divisions (all threads), and only the additions are the
        // Java's sequential chain (one thread; adding the +0.0 of a non-relevant position to a sum that starts at +0.0 changes nothing)
        if (tid == 0) { int count = 0; for (int i = 0; i < n; i++) { const int r = s_rel[i]; count += r; s_rel[i] = (count << 1) | r; } }
        group_sync<G>();
        for (int i = tid; i < n; i += G) {
            const int e = s_rel[i], cnt = e >> 1;
            if (a.aux_i) a.aux_i[cur + i] = cnt;
            s_raw[i] = (e & 1) ? ((double)cnt) / (i + 1) : 0.0;
        }
        group_sync<G>();
        if (tid == 0) {
            double ap = 0.0;
            for (int i = 0; i < n; i++) ap += s_raw[i];
            const int count = (n > 0) ? (s_rel[n - 1] >> 1) : 0;
            const int rdc = a.rd_ext ? a.rd_ext[qi] : count;
            a.ndcg[qi] = (rdc == 0) ? 0.0 : ap / rdc;
        }
        return;
    }
    if (G >= kWave && size <= kWave && (a.metric == RL_METRIC_NDCG || a.metric == RL_METRIC_DCG)) {
        // NDCG / DCG of the ranking (NDCGScorer.score :103-129, DCGScorer.java:97-103) by wavefront 0: the terms gain * discount are independent
        // (one lane each, one round of loads), only the additions are the Java's sequential chain -- one lane walking the top `size` positions paid a
        // dependent LDS read, table load, multiply and add per position (~1.4 us of every list's ~6 us on its wavefront)
        if (tid < kWave) {
            const double term = (tid < size) ? gain_of(s_rel[tid]) * a.disc[tid] : 0.0;
            const double ideal = (a.metric == RL_METRIC_NDCG) ? a.ideal[qi] : 1.0;
            double dcg = 0;
            for (int i = 0; i < size; i++) dcg += readlane_f64(term, i);
            double res = dcg;
            if (a.metric == RL_METRIC_NDCG) res = (n > 0 && ideal > 0.0) ? dcg / ideal : 0.0;
            if (tid == 0) a.ndcg[qi] = res;
        }
        return;
    }
    if (tid == 0) rank_metric(a, qi, cur, n, size, s_rel);
}

// cap = documents per list the launch's LDS was sized for (a multiple of 2): the short lists -- most of them -- are launched apart from the
// long ones so that their blocks fill a CU's wavefront slots instead of its LDS
__global__ __launch_bounds__(kThreads) void k_rank_wave(const RankArgs a, const int *qlist, int nq, int cap)
{
    constexpr int CAP = kLambdaWaveCap;
    extern __shared__ unsigned char smem_raw[];
    const int wave = threadIdx.x >> 6;
    const int slot = blockIdx.x * 4 + wave;
    if (slot >= nq) return;
    const int qi = qlist ? qlist[slot] : slot;
    unsigned char *base = smem_raw + (size_t)wave * ((size_t)cap * kRankLdsPerDoc);
    rank_query<kWave, CAP>(a, qi, lane_id(), (double *)base, (int *)(base + (size_t)cap * 8), (float *)(base + (size_t)cap * 12), (int *)(base + (size_t)cap * 16));
}

// lists of at most 16 documents: a 16-lane group per query, four per wavefront (a wavefront per query leaves 54 lanes idle)
constexpr int kRankTinyDocs = 16, kRankTinyGroups = 16;
__global__ __launch_bounds__(kRankTinyDocs * kRankTinyGroups) void k_rank_tiny(const RankArgs a, const int *qlist, int nq)
{
    __shared__ unsigned char sm[kRankTinyGroups * kRankTinyDocs * kRankLdsPerDoc];
    const int grp = threadIdx.x / kRankTinyDocs;
    const int slot = blockIdx.x * kRankTinyGroups + grp;
    if (slot >= nq) return;
    unsigned char *base = sm + (size_t)grp * (kRankTinyDocs * kRankLdsPerDoc);
    rank_query<kRankTinyDocs, kRankTinyDocs>(a, qlist[slot], threadIdx.x % kRankTinyDocs, (double *)base, (int *)(base + kRankTinyDocs * 8), (float *)(base + kRankTinyDocs * 12),
                                             (int *)(base + kRankTinyDocs * 16));
}

// Lists beyond the LDS capacity of k_rank_block (RankLib has no limit on a ranked list's length: LambdaMART.java:361-396): the same
// rank-by-counting, the scores staged through LDS in tiles, eight documents per thread and tile sweep, the ranked labels in global
// scratch.  O(n^2) like the others; such lists are rare (MSLR's longest has 1251 documents).
constexpr int kRankBlockThreads = 1024;
constexpr int kRankHugeTile = 4096, kRankHugeDocs = 8;
__global__ __launch_bounds__(kRankBlockThreads) void k_rank_huge(const RankArgs a, const int *qlist, int nq, int *rel_scratch)
{
    __shared__ double tile[kRankHugeTile];
    if ((int)blockIdx.x >= nq) return;
    const int qi = qlist[blockIdx.x], tid = threadIdx.x;
    const int cur = a.qoff[qi], n = a.qoff[qi + 1] - cur;
    int size = a.k;
    if (a.k > n || a.k <= 0) size = n;
    const bool bin_view = metric_binary_view(a.metric);
    int *s_rel = rel_scratch + cur;
    for (int base = 0; base < n; base += kRankBlockThreads * kRankHugeDocs) {   // block-uniform trip count (barriers inside)
        double v[kRankHugeDocs]; int r[kRankHugeDocs], pos[kRankHugeDocs];
#pragma unroll
        for (int u = 0; u < kRankHugeDocs; u++) { r[u] = base + tid + u * kRankBlockThreads; v[u] = r[u] < n ? a.scores[cur + r[u]] : 0.0; pos[u] = 0; }
        for (int t0 = 0; t0 < n; t0 += kRankHugeTile) {
            __syncthreads();
            const int m = min(kRankHugeTile, n - t0);
            for (int j = tid; j < m; j += kRankBlockThreads) tile[j] = a.scores[cur + t0 + j];
            __syncthreads();
            for (int j = 0; j < m; j++) {
                const double x = tile[j];
#pragma unroll
                for (int u = 0; u < kRankHugeDocs; u++) pos[u] += (x > v[u]) || (x == v[u] && t0 + j < r[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kRankHugeDocs; u++) {
            if (r[u] >= n) continue;
            const float l = a.labels[cur + r[u]];
            s_rel[pos[u]] = bin_view ? (l > 0.f ? 1 : 0) : (int)l;
            if (a.ss) { a.ss[cur + pos[u]] = v[u]; a.sl[cur + pos[u]] = l; a.srel[cur + pos[u]] = (int)l; a.sidx[cur + pos[u]] = r[u]; }
        }
    }
    __syncthreads();
    if (tid == 0) rank_metric(a, qi, cur, n, size, s_rel);
}

// long lists: 1024 threads per query (the rank is an O(n^2) count; the longest list sets the kernel's duration)
// cap = documents the launch's LDS was sized for (the longest of these lists: a block sized for kLambdaBlockCap keeps a CU to itself)
__global__ __launch_bounds__(kRankBlockThreads) void k_rank_block(const RankArgs a, const int *qlist, int nq, int cap)
{
    constexpr int CAP = kLambdaBlockCap;
    extern __shared__ unsigned char smem_raw[];
    if ((int)blockIdx.x >= nq) return;
    rank_query<kRankBlockThreads, CAP>(a, qlist[blockIdx.x], threadIdx.x, (double *)smem_raw, (int *)(smem_raw + (size_t)cap * 8), (float *)(smem_raw + (size_t)cap * 12),
                                       (int *)(smem_raw + (size_t)cap * 16));
}

// One launch for the long and the ordinary lists: the first nbig blocks rank one long list each (the whole block), the others sixteen ordinary
// lists (a wavefront each).  The long lists set the duration of a launch of their own (a block is bound by its CU's vector ALUs: n^2 / 64 wavefront
// iterations) while most of the chip idles; started first in a common launch they run beside the ordinary lists.  LDS: max(cap_big, 16 x cap) x 20 bytes.
__global__ __launch_bounds__(kRankBlockThreads) void k_rank_mixed(const RankArgs a, const int *qbig, int nbig, int cap_big, const int *qsmall, int nsmall, int cap)
{
    extern __shared__ unsigned char smem_raw[];
    if ((int)blockIdx.x < nbig) {
        rank_query<kRankBlockThreads, kLambdaBlockCap>(a, qbig[blockIdx.x], threadIdx.x, (double *)smem_raw, (int *)(smem_raw + (size_t)cap_big * 8),
                                                       (float *)(smem_raw + (size_t)cap_big * 12), (int *)(smem_raw + (size_t)cap_big * 16));
        return;
    }
    const int wave = threadIdx.x >> 6;
    const int slot = ((int)blockIdx.x - nbig) * (kRankBlockThreads / 64) + wave;
    if (slot >= nsmall) return;
    unsigned char *base = smem_raw + (size_t)wave * ((size_t)cap * kRankLdsPerDoc);
    rank_query<kWave, kLambdaWaveCap>(a, qsmall[slot], lane_id(), (double *)base, (int *)(base + (size_t)cap * 8), (float *)(base + (size_t)cap * 12), (int *)(base + (size_t)cap * 16));
}

struct LamArgs {
    const double *ss; const float *sl; const int *srel; const int *sidx; const int *qoff; const int *doc_q;
    const double *ideal; const double *disc; double2 *T; double2 *lw; unsigned long long *maxbits;        // lw[doc] = (lambda, weight)
    int N, k, K;                 // k = rows of the ranked list whose pairs are visited (see lambda_rows), K = row stride of T
    int metric, mk;              // RL_METRIC_*, the scorer's k
    const int *aux_i; const double *aux_a, *aux_b;
    double *blockmax;            // [blocks of the launch] max |lambda| written by every block (k_max_reduce folds them)
    const int *rd_ext;           // MAP with -qrel: rdCount of every list from the judgment file (APScorer.java:124-133), null = its own count
};

// max |lambda| of a block -> blockmax[blockIdx.x].  One atomicMax per wavefront on a single word (90 k of them at c2)
// serialises in L2 and cost a third of the lambda kernels; plain stores + one small reduction kernel do not.
__device__ __forceinline__ void block_store_max(double wmax, double *blockmax)
{
    __shared__ double sh_wmax[16];
    for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, o));
    if (lane_id() == 0) sh_wmax[threadIdx.x >> 6] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0;
        for (int w = 0; w < (int)((blockDim.x + 63) >> 6); w++) m = fmax(m, sh_wmax[w]);
        blockmax[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(1024) void k_max_reduce(const double *blockmax, int n, unsigned long long *maxbits)
{
    // (a few blocks, four values per thread in flight: one block walking 31 520 values in 31 dependent trips was 10 us behind every round's lambdas)
    double m = 0.0;
    const int stride = (int)gridDim.x * 1024;
    for (int i0 = (int)blockIdx.x * 1024 + (int)threadIdx.x; i0 < n; i0 += 4 * stride) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = blockmax[min(i0 + u * stride, n - 1)];
#pragma unroll
        for (int u = 0; u < 4; u++) m = fmax(m, v[u]);
    }
    __shared__ double sh[16];
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if (lane_id() == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) m = fmax(m, sh[w]);
        if (m > 0) atomicMax(maxbits, (unsigned long long)d2bits(m));
    }
}

// |changes[a][b]| of the scorer's swapChange for ranked positions a < b of the query starting at cur (LambdaMART.java:381)
__device__ double swap_change_abs(const LamArgs &g, int q, int cur, int n, int a, int b, double ideal)
{
    if (g.metric == RL_METRIC_NDCG || g.metric == RL_METRIC_DCG) {
        // NDCGScorer.java:151-157 / DCGScorer.java:84-88 (DCG: ideal == 1.0, x / 1.0 == x)
        return fabs((g.disc[a] - g.disc[b]) * (gain_of(g.srel[cur + a]) - gain_of(g.srel[cur + b])) / ideal);
    }
    if (g.metric == RL_METRIC_MAP) {                 // APScorer.java:145-159 (K ignored; rdCount = relevant documents of the list)
        const int cntq = g.aux_i[cur + n - 1];
        const int rd = g.rd_ext ? g.rd_ext[q] : cntq;       // :124-133
        if (rd == 0 || cntq == 0) return 0.0;               // :141-143
        const int la = g.sl[cur + a] > 0.f ? 1 : 0, lb = g.sl[cur + b] > 0.f ? 1 : 0;
        double change = 0;
        if (la != lb) {
            const int diff = lb - la, ra = g.aux_i[cur + a], rb = g.aux_i[cur + b];
            change += ((double)((ra + diff) * lb - ra * la)) / (a + 1);
            for (int k = a + 1; k <= b - 1; k++) if (g.sl[cur + k] > 0.f) change += ((double)diff) / (k + 1);
            change += ((double)(-rb * diff)) / (b + 1);
        }
        return fabs(change / rd);
    }
    if (g.metric == RL_METRIC_P) {                   // PrecisionScorer.java:57-77: only pairs a < size <= b; ((float) c) / size is a FLOAT division
        const int size = (n > g.mk) ? g.mk : n;
        const int ra = g.sl[cur + a] > 0.f ? 1 : 0, rb = g.sl[cur + b] > 0.f ? 1 : 0;
        if (!(a < size && b >= size)) return 0.0;
        return fabs((double)(((float)(rb - ra)) / (float)size));
    }
    if (g.metric == RL_METRIC_RR) {                  // ReciprocalRankScorer.java:48-107 (firstRank / secondRank: the rank kernel's, aux_i[2 q], [2 q + 1])
        const int size = (n > g.mk) ? g.mk : n;
        const int first = g.aux_i[2 * q], second = g.aux_i[2 * q + 1];
        const double rr = (first != -1) ? 1.0 / (first + 1) : 0.0;                                  // :70-73
        const int feff = (first != -1) ? first : size;                                              // :95
        // the third loop (:99-105) runs last: its value stands where an entry is written twice
        if (a < feff && b >= feff && g.sl[cur + b] > 0.f) return fabs(1.0 / (a + 1) - rr);
        if (first != -1 && a == first && g.srel[cur + b] == 0) {                                    // "non-relevant" is ((int) label) == 0
            if (b < size) return fabs((second == -1 || b < second) ? 1.0 / (b + 1) - rr : 1.0 / (second + 1) - rr);      // :74-83
            return fabs((second == -1) ? -rr : 1.0 / (second + 1) - rr);                            // :84-93
        }
        return 0.0;
    }
    // ERRScorer.java:91-112; a < size.  labels / R / np beyond `size` are 0 in the Java, and the k-loop past `size`
    // only adds +-0 and multiplies by 1, so it stops at min(b, size).
    const int size = (n > g.mk) ? g.mk : n;
    const int la = g.srel[cur + a], lb = (b < size) ? g.srel[cur + b] : 0;
    if (la == lb) return 0.0;
    const double Ra = g.aux_a[cur + a], Rb = g.aux_a[cur + b];
    const double base = (a == 0) ? 1.0 : g.aux_b[cur + a - 1];
    const double v1 = 1.0 / (a + 1) * base;
    double change = v1 * (Rb - Ra);
    double p = base * (Ra - Rb);
    const int kend = min(b, size);
    for (int k = a + 1; k < kend; k++) { const double Rk = g.aux_a[cur + k]; change += p * Rk / (1 + k); p *= 1.0 - Rk; }
    if (b > kend) change += p * 0.0;         // the Java's iterations past `size` add p * 0 / (1 + k): +-0 -- or NaN once p has overflowed to +-Infinity
    const double npb = g.aux_b[cur + b - 1];
    change += (npb * (1.0 - Rb) * Ra / (1.0 - Ra) - npb * Rb) / (b + 1);
    return fabs(change);
}

__global__ __launch_bounds__(kThreads) void k_pair_terms(const LamArgs g)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g.N) return;
    const int q = g.doc_q[p];
    const int cur = g.qoff[q], n = g.qoff[q + 1] - cur;
    const int b = p - cur;
    const int size = (n > g.k) ? g.k : n;                    // rows whose pairs are visited
    const int na = min(b, size);
    const double ideal = g.ideal ? g.ideal[q] : 1.0;
    const float lb = g.sl[p];
    const double sb = g.ss[p];
    double2 *row = g.T + (size_t)p * g.K;
    for (int a = 0; a < na; a++) {
        const float la = g.sl[cur + a];
        double2 t = make_double2(-1.0, 0.0);
        if (ideal > 0 && la != lb) {
            const double d = swap_change_abs(g, q, cur, n, a, b, ideal);
            if (d > 0) {
                const double sa = g.ss[cur + a];
                const double diff = (la > lb) ? (sa - sb) : (sb - sa);          // modelScores[high] - modelScores[low]
                const double rho = 1.0 / (1 + exp_fdlibm(diff));               // :383
                t.x = rho * d;                                                 // :384
                t.y = rho * (1.0 - rho) * d;                                   // :387
            }
        }
        row[a] = t;
    }
}

__global__ __launch_bounds__(kThreads) void k_lambda_acc(const LamArgs g)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    double lam = 0.0, w = 0.0;
    int outi = -1;
    if (p < g.N) {
        const int q = g.doc_q[p];
        const int cur = g.qoff[q], n = g.qoff[q + 1] - cur;
        const int b = p - cur;
        const int size = (n > g.k) ? g.k : n;
        const float lp = g.sl[p];
        const int K = g.K;
        const double2 *mine = g.T + (size_t)p * K;           // pairs (a, b), a < min(b, size)
        const int na = min(b, size);
        // j < b: b is the lower-labelled document of the pair (j, b)
        for (int a = 0; a < na; a++) {
            if (g.sl[cur + a] > lp) { const double2 t = mine[a]; if (t.x >= 0) { lam -= t.x; w += t.y; } }
        }
        // j == b: b is the higher-labelled document against every k (k < b here, k > b below)
        for (int a = 0; a < na; a++) {
            if (lp > g.sl[cur + a]) { const double2 t = mine[a]; if (t.x >= 0) { lam += t.x; w += t.y; } }
        }
        if (b < size) {
            const double2 *col = g.T + (size_t)(cur) * K + b;     // pair (b, k) lives in row k, column b
            for (int k = b + 1; k < n; k++) {
                if (lp > g.sl[cur + k]) { const double2 t = col[(size_t)k * K]; if (t.x >= 0) { lam += t.x; w += t.y; } }
            }
            // j > b
            for (int j = b + 1; j < n; j++) {
                if (g.sl[cur + j] > lp) { const double2 t = col[(size_t)j * K]; if (t.x >= 0) { lam -= t.x; w += t.y; } }
            }
        }
        outi = cur + g.sidx[p];
    }
    if (outi >= 0) g.lw[outi] = make_double2(lam, w);
    double wmax = fabs(lam);
    block_store_max(wmax, g.blockmax);
}

// Fused variant for k <= kLambdaFusedMaxK: one block per query, the term matrix lives in LDS (tiles of BT ranked
// documents).  Column threads compute the pair terms of their document; the first `size` threads are the "row
// owners" (top-k positions) and add their row in ranked order: sweep 0 = terms where the owner is the higher
// label (LambdaMART.java:371-393, j == owner), sweep 1 = terms where it is the lower one (j > owner).  Queries
// longer than one tile recompute the tiles in sweep 1 instead of storing them.
//
// A term is stored SIGNED: (+x, +y) when the row (top) document has the higher label, (-x, -y) when the column
// document has it, (0, 0) when the pair is inactive.  The ordered loops then need no labels and no compares:
// "terms where I am the higher one" is max(v, 0), "where I am the lower one" is max(-v, 0), and adding the +0.0 a
// skipped pair leaves is exact (an accumulator that starts at +0.0 and only receives non-zero terms or +0.0 is never
// -0.0).  Pair terms are computed branch-free, two rows per step, so two independent exp / division chains are in flight.
// A pair term in two halves around its rho, so that TWO pairs can put their exp / division chains into one basic block (rho_fdlibm2):
//   pair_pre_*  -> |swap change| d, the score difference (high label - low label), the signs;   pair_fin -> the signed (lambda, weight) term
// DF (block-uniform, lambda_div_fast): the list's ideal DCG lies in the range where div_by_rcp IS the IEEE quotient and ideal_r2 = rcp_newton2(ideal_div);
// otherwise the compiler's division.  A template parameter, not a run-time branch inside the term: a branch would cut the chains apart again.
struct PairPre { double d, diff; bool hi_row, on; };
#ifdef RL_LAMBDA_R04
__device__ __forceinline__ bool lambda_div_fast(double) { return false; }
#else
__device__ __forceinline__ bool lambda_div_fast(double ideal_div) { return ideal_div > 0x1p-200 && ideal_div < 0x1p200; }
#endif
// rows of the term matrix a column thread generates per step = exp / division chains it keeps in flight (the rest of a list's rows: pairs, then one)
#ifndef RL_LAMBDA_ROWS
#define RL_LAMBDA_ROWS 2
#endif
template <bool DF>
__device__ __forceinline__ PairPre pair_pre_signed(bool in_range, bool ideal_pos, double ideal_div, double ideal_r2, float la, float lb, double da, double db,
                                                   double ga, double gb, double sa, double sb)
{
    // NDCGScorer.java:154 (DCG: ideal_div == 1).  The numerator is 0 or |.| in [2^-60, 2^70] (a difference of two discounts 1 / log2(i + 2)
    // times a difference of two integer gains below 2^31): with the divisor in [2^-200, 2^200] no operand of the division needs scaling.
    const double nd = (da - db) * (ga - gb);
    PairPre p;
    p.d = fabs(DF ? div_by_rcp(nd, ideal_div, ideal_r2) : nd / ideal_div);
    p.hi_row = la > lb;
    p.diff = p.hi_row ? (sa - sb) : (sb - sa);                                     // modelScores[high] - modelScores[low]
    p.on = in_range && ideal_pos && (la != lb) && (p.d > 0);
    return p;
}
// The same from a swap change computed elsewhere (ERR, MAP)
__device__ __forceinline__ PairPre pair_pre_delta(bool in_range, float la, float lb, double d, double sa, double sb)
{
    PairPre p;
    p.d = d;
    p.hi_row = la > lb;
    p.diff = p.hi_row ? (sa - sb) : (sb - sa);
    p.on = in_range && (la != lb) && (d > 0);
    return p;
}
__device__ __forceinline__ double2 pair_fin(const PairPre &p, double rho /* LambdaMART.java:383 */)
{
    const double x = rho * p.d, y = rho * (1.0 - rho) * p.d;                       // :384, :387
    return make_double2(p.on ? (p.hi_row ? x : -x) : 0.0, p.on ? (p.hi_row ? y : -y) : 0.0);
}
__device__ __forceinline__ double2 pair_term_delta(bool in_range, float la, float lb, double d, double sa, double sb)
{
    const PairPre p = pair_pre_delta(in_range, la, lb, d, sa, sb);
    return pair_fin(p, rho_fdlibm(p.diff));
}

// |changes[a][b]| of ERRScorer.swapChange (metric/ERRScorer.java:91-112) from the tables of the top `size` positions.  The Java's
// labels[] / R[] / np[] stay 0 past `size`, its k-loop past `size` only adds p * 0 (+-0, or NaN once p is infinite) and multiplies by 1,
// and its last term is 0 / (b + 1) once np[b - 1] is 0: for every b > size the value is the same, so b == size + 1 stands for all of them.
__device__ double err_swap_abs(const int *top_rel, const double *top_R, const double *top_np, int size, int a, int b)
{
    const int la = top_rel[a], lb = (b < size) ? top_rel[b] : 0;
    if (la == lb) return 0.0;
    const double Ra = top_R[a], Rb = (b < size) ? top_R[b] : 0.0;
    const double base = (a == 0) ? 1.0 : top_np[a - 1];
    const double v1 = 1.0 / (a + 1) * base;
    double change = v1 * (Rb - Ra);
    double p = base * (Ra - Rb);
    const int kend = min(b, size);
    for (int k = a + 1; k < kend; k++) { const double Rk = top_R[k]; change += p * Rk / (1 + k); p *= 1.0 - Rk; }
    if (b > kend) change += p * 0.0;         // iterations past `size`: +-0, or NaN once p has overflowed (labels whose R exceeds 1 square |p| at every position)
    const double npb = (b - 1 < size) ? top_np[b - 1] : 0.0;
    change += (npb * (1.0 - Rb) * Ra / (1.0 - Ra) - npb * Rb) / (b + 1);
    return fabs(change);
}

// extra LDS of the ERR / MAP variants behind the K * 24 bytes of top-position tables
__host__ __device__ inline size_t lambda_fused_extra_bytes(int mode, int K, int bt)
{
    return mode == 1 ? ((size_t)2 * K + (size_t)K * (K + 2)) * 8 : mode == 2 ? (size_t)bt * 8 + (((size_t)K * 4 + 7) & ~(size_t)7) : 0;     // (P, RR: none)
}

// 1.0 / (p + 1) of every position the fused kernel can hold in its top tables (p < kLambdaFusedMaxK): the compiler's correctly rounded constants are the
// quotients the Java computes (ReciprocalRankScorer.java:73,78,80,90,102)
static_assert(kLambdaFusedMaxK == 16, "kInvPos covers the top positions of the fused lambda kernel");
__constant__ double kInvPos[16] = {1.0 / 1, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5, 1.0 / 6, 1.0 / 7, 1.0 / 8, 1.0 / 9, 1.0 / 10, 1.0 / 11, 1.0 / 12, 1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16};

// LDS of the compacted pair lists (CP) behind the top-position tables: gains [K] + one list of K * 64 two-byte entries per wavefront
__host__ __device__ inline size_t lambda_fused_cp_bytes(int K, int bt) { return (size_t)K * 8 + (size_t)2 * K * bt; }

// MODE 0: NDCG / DCG (the swap change is one expression of the pair).
// MODE 1: ERR.  The swap change of (a, b) depends on b only up to position `size`: a [size][size + 2] table per query, filled once
//         by the first threads in the Java's own operation order (err_swap_abs), replaces the scorer's inner loop.
// MODE 2: MAP.  The Java's loop over the relevant documents between a and b is a PREFIX of one sequential chain per row a (its
//         start and its sign depend on the row's own label only, APScorer.java:145-159): the row's owner walks the chain once and leaves
//         the running value in the term matrix, column b closes it with its own last term.
// MODE 3: P.    |change| is one value per list, (double)(1.0f / size), for the pairs a < size <= b whose binary relevances differ (PrecisionScorer.java:57-77).
// MODE 4: RR.   Every non-zero entry of ReciprocalRankScorer.swapChange (:48-107) is |1 / (p + 1) - rr| for a top position p (the row, the column, or
//         secondRank) or rr itself: the reciprocals are constants (kInvPos), firstRank / secondRank / rr scalars of the wavefront, selects per pair.
// CP (MODE 0): the pair terms are generated from per-wavefront LISTS of the active pairs instead of column by row.  A pair (a, b) contributes
// only when its labels differ (LambdaMART.java:376) -- on MSLR-like labels four visits in ten are pairs of equal labels, and the branch-free
// term costs them the same ~140 instructions as the others.  Every wavefront compacts the active (row, column) pairs of its own 64 columns
// (one ballot per row; entry = higher-label flag | row | lane, 2 bytes), zeroes its columns of the term matrix, and then walks the list 64
// entries at a time, two entries per lane in flight: the column's values come from the owning lane through ds_bpermute, the row's from the
// top-position tables.  The terms and the matrix are the same values; only who computes which entry changes.  No block barrier is added: a
// wavefront only reads what it wrote itself.
template <int BT, int MODE, bool CP = false>
__global__ __launch_bounds__(BT) void k_lambda_fused(const LamArgs g, const int *qlist, int nq)
{
    static_assert(!CP || MODE == 0, "compacted pair lists: NDCG / DCG only");
    extern __shared__ unsigned char smem_raw[];
    if ((int)blockIdx.x >= nq) return;
    const int q = qlist ? qlist[blockIdx.x] : blockIdx.x;
    const int K = g.K;
    // [K][BT + 8]: eight zero columns behind every row let the row owners read whole batches of 8 without bounds tests
    // (columns past the end of the query hold (0, 0) anyway: their threads have na == 0)
    constexpr int MS = BT + 8;
    double2 *M = (double2 *)smem_raw;
    double *top_s = (double *)(M + (size_t)K * MS);     // [K]
    float *top_l = (float *)(top_s + K);                // [K]
    int *top_rel = (int *)(top_l + K);                  // [K]
    double *top_d = (double *)(top_rel + K);            // [K] discounts of the top positions (offset K*(BT+8)*16 + 16K: 8-byte aligned)
    double *x_a = top_d + K;                            // ERR: R[] of the top positions [K]          MAP: 1 / (b + 1) of the tile's relevant documents [BT]
    double *x_b = x_a + K;                              // ERR: np[] of the top positions [K]
    double *x_D = x_b + K;                              // ERR: |swap change| [K][K + 2]
    int *top_ra = (int *)(x_a + BT);                    // MAP: relCount[] of the top positions [K]
    double *top_g = x_a;                                // CP: gains of the top positions [K]
    unsigned short *plist = (unsigned short *)(top_g + K) + (size_t)(threadIdx.x >> 6) * ((size_t)K * 64);     // CP: this wavefront's pair list [K * 64]
    const int KD = K + 2;
    const int tid = threadIdx.x;
    const int cur = g.qoff[q], n = g.qoff[q + 1] - cur;
    const int size = (n > g.k) ? g.k : n;               // NDCGScorer.java:133
    const double ideal = g.ideal ? g.ideal[q] : 1.0;         // DCG: no normalisation (x / 1.0 == x)
    const bool ideal_pos = ideal > 0;
    const double ideal_div = ideal_pos ? ideal : 1.0;
    const double ideal_r2 = lambda_div_fast(ideal_div) ? rcp_newton2(ideal_div) : 0.0;
    // one batch of global loads for everything the first tile needs
    float lb0 = 0.f; double sb0 = 0.0, db0 = 0.0; int rel0 = 0, sidx0 = 0;
    if (tid < n) { lb0 = g.sl[cur + tid]; sb0 = g.ss[cur + tid]; rel0 = g.srel[cur + tid]; sidx0 = g.sidx[cur + tid]; db0 = g.disc[tid]; }
    if (tid < size) { top_s[tid] = sb0; top_l[tid] = lb0; top_rel[tid] = rel0; top_d[tid] = db0; if (CP) top_g[tid] = gain_of(rel0); }
    int rb0 = 0, rd = 0;
    if constexpr (MODE == 1) { if (tid < size) { x_a[tid] = g.aux_a[cur + tid]; x_b[tid] = g.aux_b[cur + tid]; } }
    if constexpr (MODE == 2) {
        if (tid < n) rb0 = g.aux_i[cur + tid];
        if (tid < size) top_ra[tid] = rb0;
        rd = (n > 0) ? g.aux_i[cur + n - 1] : 0;        // rdCount: relevant documents of the list, or the judgment file's count (APScorer.java:124-133)
        if (g.rd_ext && rd != 0) rd = g.rd_ext[q];      // (count == 0: all changes are 0 either way, :141-143)
    }
    const double p_unit = (MODE == 3) ? (double)(1.0f / (float)size) : 0.0;      // P: PrecisionScorer.java:73, ((float) c) / size with c = +-1
    int rr_first = -1, rr_second = -1, rr_feff = size; double rr = 0.0, rr_vs = 0.0;
    for (int i = tid; i < K * 8; i += BT) M[(size_t)(i >> 3) * MS + BT + (i & 7)] = make_double2(0.0, 0.0);
    __syncthreads();
    if constexpr (MODE == 4) {
        // RR: firstRank / secondRank (ReciprocalRankScorer.java:49-61) from one ballot over the top labels, by every wavefront for itself: the results
        // are scalars, and every 1.0 / (p + 1) the swap change needs has p < size <= 16 -- a table of constants, no division and no load chain
        // in front of the pair loop (the first version read the rank kernel's aux_i and divided three times per thread: measured, DESIGN.md 21)
        const int l = tid & 63;
        const unsigned long long m = __ballot(l < size && top_l[min(l, K - 1)] > 0.f);
        const unsigned long long m2 = m & (m - 1);
        rr_first = __ffsll(m) - 1; rr_second = __ffsll(m2) - 1;                // (-1: none)
        if (rr_first != -1) { rr = kInvPos[rr_first]; rr_feff = rr_first; }     // :70-73, :95
        if (rr_second != -1) rr_vs = fabs(kInvPos[rr_second] - rr);
    }
    if constexpr (MODE == 1) {
        for (int e = tid; e < size * KD; e += BT) { const int a = e / KD, cb = e - a * KD; x_D[e] = (cb > a) ? err_swap_abs(top_rel, x_a, x_b, size, a, cb) : 0.0; }
        __syncthreads();
    }
    double chain = 0.0;                                 // MODE 2: the running value of this owner's chain
    const int ntiles = (n + BT - 1) / BT;
    double acc_o = 0.0, w_col = 0.0, wmax = 0.0;      // acc_o: the owner chain of this lane (lambda on lanes < size, weight on the next `size` lanes)
    // Sweep 1 SUBTRACTS on the lambda chain (acc -= m) and adds on the weight chain.  The lambda lanes carry the NEGATED accumulator through it:
    // -(acc - m) == (-acc) + m bit for bit (round-to-nearest is symmetric), so both kinds of lane run the same `acc += m` -- the sign flip of every
    // term was a fourth instruction per entry of an issue-bound loop.  `0.0 - acc` brings it back (and turns the -0.0 of a negated +0.0 into +0.0).
    // NaN keeps the sign the un-negated chain would give it (the tests compare the overflow regime of ERR bit for bit, NaNs included): a NaN that
    // enters the sweep comes back as it was; one generated inside it (Infinity - Infinity) is the hardware's default NaN either way and is not flipped.
    const bool lam_lane = tid < size;
    double acc_keep = 0.0; bool acc_nan_in = false;
    auto neg_in = [&](double &acc) { acc_keep = acc; acc_nan_in = acc != acc; acc = -acc; };
    auto neg_out = [&](double &acc) { acc = acc_nan_in ? acc_keep : ((acc != acc) ? acc : 0.0 - acc); };
    const bool one_tile = ntiles == 1;
    for (int sweep = 0; sweep < (one_tile ? 1 : 2); sweep++) {
        for (int tile = 0; tile < ntiles; tile++) {
            const int b = tile * BT + tid;
            const bool valid = b < n;
            const int na = valid ? min(b, size) : 0;
            int sidx_b = sidx0;
            if (sweep == 0 || ntiles > 1) {
                float lb = 0.f; double sb = 0.0, gb = 0.0, db = 0.0;
                if (tile == 0) { lb = lb0; sb = sb0; gb = gain_of(rel0); db = db0; }
                else if (valid) { lb = g.sl[cur + b]; sb = g.ss[cur + b]; gb = gain_of(g.srel[cur + b]); db = g.disc[b]; sidx_b = g.sidx[cur + b]; }
                if constexpr (MODE == 0 && CP) {
                    const int lane = tid & 63;
                    int L = 0;                                      // wave-uniform: ballots and their population counts are scalar
                    for (int a = 0; a < size; a++) {
                        const float la = top_l[a];
                        const bool act = a < na && ideal_pos && la != lb;
                        const unsigned long long m = __ballot(act);
                        const int pos = L + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                        if (act) plist[pos] = (unsigned short)((la > lb ? 0x8000u : 0u) | ((unsigned)a << 6) | (unsigned)lane);
                        L += __popcll(m);
                        M[(size_t)a * MS + tid] = make_double2(0.0, 0.0);
                    }
                    group_sync<kWave>();
                    double2 *Mw = M + (tid & ~63);
                    auto walk = [&](auto dfc) {
                        constexpr bool DF = decltype(dfc)::value;
                        auto cp_pre = [&](const unsigned e) -> PairPre {
                            const int a = (int)((e >> 6) & 15u), l = (int)(e & 63u);
                            const double cs = __shfl(sb, l), cd = __shfl(db, l), cg = __shfl(gb, l);
                            const double nd = (top_d[a] - cd) * (top_g[a] - cg);                      // NDCGScorer.java:154
                            const double ts = top_s[a];
                            PairPre p;
                            p.d = fabs(DF ? div_by_rcp(nd, ideal_div, ideal_r2) : nd / ideal_div);
                            p.hi_row = (e & 0x8000u) != 0;
                            p.diff = p.hi_row ? (ts - cs) : (cs - ts);                                // modelScores[high] - modelScores[low]
                            p.on = p.d > 0;                                                           // (in range, ideal > 0, labels differ: it is on the list)
                            return p;
                        };
                        int i0 = 0;
                        for (; i0 + 64 < L; i0 += 128) {                // two entries per lane: two independent exp / division chains in flight
                            const int iB = i0 + 64 + lane;
                            const unsigned eA = plist[i0 + lane], eB = plist[min(iB, L - 1)];
                            const PairPre pA = cp_pre(eA), pB = cp_pre(eB);
                            double rA, rB;
                            rho_fdlibm2(pA.diff, pB.diff, rA, rB);
                            Mw[(size_t)((eA >> 6) & 15u) * MS + (eA & 63u)] = pair_fin(pA, rA);
                            if (iB < L) Mw[(size_t)((eB >> 6) & 15u) * MS + (eB & 63u)] = pair_fin(pB, rB);
                        }
                        if (i0 < L) {
                            const int iA = i0 + lane;
                            const unsigned eA = plist[min(iA, L - 1)];
                            const PairPre pA = cp_pre(eA);
                            const double2 tA = pair_fin(pA, rho_fdlibm(pA.diff));
                            if (iA < L) Mw[(size_t)((eA >> 6) & 15u) * MS + (eA & 63u)] = tA;
                        }
                    };
                    if (ideal_r2 != 0.0) walk(std::true_type{}); else walk(std::false_type{});
                } else if constexpr (MODE == 0) {
                    auto gen = [&](auto dfc) {
                        constexpr bool DF = decltype(dfc)::value;
                        auto rows = [&](auto rc, const int a) {
                            constexpr int R = decltype(rc)::value;
                            PairPre pp[R]; double xs[R], rs[R];
#pragma unroll
                            for (int u = 0; u < R; u++) {
                                pp[u] = pair_pre_signed<DF>(a + u < na, ideal_pos, ideal_div, ideal_r2, top_l[a + u], lb, top_d[a + u], db, gain_of(top_rel[a + u]), gb, top_s[a + u], sb);
                                xs[u] = pp[u].diff;
                            }
                            rho_fdlibm_n<R>(xs, rs);
#pragma unroll
                            for (int u = 0; u < R; u++) M[(size_t)(a + u) * MS + tid] = pair_fin(pp[u], rs[u]);
                        };
                        int a = 0;
                        if constexpr (RL_LAMBDA_ROWS > 2) for (; a + RL_LAMBDA_ROWS <= size; a += RL_LAMBDA_ROWS) rows(std::integral_constant<int, RL_LAMBDA_ROWS>{}, a);
                        for (; a + 2 <= size; a += 2) rows(std::integral_constant<int, 2>{}, a);
                        if (a < size) rows(std::integral_constant<int, 1>{}, a);
                    };
                    if (ideal_r2 != 0.0) gen(std::true_type{}); else gen(std::false_type{});
                } else if constexpr (MODE == 1) {
                    const double *Dcol = x_D + min(b, size + 1);
                    int a = 0;
                    for (; a + 2 <= size; a += 2) {
                        const PairPre p0 = pair_pre_delta(a < na, top_l[a], lb, Dcol[a * KD], top_s[a], sb);
                        const PairPre p1 = pair_pre_delta(a + 1 < na, top_l[a + 1], lb, Dcol[(a + 1) * KD], top_s[a + 1], sb);
                        double r0, r1;
                        rho_fdlibm2(p0.diff, p1.diff, r0, r1);
                        M[(size_t)a * MS + tid] = pair_fin(p0, r0); M[(size_t)(a + 1) * MS + tid] = pair_fin(p1, r1);
                    }
                    if (a < size) M[(size_t)a * MS + tid] = pair_term_delta(a < na, top_l[a], lb, Dcol[a * KD], top_s[a], sb);
                } else if constexpr (MODE == 3 || MODE == 4) {
                    // what the column brings to its pairs, once: the swap change of a pair is then a few compares and selects of its row
                    const bool relb = lb > 0.f;
                    const bool p_below = b >= size;                                             // P: the column is past the cutoff
                    const bool rr_c3 = relb && b >= rr_feff;                                    // RR :99-105: rows above firstRank against a relevant column
                    const bool rr_c12 = rr_first != -1 && (int)lb == 0;                         // RR :74-93: the row firstRank against a "non-relevant" column
                    double rr_top = 0.0;                                                        // |1.0 / (b + 1) - rr| of a column among the top positions
                    if constexpr (MODE == 4) { if (b < size) rr_top = fabs(kInvPos[b] - rr); }
                    const double rr_col = (b < size) ? ((rr_second == -1 || b < rr_second) ? rr_top : rr_vs)       // :77-81
                                                     : ((rr_second == -1) ? rr : rr_vs);                           // :87-91  (|-rr| == rr)
                    auto delta = [&](const int a) -> double {
                        if constexpr (MODE == 3) return (p_below && (top_l[a] > 0.f) != relb) ? p_unit : 0.0;
                        else return (rr_c3 && a < rr_feff) ? fabs(kInvPos[a] - rr) : ((rr_c12 && a == rr_first) ? rr_col : 0.0);   // the third loop is the last writer
                    };
                    int a = 0;
                    for (; a + 2 <= size; a += 2) {
                        const PairPre p0 = pair_pre_delta(a < na, top_l[a], lb, delta(a), top_s[a], sb);
                        const PairPre p1 = pair_pre_delta(a + 1 < na, top_l[a + 1], lb, delta(a + 1), top_s[a + 1], sb);
                        double r0, r1;
                        rho_fdlibm2(p0.diff, p1.diff, r0, r1);
                        M[(size_t)a * MS + tid] = pair_fin(p0, r0); M[(size_t)(a + 1) * MS + tid] = pair_fin(p1, r1);
                    }
                    if (a < size) M[(size_t)a * MS + tid] = pair_term_delta(a < na, top_l[a], lb, delta(a), top_s[a], sb);
                } else {
                    const bool relb = valid && lb > 0.f;
                    const int rb = (tile == 0) ? rb0 : (valid ? g.aux_i[cur + b] : 0);
                    x_a[tid] = relb ? 1.0 / (b + 1) : 0.0;                  // == |((double)diff) / (k + 1)|; a skipped document adds 0.0
                    __syncthreads();
                    if (tid < size) {
                        const int a = tid;
                        const bool neg = top_l[a] > 0.f;                    // labels[a] == 1: every active pair of the row has diff == -1
                        if (tile == 0) chain = neg ? ((double)(-top_ra[a])) / (a + 1) : ((double)(top_ra[a] + 1)) / (a + 1);      // :150
                        const int l0 = max(0, a + 1 - tile * BT), l1 = min(BT, n - tile * BT);
                        for (int l = l0; l < l1; l++) { M[(size_t)a * MS + l].x = chain; const double cc = x_a[l]; chain = neg ? chain - cc : chain + cc; }   // :151-155
                    }
                    __syncthreads();
                    for (int a = 0; a < size; a++) {
                        const bool rela = top_l[a] > 0.f;
                        double d = 0.0;
                        if (a < na && rela != relb && rd > 0) {
                            const int diff = (int)relb - (int)rela;
                            const double change = M[(size_t)a * MS + tid].x + ((double)(-rb * diff)) / (b + 1);                   // :156
                            d = fabs(change / rd);                                                                                  // :159
                        }
                        M[(size_t)a * MS + tid] = pair_term_delta(a < na, top_l[a], lb, d, top_s[a], sb);
                    }
                }
            }
            __syncthreads();
            if (sweep == 0 && valid) {          // this document's own column: j < b (it is the lower label), then j == b against k < b
                // The column runs over all `size` rows, four LDS reads in flight: rows from na on hold (0, 0) for this column (pair_term_*: out of
                // range), and adding +0.0 to these sums is exact (they are never -0.0) -- a loop to the thread's own na read one entry, waited for the
                // LDS, added, 2 na times per document: as many wavefront cycles as the pair terms themselves.
                double lam = 0.0, w = 0.0;
#pragma unroll 1
                for (int a0 = 0; a0 < size; a0 += 4) {
                    double2 tq[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) tq[u] = (a0 + u < size) ? M[(size_t)(a0 + u) * MS + tid] : make_double2(0.0, 0.0);
#pragma unroll
                    for (int u = 0; u < 4; u++) { lam -= fmax(tq[u].x, 0.0); w += fmax(tq[u].y, 0.0); }
                }
#pragma unroll 1
                for (int a0 = 0; a0 < size; a0 += 4) {
                    double2 tq[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) tq[u] = (a0 + u < size) ? M[(size_t)(a0 + u) * MS + tid] : make_double2(0.0, 0.0);
#pragma unroll
                    for (int u = 0; u < 4; u++) { lam += fmax(-tq[u].x, 0.0); w += fmax(-tq[u].y, 0.0); }
                }
                if (b >= size) {
                    const int o = cur + sidx_b;
                    g.lw[o] = make_double2(lam, w);
                    wmax = fmax(wmax, fabs(lam));
                } else { acc_o = lam; w_col = w; }
            }
            // Row owners.  The ordered sums of a top document are two dependent f64 chains (lambda and weight) that only its
            // owner can run; the loop is bound by instruction issue with 10 of 64 lanes busy, so the two chains of an owner sit
            // on two lanes (lane a: lambda, lane size + a: weight): 3-4 instructions per term instead of 5.
            if (tile == 0 && sweep == 0) {      // the weight lanes pick up the column part their owner just computed (wavefront 0)
                const double wv = __shfl(w_col, (tid - size) & 63);
                if (tid >= size && tid < 2 * size) acc_o = wv;
            }
            if (tid < 2 * size) {               // ranked positions after the owner's own, in order
                const int a = tid < size ? tid : tid - size;
                const int l0 = max(0, a + 1 - tile * BT), l1 = min(BT, n - tile * BT);
                const double *row = (const double *)(M + (size_t)a * MS) + (tid < size ? 0 : 1);
                // (requesting the next batch of eight before the current one is added was built and measured SLOWER, profiles/r05i_ab_owner_walk_c2.txt:
                // the loop is bound by instruction issue, and the selects / copies of a second register set are more of it)
                auto walk = [&](const int sw) {
                    for (int l = l0; l < l1; l += 8) {
                        double tt[8];
#pragma unroll
                        for (int u = 0; u < 8; u++) tt[u] = row[2 * (l + u)];
                        if (sw == 0) {
#pragma unroll
                            for (int u = 0; u < 8; u++) acc_o += fmax(tt[u], 0.0);
                        } else {                // lambda: acc -= m, weight: acc += m;  a - m == a + (-m) exactly
#pragma unroll
                            for (int u = 0; u < 8; u++) acc_o += fmax(-tt[u], 0.0);
                        }
                    }
                };
                if (sweep == 1 && tile == 0 && lam_lane) neg_in(acc_o);
                walk(sweep);
                if (one_tile) {                 // a list of one tile: the second sweep reads the same matrix -- no second pass over the tiles, no barriers in between
                    if (lam_lane) neg_in(acc_o);
                    walk(1);
                    if (lam_lane) neg_out(acc_o);
                } else if (sweep == 1 && tile == ntiles - 1 && lam_lane) neg_out(acc_o);
            }
            __syncthreads();
        }
    }
    {
        const double w_fin = __shfl(acc_o, (tid + size) & 63);      // the weight chain of owner `tid` ended on lane size + tid
        if (tid < size) {
            const int o = cur + sidx0;
            g.lw[o] = make_double2(acc_o, w_fin);
            wmax = fmax(wmax, fabs(acc_o));
        }
    }
    block_store_max(wmax, g.blockmax);
}

// The same for lists of at most 16 documents (the "~10 documents per query" shape): a 16-lane group per query, four queries
// per wavefront, sixteen per block -- a block-per-query launch leaves 54 of 64 lanes idle on such lists.  One tile, so the
// terms are generated once; the groups of a wavefront only meet at wave-level barriers.
constexpr int kLambdaTinyDocs = 16, kLambdaTinyGroups = 16;
__host__ __device__ inline size_t lambda_tiny_group_bytes(int K) { return (((size_t)K * kLambdaTinyDocs * 16 + (size_t)K * 24) + 15) & ~(size_t)15; }
__global__ __launch_bounds__(kLambdaTinyDocs * kLambdaTinyGroups) void k_lambda_tiny(const LamArgs g, const int *qlist, int nq)
{
    extern __shared__ unsigned char smem_raw[];
    constexpr int MS = kLambdaTinyDocs;
    const int K = g.K;
    const int grp = threadIdx.x / kLambdaTinyDocs, gl = threadIdx.x % kLambdaTinyDocs;
    const int slot = blockIdx.x * kLambdaTinyGroups + grp;
    const bool has = slot < nq;
    const int q = has ? qlist[slot] : 0;
    const size_t per_group = lambda_tiny_group_bytes(K);
    unsigned char *gb = smem_raw + (size_t)grp * per_group;
    double2 *M = (double2 *)gb;                         // [K][16] signed pair terms (see k_lambda_fused)
    double *top_s = (double *)(M + (size_t)K * MS);     // [K]
    double *top_d = top_s + K;                          // [K]
    float *top_l = (float *)(top_d + K);                // [K]
    int *top_rel = (int *)(top_l + K);                  // [K]
    const int cur = has ? g.qoff[q] : 0, n = has ? g.qoff[q + 1] - cur : 0;
    const int size = (n > g.k) ? g.k : n;
    const double ideal = (has && g.ideal) ? g.ideal[q] : 1.0;
    const bool ideal_pos = ideal > 0;
    const double ideal_div = ideal_pos ? ideal : 1.0;
    const double ideal_r2 = lambda_div_fast(ideal_div) ? rcp_newton2(ideal_div) : 0.0;
    const int b = gl;
    const bool valid = b < n;
    float lb = 0.f; double sb = 0.0, db = 0.0; int rel = 0, sidx = 0;
    if (valid) { lb = g.sl[cur + b]; sb = g.ss[cur + b]; rel = g.srel[cur + b]; sidx = g.sidx[cur + b]; db = g.disc[b]; }
    if (b < size) { top_s[b] = sb; top_l[b] = lb; top_rel[b] = rel; top_d[b] = db; }
    group_sync<kWave>();
    const int na = valid ? min(b, size) : 0;
    const double gbn = gain_of(rel);
    // (four lists per wavefront: the reciprocal form only when every list of the wavefront is in its range -- the compiler's division is always right)
    auto gen = [&](auto dfc) {
        constexpr bool DF = decltype(dfc)::value;
        int a = 0;
        for (; a + 2 <= size; a += 2) {
            const PairPre p0 = pair_pre_signed<DF>(a < na, ideal_pos, ideal_div, ideal_r2, top_l[a], lb, top_d[a], db, gain_of(top_rel[a]), gbn, top_s[a], sb);
            const PairPre p1 = pair_pre_signed<DF>(a + 1 < na, ideal_pos, ideal_div, ideal_r2, top_l[a + 1], lb, top_d[a + 1], db, gain_of(top_rel[a + 1]), gbn, top_s[a + 1], sb);
            double r0, r1;
            rho_fdlibm2(p0.diff, p1.diff, r0, r1);
            M[(size_t)a * MS + b] = pair_fin(p0, r0); M[(size_t)(a + 1) * MS + b] = pair_fin(p1, r1);
        }
        if (a < size) {
            const PairPre p0 = pair_pre_signed<DF>(a < na, ideal_pos, ideal_div, ideal_r2, top_l[a], lb, top_d[a], db, gain_of(top_rel[a]), gbn, top_s[a], sb);
            M[(size_t)a * MS + b] = pair_fin(p0, rho_fdlibm(p0.diff));
        }
    };
    if (__all(ideal_r2 != 0.0)) gen(std::true_type{}); else gen(std::false_type{});
    group_sync<kWave>();
    double wmax = 0.0;
    if (valid) {
        // this document's own column: j < b (it is the lower label), then j == b against k < b (LambdaMART.java:371-393)
        double lam = 0.0, w = 0.0;
        for (int a = 0; a < na; a++) { const double2 t = M[(size_t)a * MS + b]; lam -= fmax(t.x, 0.0); w += fmax(t.y, 0.0); }
        for (int a = 0; a < na; a++) { const double2 t = M[(size_t)a * MS + b]; lam += fmax(-t.x, 0.0); w += fmax(-t.y, 0.0); }
        if (b < size) {         // row owner: ranked positions after its own, in order: first as the higher label, then as the lower one
            const double2 *row = M + (size_t)b * MS;
            for (int l = b + 1; l < n; l++) { lam += fmax(row[l].x, 0.0); w += fmax(row[l].y, 0.0); }
            for (int l = b + 1; l < n; l++) { lam -= fmax(-row[l].x, 0.0); w += fmax(-row[l].y, 0.0); }
        }
        g.lw[cur + sidx] = make_double2(lam, w);
        wmax = fabs(lam);
    }
    block_store_max(wmax, g.blockmax);
}

// exp probe for the tests: out[i] = exp_fdlibm_bf(x[i]) and the reference-path exp_fdlibm(x[i])
__global__ void k_exp_probe(const double *x, int n, double *out_bf, double *out_ref)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out_bf[i] = exp_fdlibm_bf(x[i]); out_ref[i] = exp_fdlibm(x[i]); }
}

// rho probe for the tests: out_fast[i] = rho_fdlibm(x[i]) (the lambda kernels' form), out_ref[i] = 1.0 / (1 + exp_fdlibm(x[i])) with the compiler's division
__global__ void k_rho_probe(const double *x, int n, double *out_fast, double *out_ref)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out_fast[i] = rho_fdlibm(x[i]); out_ref[i] = 1.0 / (1 + exp_fdlibm(x[i])); }
}
// division probe: out_fast[i] = div_by_rcp(num[i], den[i], rcp_newton2(den[i])), out_ref[i] = num[i] / den[i]
__global__ void k_div_probe(const double *num, const double *den, int n, double *out_fast, double *out_ref)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out_fast[i] = div_by_rcp(num[i], den[i], rcp_newton2(den[i])); out_ref[i] = num[i] / den[i]; }
}

// MART.computePseudoResponses (learning/tree/MART.java:47-51): pseudoResponses[i] = label - modelScores[i]
__global__ __launch_bounds__(kThreads) void k_mart_residual(const float *labels, const double *scores, double2 *lw, int N,
                                                            double *blockmax)
{
    double wmax = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < N; i += gridDim.x * kThreads) {
        const double r = (double)labels[i] - scores[i];
        lw[i] = make_double2(r, 0.0);
        wmax = fmax(wmax, fabs(r));
    }
    block_store_max(wmax, blockmax);
}

// ------------------------------------------------------------------------------------------------
// K1b: fixed-point quantisation.  q = rint(lambda * 2^E) with E chosen from max|lambda| so that one LDS
// accumulator (<= 2^kLog2Chunk addends) cannot overflow int64.  Integer sums are associative: every
// histogram value below is independent of accumulation order, thread count and GPU count.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void quant_exponents(unsigned long long maxbits, int N, int &E, int &E2)
{
    if (maxbits == 0) { E = 0; E2 = 0; return; }
    const double m = bits2d(maxbits);
    const int M = ilogb(m) + 1;                      // m < 2^M
    int lgN = 0;
    while ((1LL << lgN) < (long long)N + 1) lgN++;
    E = 62 - kLog2Chunk - M;
    E2 = 61 - lgN - 2 * M;
}

// (long long)rint(x) for |x| < 2^51 by one addition: x + 1.5 * 2^52 is rounded to an integer (nearest, ties to even -- the rounding of
// __double2ll_rn) and the integer sits in the low mantissa bits.  The library conversion is a dozen instructions (there is no f64 -> i64
// convert on gfx950); the root pass that quantises on the fly runs it once per document and feature group.  |q| < 2^48 by the choice of E
// (quant_exponents); r is NOT small on small data (r < 2^(61 - lg N)) and keeps the library conversion.
__device__ __forceinline__ long long rint_ll_small(double x)
{
    const double magic = 6755399441055744.0;        // 1.5 * 2^52
    return (long long)(d2bits(x + magic) - d2bits(magic));
}

__global__ __launch_bounds__(kThreads) void k_quantize(const Ctx c)
{
    int E, E2;
    quant_exponents(c.st->maxabs_bits, c.Nglobal, E, E2);      // the GLOBAL document count: lambda^2 sums are all-reduced as raw integers
    long long acc = 0;
    for (int k = blockIdx.x * kThreads + threadIdx.x; k < c.N; k += gridDim.x * kThreads) {
        const double l = c.lw[k].x;
        c.q[k] = __double2ll_rn(ldexp(l, E));
        const long long r = __double2ll_rn(ldexp(l * l, E2));
        c.r[k] = r;
        acc += r;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    __shared__ long long part[4];
    if (lane_id() == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd((unsigned long long *)&c.st->root_sq, (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
        if (blockIdx.x == 0) { c.st->E = E; c.st->E2 = E2; }
    }
}

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

// ------------------------------------------------------------------------------------------------
// K2/K3: histogram of one node.  grid = (feature groups, chunks).  A block owns FG features x one chunk of
// <= kChunk samples and accumulates them in LDS with native ds_add_u64 / ds_add_u32, then flushes its
// partial histogram (plain coalesced stores, no global atomics).  ROOT: samples are 0..N-1 and counts are
// static (FeatureHistogram.java:138 "count doesn't change").
// ------------------------------------------------------------------------------------------------
// docs per chunk for a node of `cnt` samples: big nodes use the largest chunk (least flush traffic), small
// nodes are cut finer so that a split step still spreads over the whole chip (a chunk's samples are
// processed serially by one block).  Must be identical in k_hist and k_hist_finish.
template <bool ROOT>
__device__ __forceinline__ int chunk_docs(const Ctx &c, int cnt)
{
    // a node is cut into ~node_div chunks (64 for the root pass): every chunk costs a partial histogram (F x T x 12 bytes)
    // that is flushed and read back, which outweighs the extra parallelism of finer cuts (measured at c2, same box: 64 -> 225.8, 12 -> 230.6, 8 -> 229.5, 6 -> 229.4 rounds/s)
    const int div = ROOT ? 64 : c.node_div;
    const int cs = ((cnt + div - 1) / div + 255) & ~255;
    return min(ROOT ? kChunk : c.node_chunk, max(ROOT ? kMinChunk : max(c.node_min, 256), cs));     // never 0: callers divide by it, also for empty (cnt == 0) slots
}

// gbins holds PRE-SCALED bin ids: 8 * bin = the byte offset of the bin's int64 accumulator inside its feature's LDS row.
__device__ __forceinline__ unsigned bin8_of(const uint4 &a, const uint4 &b, int fl)
{
    const unsigned w = fl < 8 ? (fl < 4 ? (fl < 2 ? a.x : a.y) : (fl < 6 ? a.z : a.w))
                              : (fl < 12 ? (fl < 10 ? b.x : b.y) : (fl < 14 ? b.z : b.w));
    return (fl & 1) ? (w >> 16) : (w & 0xffffu);
}

// Packed rows (P8; threshold tables of at most 257 entries, the -tc 256 case): a bin id is one byte plus, for the single bin that does not fit
// (bin 256: values above the last finite threshold), one bit of a 16-bit mask per (document, group): bin = byte + bit.  A (document, group)
// row is 16 + 2 bytes instead of 32: the root pass streams 170 instead of 296 bytes per document, a child's document-major row is 192 bytes
// -- two 128-byte memory lines -- instead of 384.
__device__ __forceinline__ unsigned pbin8_of(const uint4 &lo, unsigned hi, int fl)
{
    const unsigned w = fl < 8 ? (fl < 4 ? lo.x : lo.y) : (fl < 12 ? lo.z : lo.w);
    const unsigned byte = __builtin_amdgcn_ubfe(w, 8 * (fl & 3), 8), bit = __builtin_amdgcn_ubfe(hi, fl, 1);
    return (byte + bit) << 3;
}

// sum of the per-tile lambda^2 partials of a slot (exact integers: any order); every thread of the block calls it
__device__ long long slot_sq_left(const Ctx &c, const SlotRec &sl, long long *sh /* kThreads/64 */)
{
    long long v = 0;
    for (int i = threadIdx.x; i < sl.ntiles; i += blockDim.x) v += c.tile_sq[sl.tile0 + i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) r += sh[w];
    return r;
}

// slot of the growth step that owns global tile / chunk id `x` (ranges are consecutive); -1 = none.  Every start is loaded before any is looked at
// (a loop that loads the next start only after comparing the previous one is a chain of dependent memory round trips at the top of every block).
__device__ __forceinline__ int slot_of_chunk(const TreeState *st, int y)
{
    const int done = st->done, total = st->chunks_total, ns = st->nslots;
    int c0[kSpec];
#pragma unroll
    for (int i = 0; i < kSpec; i++) c0[i] = st->slot[i].chunk0;
    if (done || y >= total) return -1;
    int j = 0;
#pragma unroll
    for (int i = 1; i < kSpec; i++) j += (i < ns && y >= c0[i]) ? 1 : 0;
    return j;
}
__device__ __forceinline__ int slot_of_tile(const TreeState *st, int x)
{
    const int done = st->done, total = st->tiles_total, ns = st->nslots;
    int t0[kSpec];
#pragma unroll
    for (int i = 0; i < kSpec; i++) t0[i] = st->slot[i].tile0;
    if (done || x >= total) return -1;
    int j = 0;
#pragma unroll
    for (int i = 1; i < kSpec; i++) j += (i < ns && x >= t0[i]) ? 1 : 0;
    return j;
}

// grid = (feature groups x sub-passes, chunks).  A block owns SUB features of one group x one chunk of samples.
// Per sample it reads ONE 32-byte row gbins[group][k][0..15] (two 16-byte loads: full sectors for the sparse
// sample lists of child nodes, perfectly coalesced for the root) and the fixed-point lambda from the
// list-ordered copy ql (contiguous), then issues SUB ds_add_u64 (+ SUB ds_add_u32 on the counts of child nodes).
// The inner loop is kept to extract / compare-with-mode / LDS add per feature: bin ids arrive pre-scaled, padding
// features (their bins are 0 and their "mode" is 0) need no test, and with the usual <= 264 bins the LDS row stride is a
// compile-time constant (TSC), so every accumulator address is the extracted value plus an immediate offset.
// RUNS: the instantiation for data sets with columns that come in runs of equal bins (Ctx::runs; query-level features: the wavefront's 64
// consecutive samples share a bin, and 64 atomics on one LDS address serialise at ~5 cycles a lane).  Those columns leave the main loop and
// get a pass of their own in which the four samples of a quad that agree are folded into one atomic by DPP quad permutes (no LDS traffic).
// A separate instantiation because the larger loop body slows the ordinary columns down as well (HISTORY.md 4.1).
// NT: threads per block.  Child passes of few chunks leave most of the chip idle and are bound by the latency of the row gathers: a block of NT = 1024
// threads keeps four times as many gathers in flight per chunk (launch_hist picks NT; RLHIP_HIST_NT).
template <bool ROOT, int SUB, int TSC, bool RUNS, bool P8, int NT, bool CR, bool FQ>
__device__ __forceinline__ void hist_chunk(const Ctx &c, const TreeState *st, const int bx, const int by, unsigned long long *lsum)
{
    RL_TR_BEGIN();
    int node = 0, ychunk = by;
    int s_start = -1, s_count = 0, s_buf = 0, s_cs = 0;             // the accumulated child's list range straight from the slot (one GPU: its size is known)
    if (!ROOT) {
        const int j = slot_of_chunk(st, by);
        if (j < 0) return;
        const SlotRec sl = st->slot[j];                             // (copied whole: one batch of loads)
        node = sl.build_left ? sl.left : sl.right;                  // the smaller child (exact sums: order-free)
        ychunk = by - sl.chunk0; s_cs = sl.cs;
        if (sl.nleft >= 0) {        // saves the dependent load of the node record (written by the partition kernel with these very values)
            s_start = sl.build_left ? sl.pstart : sl.pstart + sl.nleft;
            s_count = sl.build_left ? sl.nleft : sl.pcount - sl.nleft;
            s_buf = 1 - sl.pbuf;
        }
    }
    NodeRec nd_s; nd_s.start = s_start; nd_s.count = s_count; nd_s.buf = s_buf;
    const NodeRec &nd = (ROOT || s_start < 0) ? c.nodes[node] : nd_s;
    const int cnt = ROOT ? c.N : nd.count;
    const int cs = (!ROOT && s_cs > 0) ? s_cs : chunk_docs<ROOT>(c, cnt);      // (balance_slots)
    const int p0 = ychunk * cs;
    if (p0 >= cnt) return;
    const int p1 = min(p0 + cs, cnt);
    const int TS = c.TS;
    const int LT = TSC ? TSC : TS;                  // LDS row stride (bins)
    constexpr int NSUB = kHistFG / SUB;
    const int grp = bx / NSUB, sp = bx % NSUB;
    const int fl0 = sp * SUB;                       // first feature of the group handled here
    const int f0 = grp * kHistFG + fl0;
    const int nf = min(SUB, c.F - f0);
    if (nf <= 0) return;
    const bool want_tot = (bx == 0);
    // root pass: the groups of sparse columns are accumulated from their entry lists by k_hist_sp (rl_csc.inc); block 0 still sums the
    // chunk's lambdas here (every column's mode bin is rebuilt from the chunk totals)
    const bool no_rows = ROOT && c.sp_on && c.sp_grp[grp];
    if (no_rows && !want_tot) return;
    unsigned char *lsum_b = (unsigned char *)lsum;
    unsigned char *lcnt_b = lsum_b + (size_t)SUB * LT * 8;         // one 32-bit count per bin (child nodes only)
    RL_TR_MARK(1);
    const int *idx = ROOT ? nullptr : c.idx[nd.buf] + nd.start;
    const long long *ql = ROOT ? c.q : c.ql[nd.buf] + nd.start;
    // rows of this feature group: group-major (dense passes: every byte of a memory line is used) or document-major (sparse nodes)
    const bool dm = ROOT ? (c.dm_root != 0) : (c.dm_div > 0 && (long long)cnt * c.dm_div <= (long long)c.N);
    const uint4 *rows = dm ? (const uint4 *)c.dbins + 2 * grp : (const uint4 *)(c.gbins + (size_t)grp * c.Npad * kHistFG);
    const size_t rstride = dm ? (size_t)2 * c.dm_gstride : (size_t)2;
    // packed rows: low bytes and the 16-bit mask of the group, document-major (one row per document) or group-major
    const unsigned char *plo = nullptr, *phi = nullptr; size_t plo_stride = 0, phi_stride = 0;
    if (P8) {
        if (dm) { plo = c.pdbins + 16 * grp; phi = c.pdbins + 16 * c.numFG + 2 * grp; plo_stride = phi_stride = (size_t)c.pd_stride; }
        else { plo = c.pbins + (size_t)grp * c.Npad * 16; phi = (const unsigned char *)c.phib + (size_t)grp * c.Npad * 2; plo_stride = 16; phi_stride = 2; }
    }
    // The most populated bin of a feature (zero for count-like features) is never accumulated: it would serialise
    // most lanes of a wavefront on one LDS address.  It is rebuilt exactly as (chunk total - other bins) downstream.
    // (one coalesced load by the first SUB lanes and a read-lane per feature: SUB loads of one word each were SUB dependent round trips)
    unsigned md8[SUB];
    {
        const int lj = lane_id();
        const unsigned mv = (lj < nf) ? 8u * (unsigned)c.mode[f0 + lj] : 0u;
#pragma unroll
        for (int j = 0; j < SUB; j++) md8[j] = (unsigned)__builtin_amdgcn_readlane((int)mv, j);
    }
    long long tot = 0;
    // FQ (root pass of the plain one-GPU path): the fixed-point lambdas are made HERE from the f64 lambdas -- k_quantize's pass over the documents
    // (a launch of ~38 us at c2) is gone; the blocks of feature group 0 store q / r for the child passes and sum r for the root's deviance.
    int qE = 0, qE2 = 0; long long sq_acc = 0;
    if (FQ) quant_exponents(st->maxabs_bits, c.Nglobal, qE, qE2);
    // (the extra stores are spread: group 0 stores q, group 1 -- when there is one -- r and its sum; a block that did both set the launch's tail)
    const bool fq_q = FQ && bx == 0, fq_r = FQ && bx == ((int)gridDim.x > 1 ? 1 : 0);
    constexpr int D = kHistDocs;
    const unsigned runmask = RUNS ? ((c.runs[grp] >> fl0) & ((1u << SUB) - 1u)) : 0u;      // block-uniform
    if (no_rows) {       // totals only
        for (int p = p0 + threadIdx.x; p < p1; p += NT) tot += ql[p];
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
        __shared__ long long wtot0[NT / 64];
        if (lane_id() == 0) wtot0[threadIdx.x >> 6] = tot;
        __syncthreads();
        if (threadIdx.x == 0) { long long v = 0; for (int w = 0; w < NT / 64; w++) v += wtot0[w]; c.part_tot[by] = v; }
        return;
    }
    const bool cr = CR && c.cr_grp[grp] != 0;         // block-uniform: this group's rows are compact
    int kn[D];
#pragma unroll
    for (int d = 0; d < D; d++) { const int p = p0 + threadIdx.x + d * NT; kn[d] = (p < p1) ? (ROOT ? p : idx[p]) : -1; }
    // (the LDS histogram is zeroed AFTER the first sample ids -- and the mode bins -- have been requested: behind the barrier their round trip was
    // serial set-up time of every chunk, ~1.8 us of a small child's 10-20 us block)
    for (int i = threadIdx.x; i < SUB * LT; i += NT) lsum[i] = 0;
    if (!ROOT) for (int i = threadIdx.x; i < SUB * LT; i += NT) ((unsigned *)lcnt_b)[i] = 0;
    __syncthreads();
    RL_TR_MARK(2);
    RL_TR_MARK(3);
    // One iteration's inputs (sample ids, fixed-point lambdas, bin rows) and its LDS atomics are two stages.  The root pass runs them back to back
    // (a perfectly coalesced stream, bound by the atomics).  Child passes request the rows of iteration i + 1 BEFORE the atomics of iteration i:
    // a row gather through a sample list is a ~2-us round trip, and with two blocks (eight wavefronts) on a CU -- one, in the small steps of a
    // late tree -- nothing else hides it: an iteration of 512 documents took 3.5 us for 1.3 us of LDS work.
    struct Stage { int k[D]; unsigned long long qv[D]; uint4 ra[D], rb[D]; unsigned hb[D]; };
    auto stage_load = [&](const int pb, const int (&kin)[D], Stage &S) {
        int (&k)[D] = S.k; unsigned long long (&qv)[D] = S.qv; uint4 (&ra)[D] = S.ra; uint4 (&rb)[D] = S.rb; unsigned (&hb)[D] = S.hb;
#pragma unroll
        for (int d = 0; d < D; d++) {
            k[d] = kin[d];
            const int p = pb + d * NT;
            if (FQ) {       // (ROOT: k == p; clamped, unconditional load)
                const double l = c.lw[min(p, p1 - 1)].x;
                const long long qq = rint_ll_small(ldexp(l, qE));
                qv[d] = (k[d] >= 0) ? (unsigned long long)qq : 0ull;
                if (fq_q && k[d] >= 0) c.q[p] = qq;
                if (fq_r && k[d] >= 0) {
                    const long long r = __double2ll_rn(ldexp(l * l, qE2));      // (r < 2^(61 - lg N): beyond the one-addition conversion on small data)
                    c.r[p] = r; sq_acc += r;
                }
            } else qv[d] = (k[d] >= 0) ? (unsigned long long)ql[p] : 0ull;
            tot += (long long)qv[d];
            const size_t kk = (size_t)max(k[d], 0);
            // (rb is the dense rows' second half only: a copy `rb = ra` here made the wavefront wait for document d's row before it asked for document d + 1's)
            if (CR && cr) { ra[d] = c.crows[(size_t)c.cr_stride * kk + grp]; rb[d] = make_uint4(0u, 0u, 0u, 0u); hb[d] = 0u; }      // compact row: one 16-byte request per (document, group)
            else if (P8) { ra[d] = *(const uint4 *)(plo + plo_stride * kk); hb[d] = *(const unsigned short *)(phi + phi_stride * kk); rb[d] = make_uint4(0u, 0u, 0u, 0u); }
            else { ra[d] = rows[rstride * kk]; rb[d] = rows[rstride * kk + 1]; hb[d] = 0u; }
        }
    };
    auto stage_acc = [&](const Stage &S) {
        const int (&k)[D] = S.k; const unsigned long long (&qv)[D] = S.qv; const uint4 (&ra)[D] = S.ra; const uint4 (&rb)[D] = S.rb; const unsigned (&hb)[D] = S.hb;
        if (CR && cr) {
            // Compact rows (sparse data: Ctx::crows): a (document, group) row lists the document's entries OUTSIDE the columns' mode bins -- up to eight
            // 16-bit words (column-in-group << 12 | bin), ascending, 0xffff = none -- so a row of mostly mode-bin cells costs one 16-byte request and
            // a couple of atomics instead of two requests and sixteen extract-and-compare steps.  The same atomics as the dense loop issues (the
            // mode bin is skipped there too), so the partial histograms are bit-identical.  A row with more than eight entries carries 0xfffe and
            // is read from the 32-byte dense row instead.
#pragma unroll
            for (int d = 0; d < D; d++) {
                if (k[d] < 0) continue;
                const unsigned w4[4] = {ra[d].x, ra[d].y, ra[d].z, ra[d].w};
                if ((w4[0] & 0xffffu) == 0xfffeu) {
                    const size_t kk = (size_t)k[d];
                    const uint4 *drow = (const uint4 *)c.dbins + 2 * grp + (size_t)2 * c.dm_gstride * kk;
                    const uint4 da = drow[0], db = drow[1];
#pragma unroll
                    for (int j = 0; j < SUB; j++) {
                        const unsigned t8 = bin8_of(da, db, fl0 + j);
                        if (t8 != md8[j]) {
                            atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), qv[d]);
                            if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), 1u);
                        }
                    }
                    continue;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const unsigned ent = (u & 1) ? (w4[u >> 1] >> 16) : (w4[u >> 1] & 0xffffu);
                    if (ent == 0xffffu) break;                  // entries are packed at the front
                    const unsigned j = ent >> 12, t8 = (ent & 0xfffu) << 3;
                    atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), qv[d]);
                    if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), 1u);
                }
            }
        } else
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (k[d] >= 0) {
#pragma unroll
                for (int j = 0; j < SUB; j++) {
                    if (RUNS && ((runmask >> j) & 1u)) continue;
                    const unsigned t8 = P8 ? pbin8_of(ra[d], hb[d], fl0 + j) : bin8_of(ra[d], rb[d], fl0 + j);
                    if (t8 != md8[j]) {
                        atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), qv[d]);
                        if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), 1u);
                    }
                }
            }
        }
        if (RUNS && runmask) {
#pragma unroll
            for (int d = 0; d < D; d++) {
                if (k[d] < 0) continue;
#pragma unroll
                for (int j = 0; j < SUB; j++) {
                    if (!((runmask >> j) & 1u)) continue;                   // block-uniform: a scalar branch
                    const unsigned t8 = P8 ? pbin8_of(ra[d], hb[d], fl0 + j) : bin8_of(ra[d], rb[d], fl0 + j);
                    // a neighbour that is not running (past the end of the chunk) reads as different: `old` = ~t8
                    const unsigned k1 = (unsigned)__builtin_amdgcn_update_dpp((int)~t8, (int)t8, 0xB1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
                    const unsigned k2 = (unsigned)__builtin_amdgcn_update_dpp((int)~t8, (int)t8, 0x4E, 0xf, 0xf, false);      // quad_perm [2,3,0,1]
                    const unsigned k3 = (unsigned)__builtin_amdgcn_update_dpp((int)~t8, (int)t8, 0x1B, 0xf, 0xf, false);      // quad_perm [3,2,1,0]
                    const unsigned mdj = md8[j];
                    unsigned long long add = qv[d]; unsigned cadd = 1u; bool mine = true;
                    if (t8 == k1 && t8 == k2 && t8 == k3) {
                        const unsigned lo = (unsigned)add, hi = (unsigned)(add >> 32);
                        add += ((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, 0xB1, 0xf, 0xf, false) << 32) |
                               (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xf, 0xf, false);
                        const unsigned lo1 = (unsigned)add, hi1 = (unsigned)(add >> 32);
                        add += ((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(0, (int)hi1, 0x4E, 0xf, 0xf, false) << 32) |
                               (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo1, 0x4E, 0xf, 0xf, false);
                        cadd = 4u; mine = (threadIdx.x & 3) == 0;
                    }
                    if (mine && t8 != mdj) {
                        atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), add);
                        if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), cadd);
                    }
                }
            }
        }
        };
    auto next_ids = [&](const int pb, int (&ko)[D]) {
#pragma unroll
        for (int d = 0; d < D; d++) { const int p = pb + d * NT; ko[d] = (p < p1) ? (ROOT ? p : idx[p]) : -1; }
    };
    constexpr bool PF = !ROOT && !FQ && RL_HIST_PREFETCH;
    constexpr bool PF2 = PF && RL_HIST_PREFETCH == 2;        // the two stages ping-pong between two register sets (no copy at the loop's end)
    if (PF2) {
        Stage S0, S1;
        int kB[D], kC[D];
        const int tb = p0 + (int)threadIdx.x;
        next_ids(tb + D * NT, kB);
        stage_load(tb, kn, S0);
        for (int pb = tb; pb < p1; pb += 2 * D * NT) {
            const int ub = pb - (int)threadIdx.x;           // block-uniform
            next_ids(pb + 2 * D * NT, kC);
            const bool h1 = ub + D * NT < p1;
            if (h1) stage_load(pb + D * NT, kB, S1);
            stage_acc(S0);
            if (!h1) break;
            next_ids(pb + 3 * D * NT, kB);
            if (ub + 2 * D * NT < p1) stage_load(pb + 2 * D * NT, kC, S0);
            stage_acc(S1);
        }
    } else if (!PF) {
        for (int pb = p0 + threadIdx.x; pb < p1; pb += D * NT) {
            Stage S;
            stage_load(pb, kn, S);
            next_ids(pb + D * NT, kn);
            stage_acc(S);
        }
    } else {
        Stage S0, S1;
        int k2[D];
        next_ids(p0 + (int)threadIdx.x + D * NT, k2);       // (kn: iteration 0, k2: iteration 1)
        stage_load(p0 + (int)threadIdx.x, kn, S0);
        for (int pb = p0 + threadIdx.x; pb < p1; pb += D * NT) {
            int k3[D];
            next_ids(pb + 2 * D * NT, k3);
            if (pb - (int)threadIdx.x + D * NT < p1) stage_load(pb + D * NT, k2, S1);      // (block-uniform)
            stage_acc(S0);
            S0 = S1;
#pragma unroll
            for (int d = 0; d < D; d++) k2[d] = k3[d];
        }
    }
    RL_TR_MARK(4);
    if (want_tot) {         // sum of q over the chunk (|q| < 2^48, <= 2^14 samples: fits int64)
        tot = (long long)wave_sum_u64((unsigned long long)tot);
        __shared__ long long wtot[NT / 64];
        if (lane_id() == 0) wtot[threadIdx.x >> 6] = tot;
        __syncthreads();
        if (threadIdx.x == 0) { long long v = 0; for (int w = 0; w < NT / 64; w++) v += wtot[w]; c.part_tot[by] = v; }
        if (FQ && threadIdx.x == 0 && by == 0) { c.st->E = qE; c.st->E2 = qE2; }
    }
    if (fq_r) {       // the root's sum of r (k_quantize's tail)
        for (int o = 32; o > 0; o >>= 1) sq_acc += __shfl_xor(sq_acc, o);
        __shared__ long long wsq[NT / 64];
        if (lane_id() == 0) wsq[threadIdx.x >> 6] = sq_acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long v = 0; for (int w = 0; w < NT / 64; w++) v += wsq[w];
            atomicAdd((unsigned long long *)&c.st->root_sq, (unsigned long long)v);
        }
    }
    __syncthreads();
    RL_TR_MARK(5);
    long long *ps = c.part_sum + ((size_t)by * c.F + f0) * TS;
    int *pc = c.part_cnt + ((size_t)by * c.F + f0) * TS;
    if (TSC) {       // (LT is a compile-time constant: no run-time division per element)
        for (int i = threadIdx.x; i < nf * LT; i += NT) {
            const int j = i / LT, t = i - j * LT;
            if (t < TS) {
                ps[j * TS + t] = (long long)lsum[i];
                if (!ROOT) pc[j * TS + t] = (int)((const unsigned *)lcnt_b)[i];
            }
        }
    } else
    for (int i = threadIdx.x; i < nf * TS; i += NT) {
        const int j = i / TS, t = i - j * TS;
        ps[i] = (long long)lsum[j * LT + t];
        if (!ROOT) pc[i] = (int)((const unsigned *)lcnt_b)[j * LT + t];
    }
    if (!ROOT) RL_TR_END(1, by * (int)gridDim.x + bx);
}


// Child passes run on a BOUNDED grid (launch_hist: about one resident set of blocks) and every block walks the chunks by, by + gridDim.y, ..: the
// number of chunks of a step is only known on the device, and a grid sized for the worst case (N / 8192 + 270 chunks x 9 groups = 6 624 blocks at
// c2) spent ~5 us per launch dispatching blocks that leave at once -- more than the working blocks of a small step need.
template <bool ROOT, int SUB, int TSC, bool RUNS = false, bool P8 = false, int NT = kThreads, bool CR = false, bool FQ = false>
__global__ __launch_bounds__(NT) void k_hist(const Ctx c)
{
    extern __shared__ unsigned long long lsum[];
    const TreeState *st = c.st;
    // XCD-aware block -> (feature group, chunk) map.  Block b is observed to run on XCD b % 8 and every XCD has its own L2: the
    // feature-group blocks of ONE chunk all read that chunk's lambdas and sample ids, so they are given ids that are congruent
    // mod 8 (chunk y lives on XCD y % 8) instead of consecutive ids that spread a chunk over all eight L2s (the PMC pass counted
    // the 8-byte lambda stream nine times).  A speed choice only; gridDim.y is a multiple of 8 (launch_hist).
#ifndef RL_HIST_NO_XCD
    const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x, lk = lin >> 3;
    const int bx = (int)(lk % gridDim.x), by = (int)((lk / gridDim.x) * 8 + (lin & 7));
#else
    const int bx = blockIdx.x, by = blockIdx.y;
#endif
    if (ROOT) { hist_chunk<ROOT, SUB, TSC, RUNS, P8, NT, CR, FQ>(c, st, bx, by, lsum); return; }
    const int total = st->done ? 0 : st->chunks_total;
    for (int y = by; y < total; y += (int)gridDim.y) {
        hist_chunk<ROOT, SUB, TSC, RUNS, P8, NT, CR, FQ>(c, st, bx, y, lsum);
        __syncthreads();        // the flush has read the LDS histogram: the next chunk may zero it
    }
}

// ------------------------------------------------------------------------------------------------
// K4/K5: one block per feature.
//   * sum the chunk partials of the (left) node into exact 128-bit bin totals
//   * inclusive prefix over threshold index -> cumulative sum / count   (FeatureHistogram.java:141-145,189-194)
//   * right sibling = parent - left                                     (FeatureHistogram.java:222-234)
//   * gain scan S = sl^2/cl + sr^2/cr per child, first maximum wins     (FeatureHistogram.java:236-264)
// LDS: TS x (hi, lo, cnt).
// ------------------------------------------------------------------------------------------------
constexpr int kParCacheTS = 1024;     // hist_finish_body keeps the parent's cumulative entries in LDS up to this many bins per feature
struct Best { double S; int t; };
__device__ __forceinline__ Best better(Best a, Best b)
{   // larger S wins; on equal S the lower threshold index (the one the Java loop meets first)
    if (b.S > a.S || (b.S == a.S && b.t >= 0 && (a.t < 0 || b.t < a.t))) return b;
    return a;
}

// block-wide best of two candidates at once (built child, sibling): one pair of barriers for both
__device__ void block_best2(Best &a, Best &b, Best *sh /* [2 * kFinThreads / 64] */, int nw_ = 0)
{
    for (int o = 32; o > 0; o >>= 1) {
        Best u; u.S = __shfl_xor(a.S, o); u.t = __shfl_xor(a.t, o);
        a = better(a, u);
        Best w; w.S = __shfl_xor(b.S, o); w.t = __shfl_xor(b.t, o);
        b = better(b, w);
    }
    const int NW = nw_ ? nw_ : (int)(blockDim.x >> 6);          // (the finish kernels run with 320 threads, or 192 on wide data: k_hist_finish_wide; blockDim.x is a load)
    __syncthreads();
    if (lane_id() == 0) { sh[threadIdx.x >> 6] = a; sh[NW + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    a = sh[0]; b = sh[NW];
    for (int i = 1; i < NW; i++) { a = better(a, sh[i]); b = better(b, sh[NW + i]); }
}

__device__ __forceinline__ double gain_S(double sl, int cl, double total, int ctot, int mls, bool &ok)
{
    const int cr = ctot - cl;
    ok = !(cl < mls || cr < mls);
    if (!ok) return -1.0;
    const double sr = total - sl;                                    // FeatureHistogram.java:251
    return sl * sl / cl + sr * sr / cr;                              // :253
}


// The mode bin was skipped by k_hist: bin[mode] = (sum over the node's samples) - (sum of the other bins), exact in
// fixed point.  s_hi/s_lo/s_cnt hold the per-bin totals (mode bin = 0); every thread calls this.
// have_pre: the caller has requested the thread's first chunk total (chunk ch0 + threadIdx.x) and the feature's mode bin already, together with its
// other loads (each was a dependent memory round trip in the middle of every finish block)
__device__ void rebuild_mode_bin(const Ctx &c, int f, int T, int ch0, int nch, int cnt_local, bool with_counts, long long *s_hi,
                                 unsigned long long *s_lo, int *s_cnt, i128 *sh_red /* kFinThreads/64 */, int *sh_redc,
                                 bool have_pre = false, long long tot_pre = 0, int mode_pre = 0)
{
    i128 part = 0; int cpart = 0;
    for (int t = threadIdx.x; t < T; t += (int)blockDim.x) { part += make_i128(s_hi[t], s_lo[t]); cpart += s_cnt[t]; }
    for (int ch = threadIdx.x; ch < nch; ch += (int)blockDim.x)
        part -= (i128)((have_pre && ch == (int)threadIdx.x) ? tot_pre : c.part_tot[ch0 + ch]);      // others - total
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t w0 = (uint32_t)(u128)part, w1 = (uint32_t)((u128)part >> 32), w2 = (uint32_t)((u128)part >> 64), w3 = (uint32_t)((u128)part >> 96);
        w0 = __shfl_xor(w0, o); w1 = __shfl_xor(w1, o); w2 = __shfl_xor(w2, o); w3 = __shfl_xor(w3, o);
        part += (i128)(((u128)w3 << 96) | ((u128)w2 << 64) | ((u128)w1 << 32) | (u128)w0);
        cpart += __shfl_xor(cpart, o);
    }
    if (lane_id() == 0) { sh_red[threadIdx.x >> 6] = part; sh_redc[threadIdx.x >> 6] = cpart; }
    __syncthreads();
    if (threadIdx.x == 0) {
        i128 others_minus_total = 0; int oc = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); i++) { others_minus_total += sh_red[i]; oc += sh_redc[i]; }
        const int m = have_pre ? mode_pre : c.mode[f];
        const i128 v = -others_minus_total;
        s_hi[m] = hi_of(v); s_lo[m] = lo_of(v);
        if (with_counts) s_cnt[m] = cnt_local - oc;
    }
    __syncthreads();
}

// multi-GPU: bin totals of the accumulated node as int64 limbs (a = v >> 44, b = v & (2^44-1), count) so that a plain
// int64 sum all-reduce of the limbs is exact; tail = the per-split scalars that travel with it
constexpr int kLimbShift = 44;
__global__ __launch_bounds__(kFinThreads) void k_hist_reduce(const Ctx c, int is_root)
{   // grid (F, slots)
    extern __shared__ unsigned long long sh_raw[];
    __shared__ i128 sh_red[kFinThreads / 64];
    __shared__ int sh_redc[kFinThreads / 64];
    const TreeState *st = c.st;
    const int slot = blockIdx.y;
    int nodeB = 0, ch0 = 0, nodeS = 0, nodeP = 0, sl_cs = 0, sl_cnt = -1;
    const bool active = is_root || (!st->done && slot < st->nslots);
    if (!is_root && active) {
        const SlotRec &sl = st->slot[slot];
        nodeB = sl.build_left ? sl.left : sl.right; nodeS = sl.build_left ? sl.right : sl.left; nodeP = sl.node; ch0 = sl.chunk0; sl_cs = sl.cs;
        if (sl.nleft >= 0) sl_cnt = sl.build_left ? sl.nleft : sl.pcount - sl.nleft;
    }
    const int f = blockIdx.x;
    const int TS = c.TS, T = c.nthr[f];
    long long *s_hi = (long long *)sh_raw;
    unsigned long long *s_lo = sh_raw + TS;
    int *s_cnt = (int *)(sh_raw + 2 * TS);
    const int cntB = is_root ? c.N : (active ? (sl_cnt >= 0 ? sl_cnt : c.nodes[nodeB].count) : 0);
    const int csB = is_root ? chunk_docs<true>(c, cntB) : (sl_cs > 0 ? sl_cs : chunk_docs<false>(c, cntB));      // (balance_slots)
    const int nch = (cntB + csB - 1) / csB;
    const int W = c.limb_words;
    const size_t slot_words = (size_t)c.F * TS * W + 4;
    long long *out = c.dist_buf + slot * slot_words + (size_t)f * TS * W;
    for (int t = threadIdx.x; t < T; t += kFinThreads) {
        i128 acc = 0; int cacc = 0;
        // (batches of eight chunk partials in flight, as in hist_finish_body: one at a time every chunk was a memory round trip)
        constexpr int kRedBatch = 8;
        const size_t cstride = (size_t)c.F * TS;
        const long long *ps = c.part_sum + ((size_t)ch0 * c.F + f) * TS + t;
        const int *pc = c.part_cnt + ((size_t)ch0 * c.F + f) * TS + t;
        unsigned long long lo = 0; long long hi = 0;
        for (int ch = 0; ch < nch; ch += kRedBatch) {
            long long v[kRedBatch]; int cn[kRedBatch];
#pragma unroll
            for (int u = 0; u < kRedBatch; u++) { const size_t o = (size_t)min(ch + u, nch - 1) * cstride; v[u] = ps[o]; cn[u] = is_root ? 0 : pc[o]; }
#pragma unroll
            for (int u = 0; u < kRedBatch; u++)
                if (ch + u < nch) { lo += (unsigned long long)(unsigned)v[u]; hi += (v[u] >> 32); cacc += cn[u]; }
        }
        acc += (i128)lo + (((i128)hi) << 32);
        s_hi[t] = hi_of(acc); s_lo[t] = lo_of(acc); s_cnt[t] = cacc;
    }
    __syncthreads();
    rebuild_mode_bin(c, f, T, ch0, nch, cntB, !is_root, s_hi, s_lo, s_cnt, sh_red, sh_redc);
    if (!is_root && active && c.cum_cnt_loc) {
        // this rank's cumulative counts of the built child and (parent - built) of its sibling: what tells the next partition of either node its
        // local left size (prepare_children)
        __syncthreads();
        __shared__ int sh_wc[kFinThreads / 64];
        int32_t *cb = c.cum_cnt_loc + ((size_t)nodeB * c.F + f) * TS, *cs_ = c.cum_cnt_loc + ((size_t)nodeS * c.F + f) * TS;
        const int32_t *cp = c.cum_cnt_loc + ((size_t)nodeP * c.F + f) * TS;
        int carry = 0;
        for (int t0 = 0; t0 < T; t0 += kFinThreads) {
            const int t = t0 + (int)threadIdx.x;
            const int v = t < T ? s_cnt[t] : 0, pv = t < T ? cp[t] : 0;
            const int inc = (int)wave_scan_u32((unsigned)v);
            if (lane_id() == 63) sh_wc[threadIdx.x >> 6] = inc;
            __syncthreads();
            int off = carry, all = 0;
#pragma unroll
            for (int w = 0; w < kFinThreads / 64; w++) { if (w < (int)(threadIdx.x >> 6)) off += sh_wc[w]; all += sh_wc[w]; }
            if (t < T) { cb[t] = off + inc; cs_[t] = pv - (off + inc); }
            carry += all;
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < T; t += kFinThreads) {
        const i128 acc = make_i128(s_hi[t], s_lo[t]);
        const long long hi = (long long)(acc >> kLimbShift), lo = (long long)(acc & ((((i128)1) << kLimbShift) - 1));
        const long long cn = is_root ? 0 : (long long)s_cnt[t];
        if (W == 3) { out[3 * t] = hi; out[3 * t + 1] = lo; out[3 * t + 2] = cn; }
        else { out[2 * t] = hi * 4294967296ll + cn; out[2 * t + 1] = lo; }       // |hi| < 2^30 and the global count < 2^31 (checked at init)
    }
    if (f == 0) {
        __shared__ long long sh_sq[kFinThreads / 64];
        const long long sqv = is_root ? st->root_sq : (active ? slot_sq_left(c, st->slot[slot], sh_sq) : 0);
        if (threadIdx.x == 0) c.dist_buf[slot * slot_words + (size_t)c.F * TS * W] = sqv;
    }
}

// ------------------------------------------------------------------------------------------------
#ifdef RL_PHASE_CLOCKS
#define RL_CLK(cond, k) do { if (cond) { const long long t_ = strict_clock(); if (threadIdx.x == 0) c.clk[(c.st->step & 63) * 32 + (k)] = t_; } } while (0)
#else
#define RL_CLK(cond, k) do { } while (0)
#endif

// Growth bookkeeping (select_step), run by the LAST block of k_hist_finish to arrive: best split of the new nodes
// across features (lowest feature index wins a tie, FeatureHistogram.java:302-309), then the best-first
// bookkeeping of RegressionTree.fit (:58-87) on LDS copies of TreeState, the node records and the queue (a single
// lane walking device memory pays ~1 us per dependent access).
//
// Speculative best-first growth.  RegressionTree.fit pops one node at a time, so a literal device version pays the
// latency of a chain of dependent kernels per split.  Here every step PREPARES up to kSpec nodes from the front of
// the queue at once (partition, child histograms, child best splits); the fit loop itself is replayed exactly and
// only COMMITS prepared nodes in the order the Java pops them.  Preparing a node writes nothing a committed node can
// see (new node records, the other ping-pong half of the node's own sample range, new histogram slots), so a
// prepared node that the loop never reaches (leaf budget exhausted) simply stays a leaf.
// ------------------------------------------------------------------------------------------------
// Per-feature results of k_hist_finish travel from its blocks to the one block that runs select_step INSIDE the same
// launch: agent-scope (write-through) stores, s_waitcnt, arrival counter -- no device-wide fence (on this 8-XCD
// part a __threadfence() per block costs an L2 write-back each).
struct FeatBest {           // best split of one feature for one new node + the cumulative histogram entry there
    unsigned long long S;    // double bits
    unsigned long long hi, lo;   // exact cumulative fixed-point sum at the split (= the left child's total)
    unsigned long long tc;   // (t << 32) | count at the split; bit 62: another threshold of this feature reaches the same S exactly
};
constexpr unsigned long long kFbTie = 1ull << 62, kFbTieDiff = 1ull << 61;
constexpr int kStepLogCap = 8192;      // entries of Ctx::steplog
template <class T> __device__ __forceinline__ void st_agent(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// What the finish blocks published (write-through stores, completed before they arrived) is read by the block that runs select_step with PLAIN loads
// behind ONE agent-scope acquire fence at its entry (it invalidates the stale lines this CU / XCD may hold of the records' fixed addresses).  Relaxed
// atomic loads were correct too, but the compiler completes each group of them (s_waitcnt vmcnt(0)) before it issues the next: a lane's five
// records were five dependent memory round trips in the step's serial tail, 22 with 700 features.
template <class T> __device__ __forceinline__ T ld_agent(const T *p) { return *p; }

// tie: bit 0 = another threshold of the feature reaches the same S, bit 1 = ... and cuts off other documents
__device__ __forceinline__ void publish_best(const Ctx &c, int slot, int side, int f, double S, int t, int cl, long long hi, unsigned long long lo, int tie = 0)
{
    FeatBest *o = c.fb + ((size_t)slot * 2 + side) * c.F + f;         // one 32-byte record: a single write-through line
    st_agent(&o->S, (unsigned long long)__double_as_longlong(S));
    st_agent(&o->hi, (unsigned long long)hi); st_agent(&o->lo, lo);
    st_agent(&o->tc, ((unsigned long long)(unsigned)t << 32) | (unsigned)cl | ((tie & 1) ? kFbTie : 0ull) | ((tie & 2) ? kFbTieDiff : 0ull));
}

// best split across features (lowest feature index wins a tie, FeatureHistogram.java:302-309).  A HALF wavefront per
// (slot, side): the 2 * kSpec reductions of a step then fit into one pass over the block's wavefronts.  `valid` is uniform
// in the half; every lane of the wavefront must call (shuffles).
// Feature sampling (c.fs_size < F, Random Forests): the node's draw = the fs_size features with the smallest keys
// feature_key(h, f), visited in key order, so a feature's RANK among the keys replaces its index: rank >= fs_size = not
// drawn, lowest rank wins a tie (:283-309).  fkeys: F words of LDS scratch owned by this half.
// The two sample sets a candidate cuts a node into, as an exact key: (documents, fixed-point sum) of the SMALLER side (of the side with the
// smaller sum when the counts are equal).  Candidates with equal keys have exactly equal true gains -- the same cut, or a mirrored one whose
// f64 S differs in the last bits only because sumRight = total - sumLeft is rounded (rl_tie.inc re-decides both kinds in the Java's order).
#ifndef RL_FB_BATCH
#define RL_FB_BATCH 8
#endif
struct PartKey { int cnt; i128 sum; };
__device__ __forceinline__ PartKey part_key(int cl, i128 sl, int ctot, i128 tot)
{
    const int cr = ctot - cl; const i128 sr = tot - sl;
    PartKey k;
    if (cl < cr) { k.cnt = cl; k.sum = sl; }
    else if (cl > cr) { k.cnt = cr; k.sum = sr; }
    else { k.cnt = cl; k.sum = sl < sr ? sl : sr; }
    return k;
}

// nthi / ntlo / nctot: the node's exact totals (for the mirrored-cut check; unused without the lazy tie-break)
// WIDE (k_select: the bookkeeping kernel of data with hundreds of features, where the block is alone on the chip and registers are free): all the gains
// of the lane's share (up to kWideS x 32 features) are requested at once and stay in registers for the tie pass -- at 700 features the three batches of
// eight, the winner's fields and the tie pass's second scan of the gains were seven dependent round trips (8-9 us of every growth step).
constexpr int kWideS = 24;
template <bool WIDE = false>
__device__ __forceinline__ void half_wave_best_feature(const Ctx &c, bool valid, int slot, int side, unsigned long long h, unsigned long long *fkeys,
                                       double &S, int &f, int &t, int &cl, long long &hi, unsigned long long &lo, int &tie,
                                       long long nthi = 0, unsigned long long ntlo = 0, int nctot = 0)
{
    const FeatBest *o = c.fb + ((size_t)slot * 2 + side) * c.F;
    const int hl = lane_id() & 31, hbase = lane_id() & 32;
    const bool sampling = c.fs_on != 0;
    if (sampling) {       // (the draw is over the REAL features: every run of a split threshold table carries its column's key -- Ctx::fcol, rl_init)
        if (valid) for (int i = hl; i < c.F; i += 32) fkeys[i] = feature_key(h, c.fcol[i] & 0x7fffffff);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    // every lane keeps the whole record of its best feature: the winner's fields come from a lane, not from a second
    // round trip to memory
    double bs = -1.0; int bf = -1, br = 0x7fffffff;
    unsigned long long bhi = 0, blo = 0, btc = 0;
    bool eq = false;            // another feature of this lane's share reaches the lane's best S exactly
    // Up to 32 * kFbFull features (the MSLR shape: 136): every lane asks for the WHOLE records of its share at once -- one memory round trip for the
    // gains, the winner's fields and the tie pass below, instead of three dependent ones (6-9 us of the step's serial tail were these loads).
    constexpr int kFbFull = 5;
    const bool small = !sampling && c.F <= 32 * kFbFull;
    unsigned long long kS[kFbFull], kH[kFbFull], kL[kFbFull], kT[kFbFull];
    [[maybe_unused]] unsigned long long wS[WIDE ? kWideS : 1];
#pragma unroll
    for (int u = 0; u < kFbFull; u++) { kS[u] = 0xbff0000000000000ull; kH[u] = kL[u] = kT[u] = 0ull; }
    if (valid && small) {
#pragma unroll
        for (int u = 0; u < kFbFull; u++) {
            const int i = hl + 32 * u;
            if (i < c.F) { kS[u] = ld_agent(&o[i].S); kH[u] = ld_agent(&o[i].hi); kL[u] = ld_agent(&o[i].lo); kT[u] = ld_agent(&o[i].tc); }
        }
#pragma unroll
        for (int u = 0; u < kFbFull; u++) {
            const int i = hl + 32 * u;
            const double s = __longlong_as_double((long long)kS[u]);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs) { eq = false; bs = s; bf = i; br = i; bhi = kH[u]; blo = kL[u]; btc = kT[u]; }         // (ascending i: the first of equal gains stays)
        }
    } else if (WIDE && valid && !sampling && c.F <= 32 * kWideS) {
#pragma unroll
        for (int u = 0; u < kWideS; u++) wS[u] = ld_agent(&o[min(hl + 32 * u, c.F - 1)].S);
#pragma unroll
        for (int u = 0; u < kWideS; u++) {
            const int i = hl + 32 * u;
            if (i >= c.F) wS[u] = 0xbff0000000000000ull /* -1.0 */;
            const double s = __longlong_as_double((long long)wS[u]);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs) { eq = false; bs = s; bf = i; br = i; }         // (ascending i: the first of equal gains stays)
        }
        if (bf >= 0) { bhi = ld_agent(&o[bf].hi); blo = ld_agent(&o[bf].lo); btc = ld_agent(&o[bf].tc); }
    } else if (valid && !sampling) {
        // Eight gains per lane are requested at once (the loads are agent-scope atomics: one at a time they cost a memory round trip per feature of
        // the lane's share -- 22 of them with 700 features, 16-19 us of this block's serial tail); the rest of a record is fetched for the lane's best only.
        constexpr int B = RL_FB_BATCH;
        for (int i0 = hl; i0 < c.F; i0 += 32 * B) {
            unsigned long long rs[B];
#pragma unroll
            for (int u = 0; u < B; u++) { const int i = i0 + 32 * u; rs[u] = (i < c.F) ? ld_agent(&o[i].S) : 0xbff0000000000000ull /* -1.0 */; }
#pragma unroll
            for (int u = 0; u < B; u++) {
                const int i = i0 + 32 * u;
                const double s = __longlong_as_double((long long)rs[u]);
                if (s == bs && s > -1.0) eq = true;
                if (s > bs) { eq = false; bs = s; bf = i; br = i; }         // (ascending i: the first of equal gains stays)
            }
        }
        if (bf >= 0) { bhi = ld_agent(&o[bf].hi); blo = ld_agent(&o[bf].lo); btc = ld_agent(&o[bf].tc); }
    } else if (valid) {
        for (int i = hl; i < c.F; i += 32) {
            const unsigned long long rs = ld_agent(&o[i].S), rh = ld_agent(&o[i].hi), rl = ld_agent(&o[i].lo), rt = ld_agent(&o[i].tc);
            int rank = i;
            {
                const unsigned long long ki = fkeys[i];
                rank = 0;
                // one count per real column: fcol[g] < 0 marks the later runs of a split table (they share their column's rank; the lower run wins an equal gain)
                const int ci = c.fcol[i] & 0x7fffffff;
                for (int g = 0; g < c.F; g++) { const int cg = c.fcol[g]; const unsigned long long kg = fkeys[g]; rank += (cg >= 0) && ((kg < ki) || (kg == ki && cg < ci)); }
                if (rank >= c.fs_size) continue;
            }
            const double s = __longlong_as_double((long long)rs);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs || (s == bs && s > -1.0 && rank < br)) { if (s > bs) eq = false; bs = s; bf = i; br = rank; bhi = rh; blo = rl; btc = rt; }
        }
    }
    RL_CLK(slot == 0 && side == 0 && valid, 17);       // the lane's share of the records has arrived and is reduced
    const int own = bf;         // this lane's candidate (its fields are in bhi / blo / btc)
    const double own_s = bs;
    for (int d = 16; d > 0; d >>= 1) {
        const double s = __shfl_xor(bs, d); const int ff = __shfl_xor(bf, d), rr = __shfl_xor(br, d);
        if (s > bs || (s == bs && ff >= 0 && (bf < 0 || rr < br || (rr == br && ff < bf)))) { bs = s; bf = ff; br = rr; }
    }
    S = bs; f = bf; t = -1; cl = 0; hi = 0; lo = 0;
    // the winner is the own candidate of exactly one lane of this half (ranks are distinct)
    RL_CLK(slot == 0 && side == 0 && valid, 18);       // ... across the half wavefront
    const unsigned long long ownmask = __ballot(bf >= 0 && own == bf) >> hbase;
    const int src = hbase + (int)__builtin_ctzll(ownmask | (1ull << 63));
    const unsigned long long tc = (unsigned long long)__shfl((long long)btc, src);
    const long long h2 = __shfl((long long)bhi, src); const unsigned long long l2 = (unsigned long long)__shfl((long long)blo, src);
    // exact ties (rl_tie.inc): several features reach the best S (2), or only other thresholds of the winning feature do (1)
    unsigned long long cross = __ballot(bf >= 0 && own >= 0 && own_s == bs && (own != bf || eq)) >> hbase;
    bool other_cut = false;     // a tied candidate of this lane's share does not have the winner's (left count, left sum): a mirrored or a different cut
    if (c.tie_on) {       // mirrored cuts of other features: equal partition keys although the f64 S differ by a rounding
        bool mir = false;
        if (valid && bf >= 0 && small) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
#pragma unroll
            for (int u = 0; u < kFbFull; u++) {
                const int i = hl + 32 * u;
                if (i == bf) continue;
                const double s = __longlong_as_double((long long)kS[u]);
                if (!(s > -1.0) || fabs(s - bs) > 1e-9 * fabs(bs)) continue;
                const unsigned long long itc = kT[u];
                const i128 isl = make_i128((long long)kH[u], kL[u]);
                const PartKey k = part_key((int)(unsigned)itc, isl, nctot, ntot);
                const bool keq = (k.cnt == wk.cnt && k.sum == wk.sum);
                mir |= keq;
                if (keq || s == bs) other_cut |= !((unsigned)itc == (unsigned)tc && isl == wsl) || (itc & kFbTieDiff) != 0;
            }
        } else if (WIDE && valid && bf >= 0 && !sampling && c.F <= 32 * kWideS) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
            // the near-equal gains of the share as bit masks (registers cannot be indexed by a run-time u); the records behind them -- rare -- come from memory
            unsigned near = 0u, exact = 0u;
#pragma unroll
            for (int u = 0; u < kWideS; u++) {
                const double s = __longlong_as_double((long long)wS[u]);
                if (hl + 32 * u != bf && s > -1.0 && !(fabs(s - bs) > 1e-9 * fabs(bs))) { near |= 1u << u; if (s == bs) exact |= 1u << u; }
            }
            while (near) {
                const int u = __builtin_ctz(near);
                near &= near - 1u;
                const int i = hl + 32 * u;
                const unsigned long long itc = ld_agent(&o[i].tc);
                const i128 isl = make_i128((long long)ld_agent(&o[i].hi), ld_agent(&o[i].lo));
                const PartKey k = part_key((int)(unsigned)itc, isl, nctot, ntot);
                const bool keq = (k.cnt == wk.cnt && k.sum == wk.sum);
                mir |= keq;
                if (keq || ((exact >> u) & 1u)) other_cut |= !((unsigned)itc == (unsigned)tc && isl == wsl) || (itc & kFbTieDiff) != 0;
            }
        } else if (valid && bf >= 0) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
            constexpr int B = RL_FB_BATCH;
            for (int i0 = hl; i0 < c.F; i0 += 32 * B) {
              unsigned long long rs[B];
#pragma unroll
              for (int u = 0; u < B; u++) { const int i = i0 + 32 * u; rs[u] = (i < c.F) ? ld_agent(&o[i].S) : 0xbff0000000000000ull; }
#pragma unroll
              for (int u = 0; u < B; u++) {
                const int i = i0 + 32 * u;
                if (i == bf) continue;
                const double s = __longlong_as_double((long long)rs[u]);
                if (!(s > -1.0) || fabs(s - bs) > 1e-9 * fabs(bs)) continue;
                const unsigned long long itc = ld_agent(&o[i].tc);
                const i128 isl = make_i128((long long)ld_agent(&o[i].hi), ld_agent(&o[i].lo));
                const PartKey k = part_key((int)(unsigned)itc, isl, nctot, ntot);
                const bool keq = (k.cnt == wk.cnt && k.sum == wk.sum);
                mir |= keq;
                if (keq || s == bs) other_cut |= !((unsigned)itc == (unsigned)tc && isl == wsl) || (itc & kFbTieDiff) != 0;
              }
            }
        }
        cross |= __ballot(mir) >> hbase;
    }
    RL_CLK(slot == 0 && side == 0 && valid, 19);       // tie pass
    const bool any_other = (__ballot(other_cut) >> hbase) & 0xffffffffull;
    tie = 0;
    if (bf >= 0) {
        t = (int)((tc >> 32) & 0xffffu); cl = (int)(unsigned)tc; hi = h2; lo = l2;
        // 2 = the Java's noise picks among several features, or among thresholds with other counts; 1 = thresholds of the winning feature that all cut
        // off the same documents; 4 (with 2) = every tied candidate of every feature cuts off the winner's (left count, exact left sum) -- the same
        // documents unless a coincidence of lambdas says otherwise, which the deferred tie-break verifies (rl_tie.inc); bits 8..: lanes (of 32)
        // whose share holds a tied feature
        tie = (cross & 0xffffffffull) ? (2 | (__builtin_popcountll(cross & 0xffffffffull) << 8)) : ((tc & kFbTieDiff) ? 2 : ((tc & kFbTie) ? 1 : 0));
        if ((cross & 0xffffffffull) && !any_other && !(tc & kFbTieDiff)) tie |= 4;
    }
}

__device__ __forceinline__ void queue_insert_lds(int *q, double *qd, int &qsize, int node, double d)
{   // RegressionTree.insert (:147-157): before the first element whose deviance is <= the new one's
    int i = 0;
    while (i < qsize) { if (qd[i] > d) i++; else break; }
    for (int j = qsize; j > i; j--) { q[j] = q[j - 1]; qd[j] = qd[j - 1]; }
    q[i] = node; qd[i] = d;
    qsize++;
}

// histogram chunks of a node of cnt samples (as k_hist cuts it)
__device__ __forceinline__ int node_chunks(const Ctx &c, int cnt) { return cnt <= 0 ? 0 : (cnt + chunk_docs<false>(c, cnt) - 1) / chunk_docs<false>(c, cnt); }

// Put node p into slot `sl` of the next growth step: its children l, l+1 get node records (global counts / exact
// totals from p's cumulative histogram); their local sample ranges are set by the partition kernel.
// tile0 / chunk0 are filled by the caller (prefix over the slots).
__device__ __forceinline__ void prepare_children(const Ctx &c, NodeRec *N, int p, int l, SlotRec &sl)
{
    NodeRec &P = N[p];
    const int r = l + 1;
    const int cl = P.best_cl;                                    // cumulative histogram entry at the split
    const long long thi = P.best_hi; const unsigned long long tlo = P.best_lo;
    NodeRec Lc, Rc;
    Lc.start = P.start; Lc.count = 0; Lc.gcount = cl; Lc.buf = 1 - P.buf; Lc.parent = p; Lc.left = Lc.right = -1;
    Rc.start = P.start; Rc.count = 0; Rc.gcount = P.gcount - cl; Rc.buf = 1 - P.buf; Rc.parent = p; Rc.left = Rc.right = -1;
    const i128 tl = make_i128(thi, tlo);                        // exact: same sample set as the left child
    const i128 tr = make_i128(P.tot_hi, P.tot_lo) - tl;
    Lc.tot_hi = hi_of(tl); Lc.tot_lo = lo_of(tl);
    Rc.tot_hi = hi_of(tr); Rc.tot_lo = lo_of(tr);
    Lc.best_f = Lc.best_t = Rc.best_f = Rc.best_t = -1; Lc.best_S = Rc.best_S = -1.0;
    Lc.best_cl = Rc.best_cl = 0; Lc.best_hi = Rc.best_hi = 0; Lc.best_lo = Rc.best_lo = 0;
    Lc.deviance = Rc.deviance = 0.0; Lc.sum_response = Rc.sum_response = 0.0; Lc.sq_response = Rc.sq_response = 0.0;
    Lc.sq = Rc.sq = 0;
    Lc.output = Rc.output = 0.f;
    Lc.pl = Lc.pr = Rc.pl = Rc.pr = -1; Lc.fid = Rc.fid = -1; Lc.prepared = Rc.prepared = 0;
    Lc.tie = Rc.tie = 0; Lc.ph = child_hash(P.ph, 0); Rc.ph = child_hash(P.ph, 1);
    N[l] = Lc; N[r] = Rc;
    P.pl = l; P.pr = r; P.prepared = 1;
    sl.node = p; sl.left = l; sl.right = r;
    sl.build_left = (cl <= P.gcount - cl) ? 1 : 0;
    sl.pstart = P.start; sl.pcount = P.count; sl.pbuf = P.buf; sl.f = P.best_f; sl.t = P.best_t;
    sl.tile0 = 0; sl.ntiles = (P.count + kPartTile - 1) / kPartTile;
    // chunks of the child that is accumulated: exact on one GPU; an upper bound of the LOCAL part when sharded
    sl.chunk0 = 0; sl.cs = 0; sl.skip_hist = 0;
    if (!c.sharded) { sl.nchunks = node_chunks(c, sl.build_left ? cl : P.gcount - cl); sl.nleft = cl; }
    else if (c.cum_cnt_loc) {       // sharded, round 6: this rank's share of the left child from its own cumulative counts (k_hist_reduce keeps them beside the all-reduced ones)
        const int nl = c.cum_cnt_loc[((size_t)p * c.F + P.best_f) * c.TS + P.best_t];
        sl.nleft = nl; sl.nchunks = node_chunks(c, sl.build_left ? nl : P.count - nl);
        N[l].count = nl; N[r].start = P.start + nl; N[r].count = P.count - nl;
    } else { sl.nchunks = (P.count == 0) ? 0 : max(64, P.count / c.node_chunk + 1) + 1; sl.nleft = -1; }
    sl.sq_left = 0;
    atomicAdd(&c.grow_docs[0], (unsigned long long)(sl.build_left ? cl : P.gcount - cl));
    atomicAdd(&c.grow_docs[1], (unsigned long long)P.gcount);
}

// Balanced chunks for a step that fills the chip (one GPU: the built children's sizes are known).  chunk_docs gives a large node the largest
// chunk, and the first steps of a c2 tree came to 810 / 1 692 / 1 233 (chunk, group) blocks for the 768 places of the chip (three 50 KB blocks per
// CU): CUs ended up with 3 to 5 (5 to 8) blocks and the launch lasted until the fullest CU was done (HISTORY.md 10.5, profiles/r04_block_placement_*).
// Here the step's documents are cut into k x balance_target chunks of ONE size (<= 2^14 documents: what an int64 accumulator holds), the same
// size for every node of the step, and launch_hist launches exactly balance_target rows of blocks, so every block row works through k chunks.
// balance_target = 56: 56 rows x 9 feature groups = 504 blocks = TWO per CU, which is what saturates a CU's LDS atomic unit; a third block on
// some CUs (80 rows) makes those CUs 1.5 x as slow as the others (measured: 80 rows +1 %, 56 rows +3 %, 64 / 72 rows worse than none).
// Steps of at most balance_min chunks keep the per-node rule (finer cuts only add partial histograms to flush and to reduce).  One thread calls
// this, after prepare_children, before the prefix over the slots.  Exact integer sums: the cut changes no result.
__device__ __forceinline__ void balance_slots(const Ctx &c, SlotRec *slot, int ns)
{
    if ((c.sharded && !c.cum_cnt_loc) || !c.balance) return;       // (local sizes unknown: chunk_docs' rule.  Until round 6 a ONE-rank communicator was balanced while k_hist_reduce
                                                                    // cut its nodes by chunk_docs' rule: runs of more than 28 chunks a step summed the wrong partials, tools/dist_scale_check.py)
    int legacy = 0; unsigned D = 0;       // (the built children of a step are disjoint: D <= N < 2^31 -- 32-bit divisions; a 64-bit one is ~100 instructions of the step's serial tail)
    int cnt[kSpec];
    for (int j = 0; j < ns && j < kSpec; j++) {
        cnt[j] = slot[j].build_left ? slot[j].nleft : slot[j].pcount - slot[j].nleft;
        legacy += slot[j].nchunks; D += (unsigned)cnt[j];
    }
    const int T = c.balance_target, cap = c.balance_cap;
    if (legacy <= c.balance_min) return;
    const unsigned tcap = (unsigned)T * (unsigned)cap;
    const int k = (int)(D / tcap + (D % tcap != 0u ? 1u : 0u));
    const int target = k * T;
    int cs = (int)((D / (unsigned)target + (D % (unsigned)target != 0u ? 1u : 0u) + 255u) & ~255u);
    for (;;) {
        if (cs > cap) cs = cap;
        int tot = 0;
        for (int j = 0; j < ns && j < kSpec; j++) tot += (cnt[j] + cs - 1) / cs;
        if (tot <= target || cs >= cap) break;
        cs += 256;
    }
    int tot = 0;
    for (int j = 0; j < ns && j < kSpec; j++) tot += (cnt[j] + cs - 1) / cs;
    if (tot > c.maxChunks) return;   // (the partial-histogram buffers hold maxChunks rows)
    for (int j = 0; j < ns && j < kSpec; j++) { slot[j].cs = cs; slot[j].nchunks = (cnt[j] + cs - 1) / cs; }
}

__device__ __forceinline__ double variance_of(double sq, double sum, int n) { return sq - sum * sum / n; }  // :348-350

__device__ __forceinline__ void copy_words(void *dst, const void *src, int nwords8)
{
    for (int i = threadIdx.x; i < nwords8; i += blockDim.x) ((unsigned long long *)dst)[i] = ((const unsigned long long *)src)[i];
}

__device__ __forceinline__ bool can_split(const Ctx &c, const NodeRec &X)
{   // RegressionTree.fit :74-77 (too few samples) and FeatureHistogram.findBestSplit :267-269, :311-313
    if (X.gcount < 2 * c.mls) return false;
    const bool zero_dev = (X.deviance >= 0.0 && X.deviance <= 0.0);
    return !(zero_dev || X.best_S == -1.0);
}

// lazy tie-break (rl_tie.inc): of the nodes about to be partitioned, those whose exactly tied best split the Java's rounding noise decides
// and that have not been resolved yet -- several features tie (2), or only thresholds of one feature do (1) but the node is a RIGHT child,
// whose Java histogram is parent - left (FeatureHistogram.java:222-234) instead of a sum of its own samples.  One thread calls this.
// A tie of kind 1 in a right child does NOT stall: every tied threshold cuts off the same documents, so the node is partitioned at once and only
// its stored threshold is re-decided, together with the tree's other such nodes, before the tree is exported (NodeRec::tie bit 0x40, `deferred`).
__device__ __forceinline__ int stalled_nodes(NodeRec *N, const int *sel, int nsel, int32_t *out, int *deferred, bool xdefer)
{
    int n = 0;
    for (int i = 0; i < nsel; i++) {
        NodeRec &X = N[sel[i]];
        if ((X.tie & 0xc0) || (X.tie & 3) == 0) continue;
        const bool right = X.parent >= 0 && N[X.parent].pr == sel[i];
        if ((X.tie & 3) == 2) {
            if (xdefer && (X.tie & 4)) { X.tie |= 0x40; *deferred = 1; }       // several features, one cut: partition now, name the feature later
            else out[n++] = sel[i];
        } else if (right) { X.tie |= 0x40; *deferred = 1; }
    }
    return n;
}

// bytes of dynamic LDS select_step needs
__host__ __device__ inline size_t select_lds_bytes(int L, int NC, bool nodes_in_lds, int F = 0, bool sampling = false)
{
    return sizeof(TreeState) + (nodes_in_lds ? (size_t)NC * sizeof(NodeRec) : 0) + (size_t)(L + 2) * 12 + (size_t)kSpec * 2 * 16 + 64 +
           (sampling ? (size_t)2 * kSpec * F * 8 + 8 : 0);
}

// Called by every thread of ONE block (the last one of k_hist_finish).  smem: TreeState | NodeRec[NC] (only if it
// fits, else the records are used in place) | qd[L+2] | bS[2 kSpec] | q[L+2] | bf, bt[2 kSpec] | sel[kSpec]
// NL (node records in LDS) is a template parameter: with a run-time choice between the LDS copy and c.nodes every access to a record was a FLAT
// load / store followed by a wait on both counters -- the fit loop's chain of dependent record reads ran at global-memory latency.
template <bool NL, bool WIDE = false>
__device__ __forceinline__ void select_step_t(const Ctx &c, bool is_root, unsigned char *smem, bool dist)
{
    constexpr bool nodes_in_lds = NL;
    static_assert(sizeof(TreeState) % 16 == 0 && sizeof(NodeRec) % 8 == 0, "copied as 8-byte words");
    TreeState &st = *(TreeState *)smem;
    unsigned char *ptr = smem + sizeof(TreeState);
    NodeRec *N = c.nodes;
    if (nodes_in_lds) { N = (NodeRec *)ptr; ptr += (size_t)c.NC * sizeof(NodeRec); }
    const int QC = c.L + 2;              // queue capacity
    double *qd = (double *)ptr; ptr += (size_t)QC * 8;
    double *bS = (double *)ptr; ptr += 2 * kSpec * 8;
    int *q = (int *)ptr; ptr += (size_t)QC * 4;
    int *bf = (int *)ptr; ptr += 2 * kSpec * 4;
    int *bt = (int *)ptr; ptr += 2 * kSpec * 4;
    int *sel = (int *)ptr; ptr += kSpec * 4;
    unsigned long long *fkeys = (unsigned long long *)(((size_t)ptr + 7) & ~(size_t)7);      // [2 kSpec][F], only with feature sampling
    __shared__ int bcl[2 * kSpec], btie[2 * kSpec]; __shared__ long long bhi[2 * kSpec]; __shared__ unsigned long long blo[2 * kSpec];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6, nwaves = blockDim.x >> 6;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");          // see ld_agent
#ifdef RL_PHASE_CLOCKS
    { const long long t_ = strict_clock(); if (!is_root && threadIdx.x == 0) c.clk[(c.st->step & 63) * 32 + 14] = t_; }      // select entry
#endif
    copy_words(&st, c.st, sizeof(TreeState) / 8);
    __syncthreads();
    const int E = st.E, E2 = st.E2;

    if (is_root) {
        if (wave == 0) {
            double S0; int f0, t0, cl0, tie0; long long hi0; unsigned long long lo0;
            const unsigned long long h0 = root_hash(c.seed, st.tree_seq);       // tree_seq = trees started before this one
            half_wave_best_feature(c, lane < 32, 0, 0, h0, fkeys, S0, f0, t0, cl0, hi0, lo0, tie0,
                                   (long long)ld_agent((const unsigned long long *)&c.fb_root[0]), ld_agent((const unsigned long long *)&c.fb_root[1]), c.cum_cnt[(size_t)c.nthr[0] - 1]);
            if (lane == 0) {
                NodeRec R;
                R.start = 0; R.count = c.N; R.buf = 0; R.parent = -1; R.left = R.right = -1;
                R.gcount = c.cum_cnt[(size_t)c.nthr[0] - 1];            // global N (static counts; feature 0, last bin)
                R.tot_hi = (long long)ld_agent((const unsigned long long *)&c.fb_root[0]); R.tot_lo = ld_agent((const unsigned long long *)&c.fb_root[1]);
                // sharded: the all-reduced sum (st.root_sq stays this rank's own: a tree that is grown a second time reduces it again)
                R.sq = c.sharded ? c.dist_buf[(size_t)c.F * c.TS * c.limb_words] : st.root_sq;
                R.sum_response = fixed_to_double(make_i128(R.tot_hi, R.tot_lo), E);
                R.sq_response = fixed_to_double((i128)R.sq, E2);
                if (c.java) { R.sum_response = c.jtot[0]; R.sq_response = c.jtot[1]; }      // sequential sums over k = 0 .. N-1 (:133-137)
                R.deviance = 3.4028234663852886e38;           // Float.MAX_VALUE  (RegressionTree.java:60)
                R.best_S = S0; R.best_f = f0; R.best_t = t0; R.output = 0.f;
                R.best_cl = cl0; R.best_hi = hi0; R.best_lo = lo0;
                R.pl = R.pr = -1; R.fid = 0; R.prepared = 0; R.tie = c.fs_on ? 0 : tie0; R.ph = h0;
                st.n_nodes = 1; st.qsize = 0; st.taken = 0; st.done = 0; st.nslots = 0; st.n_splits = 0; st.stall_n = 0; st.defer_any = 0;
                st.step = 0; st.tree_seq++;
                st.tiles_total = 0; st.chunks_total = 0; st.arrive = 0; st.epoch++;
                for (int j = 0; j < kSpec * 16; j++) (&st.arrive1[0][0])[j] = 0;
                N[0] = R;
                if (S0 == -1.0) st.done = 1;                  // root cannot split: single-leaf tree (:64-67,86)
                else if (c.tie_on && (R.tie & 3) == 2 && !((c.tie_on & 2) && (R.tie & 4))) { st.stall_n = 1; st.stall_node[0] = 0; }      // several features tie at the root: the Java's noise decides (rl_tie.inc)
                else {
                    if (c.tie_on && (R.tie & 3) == 2) { N[0].tie |= 0x40; st.defer_any = 1; }      // ... over one and the same cut: deferred
                    prepare_children(c, N, 0, 1, st.slot[0]);
                    balance_slots(c, st.slot, 1);
                    st.n_nodes = 3; st.nslots = 1; st.tiles_total = st.slot[0].ntiles; st.chunks_total = st.slot[0].nchunks;
                    c.grow_stats[0]++; c.grow_stats[1]++;
                }
                c.grow_stats[3]++;
            }
        }
        __syncthreads();
        if (nodes_in_lds) copy_words(c.nodes, N, st.n_nodes * (int)(sizeof(NodeRec) / 8));
        copy_words(c.st, &st, sizeof(TreeState) / 8);
        if (tid == 0 && c.progress)
            __hip_atomic_store(c.progress, ((unsigned long long)(unsigned)st.tree_seq << 32) | (st.stall_n > 0 ? (1ull << 31) : 0ull) | (st.defer_any ? (1ull << 30) : 0ull) | (st.done ? 1ull : 0ull),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }

    RL_CLK(true, 8);
    // A. best split per (slot, side) by one wavefront each; LDS copies of the node records and the queue
    const int ns = st.nslots, qs0 = st.qsize, nn0 = st.n_nodes;
    long long sq_left_v = 0;        // unsharded: sum of lambda^2 over the left child, reduced from the partition's per-tile partials by block (0, slot)
    if (!dist && tid < ns) sq_left_v = (long long)ld_agent(&c.fb_sq[tid]);
    // the node records and the queue are fetched first: their loads are in flight while the per-feature records are reduced
    constexpr int kPre = 8;
    const int nw8 = nodes_in_lds ? nn0 * (int)(sizeof(NodeRec) / 8) : 0;
    unsigned long long pre[kPre];
#pragma unroll
    for (int u = 0; u < kPre; u++) { const int i = tid + u * (int)blockDim.x; pre[u] = i < nw8 ? ((const unsigned long long *)c.nodes)[i] : 0ull; }
    const int q_pre = tid < qs0 ? c.queue[tid] : 0;
#ifdef RL_PHASE_CLOCKS
    if (tid == 0) c.clk[(c.st->step & 63) * 32 + 16] = (long long)wall_clock64();      // (no wait: the loads above stay in flight)
#endif
    for (int p0 = 2 * wave; p0 < 2 * ns; p0 += 2 * nwaves) {
        const int pi = p0 + (lane >> 5);
        double S; int f, t, cl, tie; long long hi; unsigned long long lo;
        unsigned long long h = 0;
        if (c.fs_on && pi < 2 * ns) h = c.nodes[(pi & 1) ? st.slot[pi >> 1].right : st.slot[pi >> 1].left].ph;
        long long nthi = 0; unsigned long long ntlo = 0; int nctot = 0;
        if (c.tie_on && pi < 2 * ns) { const NodeRec &Ch = c.nodes[(pi & 1) ? st.slot[pi >> 1].right : st.slot[pi >> 1].left]; nthi = Ch.tot_hi; ntlo = Ch.tot_lo; nctot = Ch.gcount; }
        half_wave_best_feature<WIDE>(c, pi < 2 * ns, pi >> 1, pi & 1, h, fkeys + (size_t)min(pi, 2 * kSpec - 1) * c.F, S, f, t, cl, hi, lo, tie, nthi, ntlo, nctot);
        if ((lane & 31) == 0 && pi < 2 * ns) { bS[pi] = S; bf[pi] = f; bt[pi] = t; bcl[pi] = cl; bhi[pi] = hi; blo[pi] = lo; btie[pi] = c.fs_on ? 0 : tie; }
    }
    RL_CLK(true, 15);
#pragma unroll
    for (int u = 0; u < kPre; u++) { const int i = tid + u * (int)blockDim.x; if (i < nw8) ((unsigned long long *)N)[i] = pre[u]; }
    for (int i = tid + kPre * (int)blockDim.x; i < nw8; i += blockDim.x) ((unsigned long long *)N)[i] = ((const unsigned long long *)c.nodes)[i];
    if (tid < qs0) q[tid] = q_pre;
    for (int i = tid + (int)blockDim.x; i < qs0; i += blockDim.x) q[i] = c.queue[i];
    __syncthreads();
    RL_CLK(true, 9);
    // B. complete the children of the nodes prepared by the step that just ran (one thread per slot)
    if (!dist) { if (tid < ns) st.slot[tid].sq_left = sq_left_v; }
    else if (tid < ns) st.slot[tid].sq_left = c.dist_buf[(size_t)tid * ((size_t)c.F * c.TS * c.limb_words + 4) + (size_t)c.F * c.TS * c.limb_words];     // all-reduced
    __syncthreads();
    if (tid < ns) {
        const SlotRec &sl = st.slot[tid];
        NodeRec &P = N[sl.node]; NodeRec &Lc = N[sl.left]; NodeRec &Rc = N[sl.right];
        if (sl.build_left) { Lc.sq = sl.sq_left; Rc.sq = P.sq - Lc.sq; }       // sq_left: the BUILT child's sum (k_part_scatter)
        else { Rc.sq = sl.sq_left; Lc.sq = P.sq - Rc.sq; }
        Lc.sum_response = fixed_to_double(make_i128(Lc.tot_hi, Lc.tot_lo), E);
        Rc.sum_response = fixed_to_double(make_i128(Rc.tot_hi, Rc.tot_lo), E);
        Lc.sq_response = fixed_to_double((i128)Lc.sq, E2);
        Rc.sq_response = fixed_to_double((i128)Rc.sq, E2);
        if (c.java) {       // left: sequential sums over its samples (:182-186); right: parent - left (:202-203)
            Lc.sum_response = c.jtot[2 * tid]; Lc.sq_response = c.jtot[2 * tid + 1];
            Rc.sum_response = P.sum_response - Lc.sum_response; Rc.sq_response = P.sq_response - Lc.sq_response;
        }
        Lc.deviance = variance_of(Lc.sq_response, Lc.sum_response, Lc.gcount);
        Rc.deviance = variance_of(Rc.sq_response, Rc.sum_response, Rc.gcount);
        Lc.best_S = bS[2 * tid]; Lc.best_f = bf[2 * tid]; Lc.best_t = bt[2 * tid];
        Lc.best_cl = bcl[2 * tid]; Lc.best_hi = bhi[2 * tid]; Lc.best_lo = blo[2 * tid];
        Rc.best_S = bS[2 * tid + 1]; Rc.best_f = bf[2 * tid + 1]; Rc.best_t = bt[2 * tid + 1];
        Rc.best_cl = bcl[2 * tid + 1]; Rc.best_hi = bhi[2 * tid + 1]; Rc.best_lo = blo[2 * tid + 1];
        Lc.tie = btie[2 * tid]; Rc.tie = btie[2 * tid + 1];
    }
    __syncthreads();
    RL_CLK(true, 10);
    // C. RegressionTree.fit's loop (:70-85), as far as prepared nodes allow, then the choice of the next slots.
    if (QC <= 64) {
        // Wavefront version: lane p holds queue entry p (node, deviance, can-split, prepared) in registers;
        // insert = ballot + shift, pop = shift.  (A single lane walking LDS pays ~50 ns per dependent access.)
        if (wave == 0) {
            int qn = (lane < qs0) ? q[lane] : -1;
            double qdv = 0.0; bool cs = false, prep = false;
            if (qn >= 0) { const NodeRec &X = N[qn]; qdv = X.deviance; cs = can_split(c, X); prep = X.prepared != 0; }
            int qsize = qs0, taken = st.taken, n_splits = st.n_splits, ncommit = 0;
            const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
            auto insert = [&](int node, double d, bool ncs) {          // RegressionTree.insert (:147-157)
                const int pos = __builtin_popcountll(__ballot(lane < qsize && qdv > d));
                const int un = __shfl_up(qn, 1); const double ud = __shfl_up(qdv, 1);
                const int uc = __shfl_up((int)cs, 1), up = __shfl_up((int)prep, 1);
                if (lane > pos) { qn = un; qdv = ud; cs = uc != 0; prep = up != 0; }
                else if (lane == pos) { qn = node; qdv = d; cs = ncs; prep = false; }
                qsize++;
            };
            auto pop = [&]() {
                qn = __shfl_down(qn, 1); qdv = __shfl_down(qdv, 1);
                cs = __shfl_down((int)cs, 1) != 0; prep = __shfl_down((int)prep, 1) != 0;
                qsize--;
            };
            // a split becomes part of the tree: sp.set(.., var) (:352), children enter the queue (:66-67, :82-83)
            auto commit = [&](int p) {
                NodeRec &X = N[p];
                const int l = X.pl, r = X.pr;
                const int child = (lane == 0) ? l : r;
                double dch = 0.0; int cch = 0;
                if (lane < 2) { dch = N[child].deviance; cch = can_split(c, N[child]) ? 1 : 0; }
                const double dl = __shfl(dch, 0), dr = __shfl(dch, 1);
                const int csl = __shfl(cch, 0), csr = __shfl(cch, 1);
                if (lane == 0) {
                    X.left = l; X.right = r;
                    X.deviance = variance_of(X.sq_response, X.sum_response, X.gcount);
                    N[l].fid = 2 * n_splits + 1; N[r].fid = 2 * n_splits + 2;
                    c.grow_docs[2] += (unsigned long long)N[l].gcount; c.grow_docs[3] += (unsigned long long)X.gcount;
                    if (c.steplog && X.tie) {       // debug: committed splits whose best candidate was tied, and the Java-order derivation chain they hang on
                        const int e = atomicAdd(&c.steplog[0], 1);
                        if (e < kStepLogCap) {
                            int *o = c.steplog + 8 + 8 * e;
                            int cur = p, nchain = 1, mx = X.gcount; long long tot = X.gcount;
                            const bool is_right = X.parent >= 0 && N[X.parent].pr == p;
                            while (N[cur].parent >= 0 && N[N[cur].parent].pr == cur) {       // a right child: parent - left sibling
                                const int par = N[cur].parent, sib = N[par].pl;
                                mx = max(mx, N[sib].gcount); tot += N[sib].gcount; nchain++;
                                cur = par;
                            }
                            if (cur != p) { mx = max(mx, N[cur].gcount); tot += N[cur].gcount; nchain++; }
                            o[0] = st.tree_seq; o[1] = 1; o[2] = X.tie & 255; o[3] = (is_right ? 1 : 0) | ((X.tie >> 8) << 1); o[4] = X.gcount; o[5] = mx; o[6] = nchain; o[7] = (int)min(tot, (long long)0x7fffffff);
                        }
                    }
                }
                n_splits++; ncommit++;
                insert(l, dl, csl != 0);
                insert(r, dr, csr != 0);
            };
            if (ns == 1 && st.slot[0].node == 0) commit(0);              // the root is split unconditionally (:62-67)
            bool done = true;
            while (taken + qsize < c.L && qsize > 0) {
                const int leaf = __shfl(qn, 0);
                const bool cs0 = __shfl((int)cs, 0) != 0, prep0 = __shfl((int)prep, 0) != 0;
                if (!cs0) { pop(); taken++; continue; }
                if (prep0) { pop(); commit(leaf); continue; }
                done = false;
                break;
            }
            // next step: the first kSpec unprepared nodes in queue order that the leaf budget can still reach
            int nsel = 0, err = 0;
            if (!done) {
                const int budget = c.L - (taken + qsize);                         // splits left (>= 1)
                const bool inq = lane < qsize;
                const int ahead = __builtin_popcountll(__ballot(inq && cs) & below);          // splittable nodes before p
                const bool cand = inq && cs && !prep && ahead < budget;
                const unsigned long long cmask = __ballot(cand);
                const int rank = __builtin_popcountll(cmask & below);
                nsel = min(__builtin_popcountll(cmask), kSpec);
                while (nsel > 0 && nn0 + 2 * nsel > c.NC) nsel--;
                if (cand && rank < nsel) sel[rank] = qn;
                if (nsel == 0) { done = true; err = 1; }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            int nstall = 0;
            if (c.tie_on && lane == 0) nstall = stalled_nodes(N, sel, nsel, st.stall_node, &st.defer_any, (c.tie_on & 2) != 0);
            nstall = __shfl(nstall, 0);
            if (nstall > 0) nsel = 0;                 // nothing is partitioned until the host has resolved the ties (rl_tie.inc)
            if (lane == 0) st.stall_n = nstall;
            if (lane < qsize) c.queue[lane] = qn;
            if (lane == 0) {
                st.done = done ? 1 : 0; if (err && !st.error) st.error = 1;
                st.nslots = nsel; st.qsize = qsize; st.taken = taken; st.n_splits = n_splits;
                c.grow_stats[2] += ncommit;
                if (nsel > 0) { c.grow_stats[0]++; c.grow_stats[1] += nsel; }
            }
        }
    } else {
        for (int i = tid; i < qs0; i += blockDim.x) qd[i] = N[q[i]].deviance;
        __syncthreads();
        if (tid == 0) {       // serial version for very wide trees
            int head = 0, qsize = qs0, ncommit = 0;
            auto commit = [&](int p) {
                NodeRec &X = N[p];
                X.left = X.pl; X.right = X.pr;
                X.deviance = variance_of(X.sq_response, X.sum_response, X.gcount);
                N[X.left].fid = 2 * st.n_splits + 1; N[X.right].fid = 2 * st.n_splits + 2;
                c.grow_docs[2] += (unsigned long long)N[X.left].gcount; c.grow_docs[3] += (unsigned long long)X.gcount;
                st.n_splits++;
                ncommit++;
                int n = qsize - head;
                queue_insert_lds(q + head, qd + head, n, X.left, N[X.left].deviance);
                queue_insert_lds(q + head, qd + head, n, X.right, N[X.right].deviance);
                qsize = head + n;
            };
            if (ns == 1 && st.slot[0].node == 0) commit(0);
            bool done = true;
            while ((c.L == -1 || st.taken + (qsize - head) < c.L) && (qsize - head) > 0) {
                const int leaf = q[head];
                const NodeRec &X = N[leaf];
                if (!can_split(c, X)) { head++; st.taken++; continue; }
                if (X.prepared) { head++; commit(leaf); continue; }
                done = false;
                break;
            }
            st.done = done ? 1 : 0;
            int nsel = 0;
            if (!done) {
                const int budget = (c.L == -1) ? 0x7fffffff : c.L - (st.taken + (qsize - head));
                int ahead = 0;
                for (int p = head; p < qsize && nsel < kSpec && ahead < budget; p++) {
                    const NodeRec &X = N[q[p]];
                    if (!can_split(c, X)) continue;
                    ahead++;
                    if (X.prepared) continue;
                    if (nn0 + 2 * (nsel + 1) > c.NC) { if (nsel == 0) st.error = 1; break; }
                    sel[nsel++] = q[p];
                }
                if (nsel == 0) { st.done = 1; if (!st.error) st.error = 2; }
            }
            st.stall_n = c.tie_on ? stalled_nodes(N, sel, nsel, st.stall_node, &st.defer_any, (c.tie_on & 2) != 0) : 0;
            if (st.stall_n > 0) nsel = 0;
            st.nslots = nsel;
            st.qsize = qsize - head;
            for (int i = 0; i < st.qsize; i++) c.queue[i] = q[head + i];
            c.grow_stats[2] += ncommit;
            if (nsel > 0) { c.grow_stats[0]++; c.grow_stats[1] += nsel; }
        }
    }
    __syncthreads();
    RL_CLK(true, 11);
    // D. children records of the selected nodes (one thread per slot: the histogram reads are independent)
    const int nsel = st.nslots;
    if (tid < nsel) prepare_children(c, N, sel[tid], nn0 + 2 * tid, st.slot[tid]);
    if (c.steplog && tid < nsel) {        // debug: what every growth step works on
        const int e = atomicAdd(&c.steplog[0], 1);
        if (e < kStepLogCap) {
            int *o = c.steplog + 8 + 8 * e; const NodeRec &P = N[sel[tid]];
            o[0] = st.tree_seq; o[1] = 0; o[2] = st.step + 1; o[3] = tid; o[4] = P.gcount; o[5] = st.slot[tid].build_left ? P.best_cl : P.gcount - P.best_cl; o[6] = P.tie; o[7] = nsel;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int tiles = 0, chunks = 0;
        balance_slots(c, st.slot, nsel);
        for (int j = 0; j < nsel; j++) {
            st.slot[j].tile0 = tiles; tiles += st.slot[j].ntiles;
            st.slot[j].chunk0 = chunks; chunks += st.slot[j].nchunks;
        }
        st.tiles_total = tiles; st.chunks_total = chunks;
        st.n_nodes = nn0 + 2 * nsel;
        st.arrive = 0; st.epoch++;
        for (int j = 0; j < kSpec * 16; j++) (&st.arrive1[0][0])[j] = 0;
    }
    __syncthreads();
    RL_CLK(true, 12);
    if (nodes_in_lds) copy_words(c.nodes, N, st.n_nodes * (int)(sizeof(NodeRec) / 8));
    RL_CLK(true, 13);
#ifdef RL_PHASE_CLOCKS
    if (tid == 0 && st.tree_seq == c.trace_tree) c.clk[(st.step & 63) * 32 + 28] = (long long)wall_clock64();      // end of this step's bookkeeping
#endif
    if (tid == 0) st.step++;
    __syncthreads();
    copy_words(c.st, &st, sizeof(TreeState) / 8);
    // tell the host how far the tree is (relaxed system-scope store: no fence, nothing else is read through it)
    if (tid == 0 && c.progress)
        __hip_atomic_store(c.progress, ((unsigned long long)(unsigned)st.tree_seq << 32) | (st.stall_n > 0 ? (1ull << 31) : 0ull) | (st.defer_any ? (1ull << 30) : 0ull) |
                                           ((unsigned long long)((unsigned)st.step & 0x1fffffffu) << 1) | (st.done ? 1ull : 0ull),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <bool WIDE = false>
__device__ __forceinline__ void select_step(const Ctx &c, bool is_root, unsigned char *smem, bool nodes_in_lds, bool dist)
{
    if (nodes_in_lds) select_step_t<true, WIDE>(c, is_root, smem, dist);
    else select_step_t<false, WIDE>(c, is_root, smem, dist);
}

// SELECT: the last block to arrive runs select_step (one launch per growth step's finish).  !SELECT: the per-feature work only; the bookkeeping
// follows as a launch of its own (k_select) -- for wide data, see k_hist_finish_wide.
constexpr int kFinWideThreads = 192;     // three wavefronts: 10 blocks a CU at 8 wavefronts per SIMD (2 560 resident blocks)
template <bool ROOT, bool DIST, bool JAVA, bool SELECT>
__device__ __forceinline__ void hist_finish_body(const Ctx &c, int nodes_in_lds, unsigned long long *sh_raw)
{   // grid (F, slots)
    TreeState *st = c.st;
    RL_TR_BEGIN();
    constexpr int kNT = SELECT ? kFinThreads : kFinWideThreads;      // threads of the block (blockDim.x is a load from the dispatch packet)
    // B = the node whose histogram was accumulated from its samples, S = its sibling (= parent - B)
    int nodeB = 0, nodeS = -1, nodeP = -1, sideB = 0, ch0 = 0;
    const int slot = blockIdx.y;
    // everything the block needs from the step's tables is requested at once (the slot record is copied whole, valid or not: slot < kSpec), and the
    // feature's threshold count comes from a table parallel to `live`: each of these was a dependent memory round trip at the top of every block
    const int st_done = st->done, st_nslots = st->nslots, E = st->E;
#ifndef RL_FIN_BATCH
#define RL_FIN_BATCH 1
#endif
#if RL_FIN_BATCH
    SlotRec sl_c;
    if (!ROOT) sl_c = st->slot[slot];
#else
    const SlotRec &sl_c = st->slot[ROOT ? 0 : slot];
#endif
    const int f = (!DIST && c.live) ? c.live[blockIdx.x] : (int)blockIdx.x;
    const int TS = c.TS, T = (!DIST && c.live) ? c.live_nthr[blockIdx.x] : c.nthr[f];
    if (!ROOT) {
        if (st_done || slot >= st_nslots) return;
        const SlotRec &sl = sl_c;
        nodeP = sl.node; ch0 = sl.chunk0;
        if (sl.build_left) { nodeB = sl.left; nodeS = sl.right; sideB = 0; }
        else { nodeB = sl.right; nodeS = sl.left; sideB = 1; }
    }
    [[maybe_unused]] const bool clk0 = !ROOT && blockIdx.x == 0 && blockIdx.y == 0;
    RL_CLK(clk0, 0);
    RL_TR_MARK(1);
    long long *s_hi = (long long *)sh_raw;
    unsigned long long *s_lo = sh_raw + TS;
    int *s_cnt = (int *)(sh_raw + 2 * TS);
    [[maybe_unused]] double *s_j = (double *)((unsigned char *)sh_raw + (((size_t)TS * 20 + 7) & ~(size_t)7));   // JAVA: f64 cumulative sums of the left child / the root
    // the parent's cumulative entries, kept as the gain scan reads them: the tie check and the sibling's published record used to fetch theirs from memory again
    // (a dependent round trip each, at the end of every block)
    unsigned char *s_par = (unsigned char *)sh_raw + (((size_t)TS * 20 + 7) & ~(size_t)7) + (JAVA ? (size_t)TS * 8 : 0);
    [[maybe_unused]] long long *s_phi = (long long *)s_par;
    [[maybe_unused]] unsigned long long *s_plo = (unsigned long long *)(s_par + (size_t)TS * 8);
    [[maybe_unused]] int *s_pcn = (int *)(s_par + (size_t)TS * 16);
    const bool pcache = TS <= kParCacheTS;          // (threshold tables beyond that keep the old behaviour: twice the LDS would not fit a CU at -tc 4095)
    __shared__ Best sh_best[2 * (kFinThreads / 64)];
    __shared__ i128 sh_red[kFinThreads / 64];
    __shared__ int sh_redc[kFinThreads / 64];

    // block (0, slot) also folds the partition's per-tile lambda^2 partials of its slot (select_step used to do that in the serial tail)
    __shared__ long long sh_sqw[kFinThreads / 64];
    long long sqacc = 0;
    const bool sq_block = !ROOT && !DIST && blockIdx.x == 0;
    if (sq_block) {
        const SlotRec &sl = sl_c;
        // (eight per thread and trip, unconditional from a clamped index: one at a time the 1 841 tile partials of a 3.8 M-document parent were six serial round trips)
        constexpr int kSqBatch = 8;
        for (int i0 = (int)threadIdx.x; i0 < sl.ntiles; i0 += kSqBatch * kNT) {
            long long v[kSqBatch];
#pragma unroll
            for (int u = 0; u < kSqBatch; u++) v[u] = c.tile_sq[sl.tile0 + min(i0 + u * kNT, sl.ntiles - 1)];
#pragma unroll
            for (int u = 0; u < kSqBatch; u++) if (i0 + u * kNT < sl.ntiles) sqacc += v[u];
        }
    }
    int cntB_ = ROOT ? c.N : 0;
    if (!ROOT) {
        const SlotRec &slb = sl_c;
        cntB_ = (slb.nleft >= 0) ? (slb.build_left ? slb.nleft : slb.pcount - slb.nleft) : c.nodes[nodeB].count;      // one GPU: known from the slot
    }
    const int cntB = cntB_;
    const int csB = (!ROOT && sl_c.cs > 0) ? sl_c.cs : chunk_docs<ROOT>(c, cntB);      // (balance_slots)
    const int nch = (cntB + csB - 1) / csB;
    const size_t slotB = ((size_t)nodeB * c.F + f) * TS;
    // the parent's cumulative entry this thread needs in the gain scan: requested now, with the chunk partials, not after the prefix
    // (every gain-scan iteration of the thread: two with the 192-thread blocks of k_hist_finish_wide and 257 bins)
    constexpr int kPreIt = SELECT ? 1 : 2;
    long long pre_phi[kPreIt]; unsigned long long pre_plo[kPreIt]; int pre_pcnt[kPreIt];
#pragma unroll
    for (int u = 0; u < kPreIt; u++) {
        pre_phi[u] = 0; pre_plo[u] = 0; pre_pcnt[u] = 0;
        if (RL_FIN_BATCH && !ROOT) {
            const size_t o = ((size_t)nodeP * c.F + f) * TS + min((int)threadIdx.x + u * kNT, TS - 1);       // (clamped, unconditional)
            pre_phi[u] = c.cum_hi[o]; pre_plo[u] = c.cum_lo[o]; pre_pcnt[u] = c.cum_cnt[o];
        }
    }
    // ... the parent's totals (its last cumulative entry; the same address for every thread) ...
    long long tp_hi = 0; unsigned long long tp_lo = 0; int tp_cn = 0;
    if (!ROOT) { const size_t o = ((size_t)nodeP * c.F + f) * TS + (T - 1); tp_hi = c.cum_hi[o]; tp_lo = c.cum_lo[o]; tp_cn = c.cum_cnt[o]; }
    // ... and what the mode-bin rebuild needs: this thread's chunk total and the feature's mode bin
    long long pre_tot = 0; int pre_mode = 0;
    if (!DIST) { pre_tot = c.part_tot[ch0 + max(min((int)threadIdx.x, nch - 1), 0)]; pre_mode = c.mode[f]; }
    if (DIST) {     // totals were reduced over the chunks by k_hist_reduce and over the ranks by the all-reduce
        const int W = c.limb_words;
        const size_t slot_words = (size_t)c.F * TS * W + 4;
        const long long *in = c.dist_buf + slot * slot_words + (size_t)f * TS * W;
        for (int t = threadIdx.x; t < T; t += kNT) {
            long long hi, lo, cn;
            if (W == 3) { hi = in[3 * t]; lo = in[3 * t + 1]; cn = in[3 * t + 2]; }
            else { const long long w0 = in[2 * t]; cn = w0 & 0xffffffffll; hi = w0 >> 32; lo = in[2 * t + 1]; }   // the counts of all ranks sum to < 2^31
            const i128 acc = (((i128)hi) << kLimbShift) + (i128)lo;
            s_hi[t] = hi_of(acc); s_lo[t] = lo_of(acc); s_cnt[t] = (int)cn;
        }
    } else {
        const size_t cstride = (size_t)c.F * TS;
        for (int t = threadIdx.x; t < T; t += kNT) {
            i128 acc = 0;
            int cacc = 0;
            const long long *ps = c.part_sum + ((size_t)ch0 * c.F + f) * TS + t;
            const int *pc = c.part_cnt + ((size_t)ch0 * c.F + f) * TS + t;
            // Latency-bound: kFinBatch chunk partials are requested before the first is used (the 64-bit halves are summed separately so that no carry chain
            // ties a load to the previous one).  The loads are written as a batch of their own, unconditional, from a clamped chunk index: left to the scheduler
            // under k_hist_finish_wide's 64-register cap every load was completed before the next was issued (ten serial round trips for the five chunks of a
            // c3 node: 10 of the block's 22 us).
            constexpr int kFinBatch = ROOT ? 32 : (SELECT ? 16 : 8);        // (the root pass has hundreds of chunks and no counts to load)
            unsigned long long lo = 0; long long hi = 0;
            for (int ch = 0; ch < nch; ch += kFinBatch) {
                long long v[kFinBatch]; int cn[kFinBatch];
#pragma unroll
                for (int u = 0; u < kFinBatch; u++) {
                    const size_t o = (size_t)min(ch + u, nch - 1) * cstride;
                    v[u] = ps[o];
                    cn[u] = ROOT ? 0 : pc[o];
                }
#pragma unroll
                for (int u = 0; u < kFinBatch; u++)
                    if (ch + u < nch) { lo += (unsigned long long)(unsigned)v[u]; hi += (v[u] >> 32); cacc += cn[u]; }
            }
            acc += (i128)lo + (((i128)hi) << 32);
            s_hi[t] = hi_of(acc); s_lo[t] = lo_of(acc); s_cnt[t] = cacc;
        }
    }
    if (JAVA) for (int t = threadIdx.x; t < T; t += kNT) s_j[t] = c.jbin[((size_t)slot * c.F + f) * TS + t];
    if (sq_block) {
        for (int o = 32; o > 0; o >>= 1) sqacc += __shfl_xor(sqacc, o);
        if (lane_id() == 0) sh_sqw[threadIdx.x >> 6] = sqacc;
    }
    __syncthreads();
    if (sq_block && threadIdx.x == 0) { sqacc = 0; for (int w = 0; w < (kNT >> 6); w++) sqacc += sh_sqw[w]; }
    RL_CLK(clk0, 1);
    RL_TR_MARK(2);
    if (!DIST) rebuild_mode_bin(c, f, T, ch0, nch, cntB, !ROOT, s_hi, s_lo, s_cnt, sh_red, sh_redc, true, pre_tot, pre_mode);
    RL_CLK(clk0, 2);
    // prefix over t by wavefront 0: lane-local segment scan + wave scan of segment totals
    if (threadIdx.x < 64) {
        const int seg = (T + 63) / 64;
        const int b0 = min((int)threadIdx.x * seg, T), b1 = min(b0 + seg, T);
        i128 run = 0; int crun = 0;
        for (int t = b0; t < b1; t++) {
            run += make_i128(s_hi[t], s_lo[t]); crun += s_cnt[t];
            s_hi[t] = hi_of(run); s_lo[t] = lo_of(run); s_cnt[t] = crun;
        }
        i128 inc = run; int cinc = crun;
        for (int d = 1; d < 64; d <<= 1) {
            i128 u = shfl_up_i128(inc, d); int cu = __shfl_up(cinc, d);
            if ((int)threadIdx.x >= d) { inc += u; cinc += cu; }
        }
        const i128 off = inc - run; const int coff = cinc - crun;
        for (int t = b0; t < b1; t++) {
            const i128 v = make_i128(s_hi[t], s_lo[t]) + off;
            s_hi[t] = hi_of(v); s_lo[t] = lo_of(v); s_cnt[t] += coff;
        }
    } else if (JAVA && threadIdx.x == 64) {
        // sum[f][t] += sum[f][t-1] for t = 1 .. T-1, in that order (FeatureHistogram.java:141-145,189-194): one dependent chain
        double run = s_j[0];
        for (int t = 1; t < T; t++) { run = s_j[t] + run; s_j[t] = run; }
    }
    __syncthreads();

    RL_CLK(clk0, 3);
    RL_TR_MARK(3);
    const size_t slotP = ROOT ? 0 : ((size_t)nodeP * c.F + f) * TS;
    const size_t slotS = ROOT ? 0 : ((size_t)nodeS * c.F + f) * TS;
    // node totals = last cumulative bin (identical for every feature because the sums are exact)
    const i128 totB = make_i128(s_hi[T - 1], s_lo[T - 1]);
    i128 totS = 0;
    int ctotB, ctotS = 0;
    if (ROOT) {
        ctotB = c.cum_cnt[slotB + T - 1];
    } else {
        ctotB = s_cnt[T - 1];
        totS = make_i128(tp_hi, tp_lo) - totB;
        ctotS = tp_cn - ctotB;
    }
    double sumB = fixed_to_double(totB, E), sumS = fixed_to_double(totS, E);
    if (JAVA) {
        // node totals in the Java's order: the built (left) node's sumResponse is the sequential sum over its samples, the right
        // sibling's is parent - left (:202-203); B / S are whichever of the two the exact path accumulated / derived
        const double sumL = c.jtot[2 * slot];
        const double sumR = ROOT ? 0.0 : c.nodes[nodeP].sum_response - sumL;
        sumB = (sideB == 0) ? sumL : sumR; sumS = (sideB == 0) ? sumR : sumL;
    }
    Best bb = {-1.0, -1}, bs = {-1.0, -1};
    bool eqb = false, eqs = false;        // a later threshold of this thread reaches the thread's best S exactly
    bool eqbd = false, eqsd = false;      // ... with another left count (different sample sets: only possible beyond kFinThreads thresholds)
    int bbc = 0, bsc = 0;                 // left counts at the thread's best candidates
    for (int t = threadIdx.x; t < T; t += kNT) {
        const i128 vb = make_i128(s_hi[t], s_lo[t]);
        c.cum_hi[slotB + t] = s_hi[t]; c.cum_lo[slotB + t] = s_lo[t];
        int cb;
        if (ROOT) cb = c.cum_cnt[slotB + t];
        else { cb = s_cnt[t]; c.cum_cnt[slotB + t] = cb; }
        bool ok;
        double vbd, vsd = 0.0;
        if (JAVA) {
            const double jl_t = s_j[t];                                                  // left child (or root), cumulative
            const double jr_t = ROOT ? 0.0 : c.jcum[slotP + t] - jl_t;                   // FeatureHistogram.java:230
            vbd = (sideB == 0) ? jl_t : jr_t; vsd = (sideB == 0) ? jr_t : jl_t;
            c.jcum[slotB + t] = vbd;
            if (!ROOT) c.jcum[slotS + t] = vsd;
        } else vbd = fixed_to_double(vb, E);
        double S = gain_S(vbd, cb, sumB, ctotB, c.mls, ok);
        if (ok && S == bb.S) { eqb = true; eqbd |= (cb != bbc); }
        if (ok && S > bb.S) { bb.S = S; bb.t = t; bbc = cb; eqb = false; eqbd = false; }
        if (!ROOT) {
            const int it = (t - (int)threadIdx.x) / kNT;
            long long phi; unsigned long long plo; int pcn;
            if (RL_FIN_BATCH && it == 0) { phi = pre_phi[0]; plo = pre_plo[0]; pcn = pre_pcnt[0]; }
            else if (RL_FIN_BATCH && kPreIt > 1 && it == 1) { phi = pre_phi[kPreIt - 1]; plo = pre_plo[kPreIt - 1]; pcn = pre_pcnt[kPreIt - 1]; }
            else { phi = c.cum_hi[slotP + t]; plo = c.cum_lo[slotP + t]; pcn = c.cum_cnt[slotP + t]; }
            if (pcache) { s_phi[t] = phi; s_plo[t] = plo; s_pcn[t] = pcn; }
            const i128 vs = make_i128(phi, plo) - vb;      // FeatureHistogram.java:230-231
            const int cs2 = pcn - cb;
            c.cum_hi[slotS + t] = hi_of(vs); c.cum_lo[slotS + t] = lo_of(vs); c.cum_cnt[slotS + t] = cs2;
            if (!JAVA) vsd = fixed_to_double(vs, E);
            S = gain_S(vsd, cs2, sumS, ctotS, c.mls, ok);
            if (ok && S == bs.S) { eqs = true; eqsd |= (cs2 != bsc); }
            if (ok && S > bs.S) { bs.S = S; bs.t = t; bsc = cs2; eqs = false; eqsd = false; }
        }
    }
    RL_CLK(clk0, 4);
    RL_TR_MARK(4);
    const Best myb = bb, mys = bs;
    block_best2(bb, bs, sh_best, kNT >> 6);
    // exact ties inside the feature: some other threshold reaches the winner's S bit for bit (the same two sample sets: an empty-bin plateau).
    // The first one wins here as in the Java -- unless the Java's node histogram is a difference (a right child), see rl_tie.inc
    // (__syncthreads_or answers "any thread non-zero", not the bitwise OR of the arguments: one call per side)
    int tiebits = 0;
    if (!JAVA) {
        tiebits = __syncthreads_or((myb.t >= 0 && myb.S == bb.S && (myb.t != bb.t || eqb)) ? 1 : 0) ? 1 : 0;
        if (!ROOT) tiebits |= __syncthreads_or((mys.t >= 0 && mys.S == bs.S && (mys.t != bs.t || eqs)) ? 1 : 0) ? 2 : 0;
        // Do all tied thresholds cut off the SAME documents?  Thresholds of one feature are nested, so an equal left count means identical sets:
        // the partition is then known whatever the Java's noise picks and only the stored threshold has to wait for it (rl_tie.inc: deferred).
        if (tiebits & 1) {
            const int wc = ROOT ? c.cum_cnt[slotB + bb.t] : s_cnt[bb.t];
            if (__syncthreads_or((myb.t >= 0 && myb.S == bb.S && ((myb.t != bb.t && bbc != wc) || eqbd)) ? 1 : 0)) tiebits |= 4;
        }
        if (tiebits & 2) {
            const int wc = (pcache ? s_pcn[bs.t] : c.cum_cnt[slotP + bs.t]) - s_cnt[bs.t];
            if (__syncthreads_or((mys.t >= 0 && mys.S == bs.S && ((mys.t != bs.t && bsc != wc) || eqsd)) ? 1 : 0)) tiebits |= 8;
        }
    }
    RL_CLK(clk0, 5);
    RL_TR_MARK(5);

    // publish this feature's results, then count the block as arrived; the last block runs the growth bookkeeping
    __shared__ int sh_last;
    if (threadIdx.x == 0) {
        {
            const int t = max(bb.t, 0);
            publish_best(c, slot, sideB, f, bb.S, bb.t, ROOT ? c.cum_cnt[slotB + t] : s_cnt[t], s_hi[t], s_lo[t], (tiebits & 1) | ((tiebits >> 1) & 2));
        }
        if (!ROOT) {
            const int t = max(bs.t, 0);
            const i128 vs = (pcache ? make_i128(s_phi[t], s_plo[t]) : make_i128(c.cum_hi[slotP + t], c.cum_lo[slotP + t])) - make_i128(s_hi[t], s_lo[t]);
            publish_best(c, slot, 1 - sideB, f, bs.S, bs.t, (pcache ? s_pcn[t] : c.cum_cnt[slotP + t]) - s_cnt[t], hi_of(vs), lo_of(vs), ((tiebits >> 1) & 1) | ((tiebits >> 2) & 2));
        }
        if (sq_block) st_agent(&c.fb_sq[slot], (unsigned long long)sqacc);
        if (ROOT && blockIdx.x == 0) { st_agent((unsigned long long *)&c.fb_root[0], (unsigned long long)hi_of(totB)); st_agent((unsigned long long *)&c.fb_root[1], lo_of(totB)); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        RL_CLK(clk0, 6);
        if (!ROOT) RL_TR_END(2, blockIdx.y * gridDim.x + blockIdx.x);
        if (!SELECT) return;
        // two-level arrival: hundreds of blocks on ONE counter serialise in L2 (the last block saw ~11 us of it); <= 16 groups
        // of features per slot count first, the last block of a group counts on the top-level word
        const int F = (int)gridDim.x, gs = (F + 15) / 16, grp = (int)blockIdx.x / gs, ngrp = (F + gs - 1) / gs;
        const int in_grp = min(gs, F - grp * gs);
        sh_last = 0;
        // (release on arrival, acquire for the block that arrives last: ADVICE r04 -- the relaxed form rested on every producer store being a write-through
        // st_agent and on the consumer's one acquire fence; the fused kernel is the fall-back path since round 5 / 6, the ordering costs it nothing measurable)
        if (__hip_atomic_fetch_add(&st->arrive1[slot][grp], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1) {
            const int target = ROOT ? ngrp : ngrp * st_nslots;
            sh_last = (__hip_atomic_fetch_add(&st->arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == target - 1) ? 1 : 0;
        }
    }
    RL_CLK(clk0, 7);
    if (!SELECT) return;
    __syncthreads();
    if (!sh_last) return;
    // the growth steps' fused kernel carries ONE instantiation of the bookkeeping (node records in LDS: the host takes the two-launch path when
    // they do not fit, enqueue_growth_step) -- its speed depends on its size: a second inlined copy costs scalar spills and scratch in every block
    if (!ROOT && !DIST && !JAVA) select_step_t<true>(c, false, (unsigned char *)sh_raw, false);
    else select_step(c, ROOT, (unsigned char *)sh_raw, nodes_in_lds != 0, DIST);
}

template <bool ROOT, bool DIST, bool JAVA = false>
#ifndef RL_FIN_WAVES
#define RL_FIN_WAVES 4
#endif
#if RL_FIN_WAVES
__attribute__((amdgpu_waves_per_eu(RL_FIN_WAVES)))
#endif
__global__ __launch_bounds__(kFinThreads) void k_hist_finish(const Ctx c, int nodes_in_lds)
{   // grid (F, slots); the last block to arrive also runs select_step
    extern __shared__ unsigned long long sh_raw[];
    hist_finish_body<ROOT, DIST, JAVA, true>(c, nodes_in_lds, sh_raw);
}

// Wide data (hundreds of live features x kSpec slots = thousands of blocks a step): the bookkeeping that ONE block runs sets the register budget of
// all of them (96 VGPRs = 5 blocks a CU = 1280 resident blocks: a step's blocks came in two rounds and the last block waited 15-45 us for the
// second).  Without it the per-feature work needs 56 registers: 8 blocks a CU, one round; select_step then costs a launch of its own (~5 us).
__attribute__((amdgpu_waves_per_eu(8)))
__global__ __launch_bounds__(kFinWideThreads) void k_hist_finish_wide(const Ctx c)
{
    extern __shared__ unsigned long long sh_raw[];
    hist_finish_body<false, false, false, false>(c, 0, sh_raw);
}
__global__ __launch_bounds__(kFinThreads) void k_select(const Ctx c, int nodes_in_lds)
{
    extern __shared__ unsigned long long sh_raw[];
    if (c.st->done || c.st->nslots <= 0) return;        // a finished or stalled tree: the step is empty (the fused kernel's blocks all leave before they arrive)
    select_step<true>(c, false, (unsigned char *)sh_raw, nodes_in_lds != 0, false);
}

// ------------------------------------------------------------------------------------------------
// K6: stable partition of the sample lists of the step's nodes by bin[f*][k] <= t*.  grid = tiles of all slots.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_part_count(const Ctx c)
{   // sharded runs only: left members per tile
    const TreeState *st = c.st;
    const int j = slot_of_tile(st, blockIdx.x);
    if (j < 0) return;
    const SlotRec &sl = st->slot[j];
    const int cnt = sl.pcount, t = sl.t;
    const bool root = (sl.node == 0);
    const int *src = root ? nullptr : c.idx[sl.pbuf] + sl.pstart;
    const int base = (blockIdx.x - sl.tile0) * kPartTile;
    const uint16_t *b = c.bins + (size_t)sl.f * c.Npad;
    constexpr int PER = kPartTile / kThreads;
    int ks[PER]; unsigned short bv[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int pos = base + i * kThreads + threadIdx.x;
        ks[i] = (pos < cnt) ? (root ? pos : src[pos]) : -1;
    }
#pragma unroll
    for (int i = 0; i < PER; i++) bv[i] = b[max(ks[i], 0)];          // unconditional gathers (see k_part_scatter)
    int n = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) n += (ks[i] >= 0) && ((int)bv[i] <= t);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    __shared__ int part[4];
    if (lane_id() == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) c.tile_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Tile descriptors of the single-pass partition (decoupled look-back): (epoch << 34) | (status << 32) | left count.
// epoch = growth step counter, so descriptors of earlier steps are simply invalid (no clearing pass).
constexpr unsigned long long kDescAgg = 1ull, kDescPrefix = 2ull;
__device__ __forceinline__ unsigned long long make_desc(int epoch, unsigned long long status, int v)
{
    return ((unsigned long long)(epoch & 0x3fffffff) << 34) | (status << 32) | (unsigned)v;
}

// exclusive number of left members in the tiles before local tile `ltile` of this slot; publishes this tile's
// aggregate first and its inclusive prefix afterwards.  Called by wavefront 0 of the block (all 64 lanes).
// Blocks are dispatched in blockIdx order, so every tile looked at belongs to a block that is running or finished.
__device__ int lookback_exclusive(unsigned long long *desc, int ltile, int epoch, int tile_left, int *error)
{
    const int lane = lane_id();
    if (ltile == 0) {
        if (lane == 0) __hip_atomic_store(&desc[0], make_desc(epoch, kDescPrefix, tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return 0;
    }
    if (lane == 0) __hip_atomic_store(&desc[ltile], make_desc(epoch, kDescAgg, tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long tag = (unsigned long long)(epoch & 0x3fffffff);
    int excl = 0, look = ltile - 1, spins = 0;
    // kLookWin windows of 64 predecessors are requested at once: the tiles of a step run concurrently, so their aggregates are all there after one
    // memory round trip, while a prefix only appears once a tile has finished its own look-back -- walking back 64 tiles per round trip put
    // (tiles / 64) round trips on the last tile of a large node (8 for a 1 M-document parent).  The windows are consumed nearest first exactly as
    // before; the first one that is not complete yet ends the batch and is asked for again.
#ifndef RL_LOOK_WIN
#define RL_LOOK_WIN 8
#endif
    constexpr int kLookWin = RL_LOOK_WIN;
    bool found = false;
    while (!found) {
        unsigned long long dw[kLookWin];
#pragma unroll
        for (int u = 0; u < kLookWin; u++) {
            const int i = look - 64 * u - lane;               // lane 0 = nearest predecessor of the window
            dw[u] = make_desc(epoch, kDescPrefix, 0);         // before the first tile: prefix 0
            if (i >= 0) dw[u] = __hip_atomic_load(&desc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // (one reduction per batch, on the DPP path: a __shfl_xor is a ds_bpermute, and six dependent LDS round trips per window -- 48 per batch -- were
        // most of the 4-5 us a tile waited AFTER its last predecessor had published)
        bool stale = false;
        unsigned acc = 0u;
#pragma unroll
        for (int u = 0; u < kLookWin; u++) {
            if (found || stale) continue;
            const unsigned long long d = dw[u];
            const bool valid = ((d >> 34) == tag) && (((d >> 32) & 3ull) != 0ull);
            const bool isp = valid && (((d >> 32) & 3ull) == kDescPrefix);
            const unsigned long long vmask = __ballot(valid), pmask = __ballot(isp);
            const int fp = pmask ? __builtin_ctzll(pmask) : 64;                // nearest lane holding an inclusive prefix
            const unsigned long long need = (fp >= 63) ? ~0ull : ((1ull << (fp + 1)) - 1ull);
            if ((vmask & need) == need) {
                acc += (lane <= fp) ? (unsigned)d : 0u;
                if (pmask) found = true;
                else look -= 64;
            } else stale = true;
        }
        excl += (int)wave_sum_u32(acc);
        if (stale && !found) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1 << 22)) { if (lane == 0) atomicExch(error, 3); break; }      // never hang the GPU
        }
    }
    if (lane == 0) __hip_atomic_store(&desc[ltile], make_desc(epoch, kDescPrefix, excl + tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

// Two-level form of the same (round 5).  With every tile of a large node resident at once nobody finds a published PREFIX to stop at: tile i walked
// back over all i aggregates -- n^2 / 128 uncached wave loads on 15 KB of descriptors (13.6 MB at 1 841 tiles, a handful of memory channels) -- and
// the look-back ended 9-17 us after the last count had been published (profiles/r05c_step_trace_*).  Here a tile reads ONE window: the aggregates
// of its own group of 64 tiles; the last tile of a group publishes the group's total, and a tile adds the totals of the groups before its own
// (one more window per 4 096 tiles): 1 KB per tile, two dependent round trips behind the slowest publication.
__device__ __forceinline__ unsigned long long ld_desc(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ int lookback2_exclusive(unsigned long long *desc, unsigned long long *gdesc, int ltile, int epoch, int tile_left, int *error)
{
    const int lane = lane_id();
    const int g = ltile >> 6, r = ltile & 63;
    if (lane == 0) __hip_atomic_store(&desc[ltile], make_desc(epoch, kDescAgg, tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long tag = (unsigned long long)(epoch & 0x3fffffff);
    const int ngw = (g + 63) >> 6;                       // windows of group totals before this tile's group
    constexpr int kGW = 8;                               // in flight together (32 768 tiles); more are walked in further trips
    int excl = 0, spins = 0;
    // own group: aggregates of the tiles before this one
    bool have_in = (r == 0);
    unsigned gdone = 0u;                                 // bit u: window u of the group totals has been summed
    int gw0 = 0;
    while (true) {
        unsigned long long din = make_desc(epoch, kDescAgg, 0);
        if (!have_in && lane < r) din = ld_desc(&desc[(g << 6) + lane]);
        unsigned long long dg[kGW];
#pragma unroll
        for (int u = 0; u < kGW; u++) {
            dg[u] = make_desc(epoch, kDescPrefix, 0);
            const int gi = ((gw0 + u) << 6) + lane;
            if (gw0 + u < ngw && !((gdone >> u) & 1u) && gi < g) dg[u] = ld_desc(&gdesc[gi]);
        }
        unsigned acc = 0u;
        if (!have_in) {
            const bool ok = ((din >> 34) == tag) && (((din >> 32) & 3ull) != 0ull);
            if (__ballot(!ok) == 0ull) {
                const unsigned mine = (lane < r) ? (unsigned)din : 0u;
                const unsigned in_sum = wave_sum_u32(mine);
                excl += (int)in_sum;
                have_in = true;
                // the last tile of a full group publishes the group's total (nobody needs the total of the node's last, partial group)
                if (r == 63 && lane == 0)
                    __hip_atomic_store(&gdesc[g], make_desc(epoch, kDescPrefix, (int)in_sum + tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        bool all_g = true;
#pragma unroll
        for (int u = 0; u < kGW; u++) {
            if (gw0 + u >= ngw || ((gdone >> u) & 1u)) continue;
            const bool ok = ((dg[u] >> 34) == tag) && (((dg[u] >> 32) & 3ull) == kDescPrefix);
            if (__ballot(!ok) == 0ull) { acc += (unsigned)dg[u]; gdone |= 1u << u; }
            else all_g = false;
        }
        excl += (int)wave_sum_u32(acc);
        if (all_g && gw0 + kGW < ngw) { gw0 += kGW; gdone = 0u; all_g = false; if (have_in) continue; }
        if (have_in && all_g) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 22)) { if (lane == 0) atomicExch(error, 3); break; }      // never hang the GPU
    }
    return excl;
}

// (Measured and dropped, round 5: group totals ACCUMULATED by the tiles -- one agent-scope atomic add of (1 << 32 | count) per tile on its group's word,
// valid at 64 arrivals -- so that the two windows no longer depend on each other: 64 same-address atomics per word serialise at the memory side,
// c2 414 -> 364 rounds/s.)
// LOOKBACK (one GPU: the size of the left child is known from the count histogram): single pass.
// !LOOKBACK (sharded: local sizes unknown): second pass after k_part_count.
// Samples are read and written row-wise (thread t takes samples t, t+256, ..): every load is coalesced and each
// wavefront writes one contiguous run to the left list and one to the right list per row.  The fixed-point lambda of the
// built child's members is written in list order next to their ids (ql): its histogram pass reads it contiguously.
#ifndef RL_PART_WAVES
#define RL_PART_WAVES 0
#endif
template <bool LOOKBACK>
__global__ __launch_bounds__(kThreads)
#if RL_PART_WAVES
__attribute__((amdgpu_waves_per_eu(RL_PART_WAVES)))
#endif
void k_part_scatter(const Ctx c)
{
    TreeState *st = c.st;
    RL_TR_BEGIN();
    const int j = slot_of_tile(st, blockIdx.x);
    if (j < 0) return;
    const SlotRec sl = st->slot[j];                                 // (copied whole: one batch of loads)
    const int epoch = st->epoch;
    const int cnt = sl.pcount, t = sl.t, pstart = sl.pstart, pbuf = sl.pbuf;
    const bool root = (sl.node == 0);
    const bool bl = sl.build_left != 0;         // the child whose histogram is accumulated from its documents (the smaller one)
    RL_TR_MARK(1);
    const int *src = root ? nullptr : c.idx[pbuf] + pstart;
    const int ltile = blockIdx.x - sl.tile0;
    const int base = ltile * kPartTile;
    constexpr int PER = kPartTile / kThreads, NW = kThreads / 64;
    const uint16_t *b = c.bins + (size_t)sl.f * c.Npad;
    __shared__ int wl[PER * NW + 1];
    __shared__ int sh_tileoff, sh_total;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int ks[PER]; unsigned long long bal[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int pos = base + i * kThreads + threadIdx.x;
        ks[i] = (pos < cnt) ? (root ? pos : src[pos]) : -1;
    }
    // (every gather below is UNCONDITIONAL, from a clamped index: a load inside `if (member)` sits in its own exec region and the compiler completes it
    // -- s_waitcnt vmcnt(0) -- before it issues the next one: the eight bin gathers and the eight lambda gathers of a thread were sixteen serial memory
    // round trips.  Lanes that do not need a value read element 0: one broadcast line)
    bool isl[PER];
    {
        unsigned short bv[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) bv[i] = b[max(ks[i], 0)];
#pragma unroll
        for (int i = 0; i < PER; i++) isl[i] = (ks[i] >= 0) && ((int)bv[i] <= t);
    }
    RL_TR_MARK(2);
#pragma unroll
    for (int i = 0; i < PER; i++) {
        bal[i] = __ballot(isl[i]);
        if (lane == 0) wl[i * NW + wave] = __builtin_popcountll(bal[i]);
    }
    __syncthreads();
    RL_TR_MARK(3);
    if (wave == 0) {       // exclusive prefix over the (row, wave) runs of the tile
        static_assert(PER * NW <= 64, "one wave scan over the tile's (row, wave) runs");
        const int v = (lane < PER * NW) ? wl[lane] : 0;
        const int inc = (int)wave_scan_u32((unsigned)v);
        const int tile_left = (int)readlane_u32((unsigned)inc, PER * NW - 1);
        if (lane < PER * NW) wl[lane] = inc - v;
        int tileoff, nleft;
        if (LOOKBACK) {
#if RL_LOOKBACK2
            tileoff = lookback2_exclusive(c.tile_desc + sl.tile0, c.tile_gdesc + (sl.tile0 >> 6) + j, ltile, epoch, tile_left, &st->error);
#else
            tileoff = lookback_exclusive(c.tile_desc + sl.tile0, ltile, epoch, tile_left, &st->error);
#endif
            nleft = sl.nleft;
        } else {           // left members in earlier tiles, and in all tiles (= local size of the left child)
            const int *tc = c.tile_cnt + sl.tile0;
            int pre = 0, tot = 0;
            for (int i = lane; i < sl.ntiles; i += 64) { const int x = tc[i]; tot += x; if (i < ltile) pre += x; }
            for (int o = 32; o > 0; o >>= 1) { pre += __shfl_xor(pre, o); tot += __shfl_xor(tot, o); }
            tileoff = pre; nleft = tot;
        }
        if (lane == 0) { sh_tileoff = tileoff; sh_total = nleft; }
    }
    // Only the BUILT child's histogram pass reads lambda in list order, and lambda^2 is needed as one sum per child: both are fetched by document id
    // for the members of the built child alone.  The lists themselves carry document ids only: a partition moves 8 bytes per document of the parent
    // instead of 40.  The gathers are requested HERE -- after the tile's count has been published, by wavefronts 1.. while wavefront 0 waits in the
    // look-back (and by wavefront 0 after it): requested before the barrier above (round 4) they sat between a tile and the publication of its
    // count, and every later tile's look-back waits for the slowest publication before it.
    long long qv[PER], rv[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const bool mine = (ks[i] >= 0) && (isl[i] == bl);
        const int ka = mine ? ks[i] : 0;
        qv[i] = c.q[ka]; rv[i] = c.r[ka];
    }
#pragma unroll
    for (int i = 0; i < PER; i++) if (!((ks[i] >= 0) && (isl[i] == bl))) { qv[i] = 0ll; rv[i] = 0ll; }
    __syncthreads();
    const int tileoff = sh_tileoff, nleft = sh_total;
    RL_TR_MARK(4);
    int *dstL = c.idx[1 - pbuf] + pstart;
    long long *qL = c.ql[1 - pbuf] + pstart;
    if (ltile == 0 && threadIdx.x == 0) {       // local list ranges of the two children
        NodeRec &Lw = c.nodes[sl.left]; NodeRec &Rw = c.nodes[sl.right];
        Lw.start = pstart; Lw.count = nleft;
        Rw.start = pstart + nleft; Rw.count = cnt - nleft;
    }
    long long sq = 0;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int i = 0; i < PER; i++) {
        if (ks[i] < 0) continue;
        const int pos = base + i * kThreads + threadIdx.x;
        const int lbefore = tileoff + wl[i * NW + wave] + __builtin_popcountll(bal[i] & below);   // left members before pos
        const int d = isl[i] ? lbefore : nleft + (pos - lbefore);       // stable: left run, then right run
        dstL[d] = ks[i];
        if (isl[i] == bl) { qL[d] = qv[i]; sq += rv[i]; }
    }
    // fixed-point sum of lambda^2 over the tile's members of the BUILT child: one partial per tile (summed by slot_sq_left / k_hist_finish block
    // (0, slot)); thousands of atomics on one address would serialise in L2.  The sibling's sum is parent - built, exactly (integers).
    RL_TR_MARK(5);
    sq = (long long)wave_sum_u64((unsigned long long)sq);
    __shared__ long long sh_sq[NW];
    if (lane == 0) sh_sq[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) { long long v = 0; for (int w = 0; w < NW; w++) v += sh_sq[w]; c.tile_sq[blockIdx.x] = v; }
    RL_TR_END(0, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// K7: leaves.  k_leaf_table lists the leaves in ascending `start` == left-first DFS order
// (Split.leaves, Split.java:100-113): a left child always owns the front part of its parent's range.
// ------------------------------------------------------------------------------------------------
constexpr int kLeafTableCap = 1024;      // node records staged in LDS by k_leaf_table

__global__ __launch_bounds__(kThreads) void k_leaf_table(const Ctx c, const ChainBufs cb, int32_t *seg_buf)
{
    __shared__ int s_left[kLeafTableCap], s_right[kLeafTableCap], s_start[kLeafTableCap], s_buf[kLeafTableCap], s_stack[kLeafTableCap];
    TreeState *st = c.st;
    if (threadIdx.x == 0 && c.grow_docs[8] != 0ull) {       // RL_ARR_BUBBLES: device time between the bookkeeping that ended the tree and this launch
        const unsigned long long now = wall_clock64();
        c.grow_docs[4] += now - c.grow_docs[8]; c.grow_docs[5] += 1ull; c.grow_docs[8] = 0ull;
    }
    const int nn = st->n_nodes;
    if (nn <= kLeafTableCap) {
        // the walk is a chain of dependent reads: stage the few fields it needs in LDS first (one round trip to memory)
        for (int x = threadIdx.x; x < nn; x += kThreads) {
            const NodeRec &X = c.nodes[x];
            s_left[x] = X.left; s_right[x] = X.right; s_start[x] = X.start; s_buf[x] = X.buf;
        }
        __syncthreads();
        if (threadIdx.x != 0) return;
        // pre-order walk, left first; the chain plan (one segment per leaf, rl_chain.inc) is written as the leaves appear
        int n = 0, sp = 0, tiles = 0, prev = 0;
        s_stack[sp++] = 0;
        while (sp > 0) {
            const int x = s_stack[--sp];
            if (s_left[x] < 0) {
                const int start = s_start[x];
                if (n > 0) tiles += (start - prev + kChainTile - 1) / kChainTile;
                c.leaf_node[n] = x; c.leaf_start[n] = start;
                cb.seg_start[n] = start; cb.seg_tile0[n] = tiles;
                seg_buf[n] = (x == 0) ? -1 : s_buf[x];
                prev = start; n++;
            } else { s_stack[sp++] = s_right[x]; s_stack[sp++] = s_left[x]; }      // depth <= splits < nn
        }
        if (n > 0) tiles += (c.N - prev + kChainTile - 1) / kChainTile;
        for (int i = n; i <= c.L + 1; i++) c.leaf_start[i] = c.N;      // unused leaf slots are empty segments
        st->n_leaves = n;
        cb.seg_start[n] = c.N; cb.seg_tile0[n] = tiles;
        cb.plan->n_seg = n; cb.plan->n = c.N; cb.plan->n_tiles = tiles; cb.plan->n_chunks = tiles + n;
        return;
    }
    if (threadIdx.x != 0) return;
    // very large trees: insertion sort of all leaves by start, straight from memory
    int n = 0;
    for (int x = 0; x < nn; x++) if (c.nodes[x].left < 0 && c.nodes[x].fid >= 0) {
        int i = n++;
        while (i > 0 && c.leaf_start[i - 1] > c.nodes[x].start) { c.leaf_start[i] = c.leaf_start[i - 1]; c.leaf_node[i] = c.leaf_node[i - 1]; i--; }
        c.leaf_start[i] = c.nodes[x].start; c.leaf_node[i] = x;
    }
    for (int i = n; i <= c.L + 1; i++) c.leaf_start[i] = c.N;
    st->n_leaves = n;
    int tiles = 0;
    for (int i = 0; i < n; i++) {
        cb.seg_start[i] = c.leaf_start[i];
        cb.seg_tile0[i] = tiles;
        tiles += (c.leaf_start[i + 1] - c.leaf_start[i] + kChainTile - 1) / kChainTile;
        seg_buf[i] = (c.leaf_node[i] == 0) ? -1 : c.nodes[c.leaf_node[i]].buf;
    }
    cb.seg_start[n] = c.N; cb.seg_tile0[n] = tiles;
    cb.plan->n_seg = n; cb.plan->n = c.N; cb.plan->n_tiles = tiles; cb.plan->n_chunks = tiles + n;
}

// leaf output = s1 / s2 in float, 0 when s2 == 0   (LambdaMART.java:409-413)
__global__ __launch_bounds__(kThreads) void k_leaf_output(const Ctx c, const ChainBufs cb)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && cb.stats[3] != 0) {       // RL_ARR_BUBBLES: device time since the chain's last stitch pass ended (10 ns units, 32 bits)
        c.grow_docs[6] += (unsigned long long)(unsigned)((int)wall_clock64() - cb.stats[3]); c.grow_docs[7] += 1ull; cb.stats[3] = 0;
    }
    const int li = blockIdx.x * kThreads + threadIdx.x;
    if (li >= c.st->n_leaves) return;
    const float s1 = cb.result[li], s2 = cb.result[cb.maxseg + li];
    NodeRec &X = c.nodes[c.leaf_node[li]];
    if (c.mart) X.output = s1 / (float)X.gcount;                  // MART.updateTreeOutput (MART.java:54-65): float sum / int count
    else X.output = (s2 == 0.f) ? 0.f : s1 / s2;
}

__global__ void k_metric_finish(const ChainBufs cb, int n, float *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = cb.result[0] / (float)n;    // LambdaMART.java:470
}

// one wavefront per leaf: the two Java float running sums, element by element, in sample order
// (LambdaMART.java:401-413).  64 samples are fetched in parallel, then chained through readlane.
__global__ __launch_bounds__(64) void k_leaf_chain(const Ctx c)
{
    const TreeState *st = c.st;
    const int li = blockIdx.x;
    if (li >= st->n_leaves) return;
    const int node = c.leaf_node[li];
    NodeRec &X = c.nodes[node];
    const bool root = (node == 0);
    const int *idx = root ? nullptr : c.idx[X.buf] + X.start;
    const int cnt = X.count;
    float s1 = 0.f, s2 = 0.f;
    for (int base = 0; base < cnt; base += 64) {
        const int i = base + lane_id();
        double x1 = 0.0, x2 = 0.0;
        if (i < cnt) { const int k = root ? i : idx[i]; const double2 v = c.lw[k]; x1 = v.x; x2 = v.y; }
        const int m = min(64, cnt - base);
        const uint32_t a0 = (uint32_t)d2bits(x1), a1 = (uint32_t)(d2bits(x1) >> 32);
        const uint32_t b0 = (uint32_t)d2bits(x2), b1 = (uint32_t)(d2bits(x2) >> 32);
#pragma unroll
        for (int j = 0; j < 64; j++) {
            if (j < m) {
                const uint64_t ua = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)a1, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)a0, j);
                const uint64_t ub = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)b1, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)b0, j);
                s1 = float_chain_step(s1, bits2d(ua));
                s2 = float_chain_step(s2, bits2d(ub));
            }
        }
    }
    if (lane_id() == 0) X.output = c.mart ? s1 / (float)X.gcount : ((s2 == 0.f) ? 0.f : s1 / s2);     // :409-413 / MART.java:64
}

// A block takes runs of kScoreBatch x kThreads consecutive leaf-order positions: the leaf of a position is a search in the LDS copy of the leaf
// table, whose entries carry the list buffer and the step lr * output of the leaf (no dependent load of the node record), and the kScoreBatch
// document ids, then the kScoreBatch scores, of a thread are requested together (unconditional loads from clamped positions: a load inside a
// per-lane condition is completed before the next one is issued).
constexpr int kScoreBatch = 4;
__global__ __launch_bounds__(kThreads) void k_score_update(const Ctx c)
{
    __shared__ int s_start[1024 + 1];
    __shared__ int s_buf[1024];
    __shared__ double s_step[1024];
    const TreeState *st = c.st;
    const int nl = st->n_leaves;
    const bool use_lds = nl <= 1024;
    if (use_lds) {
        for (int i = threadIdx.x; i <= nl; i += kThreads) s_start[i] = c.leaf_start[i];
        for (int i = threadIdx.x; i < nl; i += kThreads) {
            const int node = c.leaf_node[i];
            const NodeRec &X = c.nodes[node];
            s_buf[i] = (node == 0) ? -1 : X.buf;
            s_step[i] = (double)c.lr * (double)X.output;                  // LambdaMART.java:208
        }
        __syncthreads();
    }
    const int N = c.N;
    if (!use_lds) {
        for (int p = blockIdx.x * kThreads + threadIdx.x; p < N; p += gridDim.x * kThreads) {
            int lo = 0, hi = nl - 1;                       // last leaf with start <= p
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (c.leaf_start[mid] <= p) lo = mid; else hi = mid - 1; }
            const int node = c.leaf_node[lo];
            const NodeRec &X = c.nodes[node];
            const int k = (node == 0) ? p : c.idx[X.buf][p];
            c.scores[k] += (double)c.lr * (double)X.output;
        }
        return;
    }
    constexpr int RUN = kScoreBatch * kThreads;
    for (int base = blockIdx.x * RUN; base < N; base += gridDim.x * RUN) {
        int p[kScoreBatch], k[kScoreBatch]; double step[kScoreBatch], sc[kScoreBatch];
        int buf[kScoreBatch];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) {
            p[u] = min(base + u * kThreads + (int)threadIdx.x, N - 1);
            int lo = 0, hi = nl - 1;                       // last leaf with start <= p
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_start[mid] <= p[u]) lo = mid; else hi = mid - 1; }
            buf[u] = s_buf[lo]; step[u] = s_step[lo];
        }
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) k[u] = c.idx[max(buf[u], 0)][p[u]];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) { if (buf[u] < 0) k[u] = p[u]; }
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) sc[u] = c.scores[k[u]];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++)
            if (base + u * kThreads + (int)threadIdx.x < N) c.scores[k[u]] = sc[u] + step[u];
    }
}

// The same update as a stream over the documents: the leaf of every document was left behind by the gather of the leaf sums (ChainSource::seg_of),
// so a document costs one 2-byte and one 8-byte coalesced read and one coalesced write -- through the leaves' lists every document is an 8-byte
// read-modify-write at a random address, a memory sector each way (68 -> ~20 us at 3.77 M documents).  modelScores[k] += learningRate * output
// (LambdaMART.java:203-210), the same double product.
__global__ __launch_bounds__(kThreads) void k_score_stream(const Ctx c)
{
    __shared__ double s_step[1024];
    const TreeState *st = c.st;
    const int nl = st->n_leaves;
    for (int i = threadIdx.x; i < nl; i += kThreads) s_step[i] = (double)c.lr * (double)c.nodes[c.leaf_node[i]].output;                  // LambdaMART.java:208
    __syncthreads();
    const int N = c.N;
    constexpr int RUN = kScoreBatch * kThreads;
    for (int base = blockIdx.x * RUN; base < N; base += gridDim.x * RUN) {
        int k[kScoreBatch]; unsigned short lf[kScoreBatch]; double sc[kScoreBatch];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) { k[u] = min(base + u * kThreads + (int)threadIdx.x, N - 1); lf[u] = c.leaf_of[k[u]]; sc[u] = c.scores[k[u]]; }
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++)
            if (base + u * kThreads + (int)threadIdx.x < N) c.scores[k[u]] = sc[u] + s_step[min((int)lf[u], 1023)];
    }
}

// ------------------------------------------------------------------------------------------------
// K8: per-round metric: NDCG per query comes from k_rank_*, the float running mean is below / in rl_chain.inc
// ------------------------------------------------------------------------------------------------
// float s = 0; for q: s += score_q; s / Q      (LambdaMART.java:469-471,474-483)
__global__ __launch_bounds__(64) void k_float_mean(const double *v, int n, float *out)
{
    float s = 0.f;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane_id();
        const double x = (i < n) ? v[i] : 0.0;
        const uint32_t a0 = (uint32_t)d2bits(x), a1 = (uint32_t)(d2bits(x) >> 32);
        const int m = min(64, n - base);
#pragma unroll
        for (int j = 0; j < 64; j++) {
            if (j < m) {
                const uint64_t ua = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)a1, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)a0, j);
                s = float_chain_step(s, bits2d(ua));
            }
        }
    }
    if (lane_id() == 0) *out = s / (float)n;
}

// double mean in list order  (MetricScorer.score(List), metric/MetricScorer.java:46-52)
__global__ __launch_bounds__(64) void k_double_mean(const double *v, int n, double *out)
{
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n; i++) s += v[i];
    *out = s / n;
}

// ------------------------------------------------------------------------------------------------
// tree bookkeeping: copy the grown tree into the ensemble (creation order), evaluate it on raw rows
// ------------------------------------------------------------------------------------------------
struct EnsTree {   // device layout of one kept tree, node i at [tree*MAXN + i]
    int32_t *feat_idx;   // column index, -1 = leaf
    float *thr;
    int32_t *left, *right;
    float *out;
    int32_t *n_nodes;    // [n_trees]
    int32_t *count;      // training samples per node (diagnostic)
    double *deviance;
};

__global__ __launch_bounds__(kThreads) void k_export_tree(const Ctx c, const EnsTree e, int tree)
{   // only committed nodes (fid >= 0) are part of the tree; fid = creation order of the committed splits
    const TreeState *st = c.st;
    const int nn = st->n_nodes;
    for (int i = threadIdx.x; i < nn; i += kThreads) {
        const NodeRec &X = c.nodes[i];
        if (X.fid < 0) continue;
        const size_t o = (size_t)tree * c.MAXN + X.fid;
        const bool leaf = X.left < 0;
        e.feat_idx[o] = leaf ? -1 : (c.vcol ? c.vcol[X.best_f] : X.best_f);          // the column of the row matrix (a virtual feature's real column)
        e.thr[o] = leaf ? 0.f : c.thr[(size_t)X.best_f * c.TS + X.best_t];
        e.left[o] = leaf ? -1 : c.nodes[X.left].fid; e.right[o] = leaf ? -1 : c.nodes[X.right].fid;
        e.out[o] = leaf ? X.output : 0.f;
        e.count[o] = X.gcount;
        e.deviance[o] = X.deviance;
    }
    if (threadIdx.x == 0) e.n_nodes[tree] = 2 * st->n_splits + 1;
}

// Split.eval (Split.java:115-125) of tree `tree` on row-major rows; adds lr*out to the running double
// scores of the validation set (LambdaMART.java:230-234).
__global__ __launch_bounds__(kThreads) void k_valid_update(const EnsTree e, int MAXN, int tree, const float *X, int n, int F,
                                                            float lr, double *vscores)
{
    const size_t o = (size_t)tree * MAXN;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const float *row = X + (size_t)i * F;
        int nd = 0;
        while (e.feat_idx[o + nd] != -1) nd = (row[e.feat_idx[o + nd]] <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
        vscores[i] += (double)lr * (double)e.out[o + nd];
    }
}

// Ensemble.eval (Ensemble.java:110-116): float s; s += tree.eval(dp) * weight   for trees 0..nt-1.
// rows: row-major [n][stride]; column of feature index f is colmap ? colmap[f] : f.
__global__ __launch_bounds__(kThreads) void k_ensemble_eval(const EnsTree e, int MAXN, int nt, const float *X, int64_t n,
                                                             int stride, float w, float *out, double *out_d)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = X + (size_t)i * stride;
        float s = 0.f;
        for (int t = 0; t < nt; t++) {
            const size_t o = (size_t)t * MAXN;
            int nd = 0;
            while (e.feat_idx[o + nd] != -1) {
                const int fc = e.feat_idx[o + nd];
                const float v = (fc < stride) ? row[fc] : 0.f;
                nd = (v <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
            }
            s = (float)((double)s + (double)e.out[o + nd] * (double)w);
        }
        if (out) out[i] = s;
        if (out_d) out_d[i] = (double)s;
    }
}

}  // namespace rl
