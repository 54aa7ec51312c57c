// rl_kernels_round.inc -- gfx950 kernels of one boosting round (included by rl_trainer.hip).  K1 .. K3 and K7 .. K10 are in this file; the
// growth step of a tree (K4 .. K6) is included between them, one rl_k_*.inc piece per stage.
//
// K1  k_rank_*, k_lambda_fused / k_pair_terms + k_lambda_acc, k_mart_residual, k_max_reduce
//                       per-query stable rank + pairwise swap change x sigmoid   LambdaMART.java:361-396, MART.java:47-51
// K1b k_quantize        lambda -> order-independent fixed point                   (DESIGN.md 3 "exact sums")
// K2/3 k_hist<ROOT>     LDS-staged per-chunk histograms                           FeatureHistogram.java:126-146,166-195
// K4/5 k_hist_finish    chunk reduction, prefix over thresholds, sibling = parent - built child, per-feature gain scan
//      rl_k_finish.inc (its helpers and k_hist_reduce: rl_k_reduce.inc; the per-feature best-split exchange: rl_k_best.inc)
//                                                                                 FeatureHistogram.java:141-145,189-194,222-264
//      select_step      (last block of k_hist_finish) best-first growth bookkeeping, speculative slots
//      rl_k_select.inc                                                            RegressionTree.java:58-87,147-157
// K6  k_part_scatter<LOOKBACK> (+ k_part_count when sharded)  stable partition    FeatureHistogram.java:328-341
//      rl_k_partition.inc
// K7  k_leaf_table, k_leaf_output, k_score_update (+ rl_chain.inc)                LambdaMART.java:398-415, 203-210
// K8  per-query metric in k_rank_*, float mean via rl_chain.inc / k_float_mean    LambdaMART.java:442-483
// K10 k_ensemble_eval, k_valid_update (k_model_eval* live in rl_model_eval.inc)   Ensemble.java:110-116, Split.java:115-125

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

}  // namespace rl

// K4/K5 and K6, the growth step of a tree: one piece per stage, each a namespace rl block of its own, in dependency order
#include "rl_k_reduce.inc"
#include "rl_k_best.inc"
#include "rl_k_select.inc"
#include "rl_k_finish.inc"
#include "rl_k_partition.inc"

namespace rl {

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
