// rl_k_rank.inc -- K1, first part, and K8's per-query metric: the stable descending rank of every query (MergeSorter.sort,
// utilities/MergeSorter.java:134-189) and the scorer's value of that ranking (DCGScorer.java:97-103, APScorer.java:86-94, ERRScorer.java:71-73).
// group_sync, RankArgs, rank_metric, rank_query and the five k_rank_* kernels, one per class of list length (launch_rank, rl_launch.inc, picks them).
// Included by rl_kernels_round.inc; needs that file's helpers ahead of the include (java_pow2m1, gain_of) and none of the other pieces.

namespace rl {

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

}  // namespace rl
