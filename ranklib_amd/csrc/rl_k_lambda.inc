// rl_k_lambda.inc -- K1, second part: the pseudo-responses of a round from the ranked lists that k_rank_* left.  LambdaMART's lambdas and weights
// (LambdaMART.java:361-396; the metrics' swap changes: DCGScorer.java, APScorer.java, ERRScorer.java, ReciprocalRankScorer.java, PrecisionScorer.java)
// in three forms -- k_pair_terms + k_lambda_acc, k_lambda_fused, k_lambda_tiny -- and MART's residuals (k_mart_residual, MART.java:47-51).  LamArgs,
// block_store_max and k_max_reduce (max |lambda|, which K1b scales by), swap_change_abs, PairPre and the pair-term halves, err_swap_abs, and
// the three k_*_probe kernels the tests read exp / rho / division through.
// Included by rl_kernels_round.inc; needs that file's helpers ahead of the include (gain_of) and rl_k_rank.inc (group_sync).

namespace rl {

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

}  // namespace rl
