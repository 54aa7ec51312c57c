// rl_kernels_init.inc -- one-time kernels of LambdaMART.init() (K9): SoA transpose, candidate thresholds,
// binning, root counts.  Replaces learning/tree/LambdaMART.java:93-150 and
// learning/tree/FeatureHistogram.java:75-112 without the F index sorts of N doubles: the threshold table only
// needs (min, max, the distinct values if there are few of them), and the bin of a value is a lower bound
// in that table.

namespace rl {

// X row-major [N][F]  ->  Xt feature-major [F][Npad]   (32x32 LDS tile transpose, both sides coalesced)
__global__ __launch_bounds__(kThreads) void k_transpose(const float *X, float *Xt, int N, int F, int Npad)
{
    __shared__ float tile[32][33];
    const int k0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, f = f0 + tx;
        tile[r][tx] = (k < N && f < F) ? X[(size_t)k * F + f] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int f = f0 + r, k = k0 + tx;
        if (f < F && k < N) Xt[(size_t)f * Npad + k] = tile[tx][r];
    }
}

struct FeatStats {
    uint32_t *minkey, *maxkey;   // [F] ordered float keys
    uint32_t *set;               // [F][HS] open-addressing set of distinct value keys (0 = empty)
    int32_t *nset;               // [F] entries in the set
    int32_t *overflow;           // [F] more than `limit` distinct values
    int32_t *bad;                // [1] non-finite input seen
    int32_t HS, limit;
};

__device__ __forceinline__ uint32_t hash_key(uint32_t k) { k ^= k >> 16; k *= 0x7feb352du; k ^= k >> 15; k *= 0x846ca68bu; k ^= k >> 16; return k; }

// insert into an open-addressing table; returns 1 if newly inserted, 0 if present, -1 if the table is full
__device__ __forceinline__ int set_insert(uint32_t *tab, int HS, uint32_t key)
{
    uint32_t h = hash_key(key) & (uint32_t)(HS - 1);
    for (int probe = 0; probe < HS; probe++) {
        const uint32_t old = atomicCAS(&tab[h], 0u, key);
        if (old == 0u) return 1;
        if (old == key) return 0;
        h = (h + 1) & (uint32_t)(HS - 1);
    }
    return -1;
}

// grid (F, slices).  Per feature: min / max and the set of distinct values while it stays <= limit.
// -0.0 is folded into +0.0 (Java compares by value, so both are "the same distinct value").
__global__ __launch_bounds__(kThreads) void k_feat_stats(const float *Xt, int N, int Npad, FeatStats fs)
{
    extern __shared__ uint32_t lset[];
    __shared__ int lcount, lover;
    const int f = blockIdx.x;
    for (int i = threadIdx.x; i < fs.HS; i += kThreads) lset[i] = 0;
    if (threadIdx.x == 0) { lcount = 0; lover = 0; }
    __syncthreads();
    const float *col = Xt + (size_t)f * Npad;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    bool bad = false;
    const int per = (N + gridDim.y - 1) / gridDim.y;
    const int k0 = blockIdx.y * per, k1 = min(N, k0 + per);
    const bool skip_set = fs.overflow[f] != 0;
    for (int k = k0 + threadIdx.x; k < k1; k += kThreads) {
        float v = col[k];
        if (v == 0.f) v = 0.f;                         // folds -0.0
        if (v != v) bad = true;                        // NaN only: +-Infinity is a value like any other (it sorts last / first: float_key)
        const uint32_t key = float_key(v);
        kmin = min(kmin, key); kmax = max(kmax, key);
        if (!skip_set && !lover) {
            const int r = set_insert(lset, fs.HS, key);
            if (r != 0) { if (r < 0 || atomicAdd(&lcount, 1) + 1 > fs.limit) lover = 1; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o)); kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o)); }
    if (lane_id() == 0 && k0 < k1) { atomicMin(&fs.minkey[f], kmin); atomicMax(&fs.maxkey[f], kmax); }
    if (bad) atomicExch(fs.bad, 1);
    __syncthreads();
    if (lover) { if (threadIdx.x == 0) atomicExch(&fs.overflow[f], 1); return; }
    if (skip_set) return;
    uint32_t *gset = fs.set + (size_t)f * fs.HS;
    for (int i = threadIdx.x; i < fs.HS; i += kThreads) {
        const uint32_t key = lset[i];
        if (key == 0u) continue;
        if (fs.overflow[f]) break;
        const int r = set_insert(gset, fs.HS, key);
        if (r != 0) { if (r < 0 || atomicAdd(&fs.nset[f], 1) + 1 > fs.limit) atomicExch(&fs.overflow[f], 1); }
    }
}

// one block per feature: the threshold table  (LambdaMART.java:135-149)
__global__ __launch_bounds__(kThreads) void k_thresholds(FeatStats fs, int nThreshold, int TS, float *thr, int32_t *nthr)
{
    extern __shared__ uint32_t keys[];
    const int f = blockIdx.x;
    float *out = thr + (size_t)f * TS;
    if (fs.overflow[f]) {
        if (threadIdx.x == 0) {
            const float fmin = key_float(fs.minkey[f]), fmax = key_float(fs.maxkey[f]);
            const float step = fabsf(fmax - fmin) / (float)nThreshold;          // :142 (float arithmetic)
            float v = fmin;
            out[0] = v;
            for (int j = 1; j < nThreshold; j++) { v = v + step; out[j] = v; }  // :145-147 float adds
            out[nThreshold] = 3.4028234663852886e38f;                           // Float.MAX_VALUE
            nthr[f] = nThreshold + 1;
        }
        return;
    }
    // bitonic sort of the (<= limit) distinct keys; empty slots become +inf keys
    const int HS = fs.HS;
    const uint32_t *gset = fs.set + (size_t)f * HS;
    for (int i = threadIdx.x; i < HS; i += kThreads) { const uint32_t k = gset[i]; keys[i] = k ? k : 0xFFFFFFFFu; }
    __syncthreads();
    for (int size = 2; size <= HS; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < HS / 2; i += kThreads) {
                const int lo = (i / stride) * (stride << 1) + (i % stride), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const uint32_t a = keys[lo], b = keys[hi];
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    }
    const int m = fs.nset[f];
    for (int i = threadIdx.x; i < m; i += kThreads) out[i] = key_float(keys[i]);
    if (threadIdx.x == 0) { out[m] = 3.4028234663852886e38f; nthr[f] = m + 1; }   // :136-140
}

// bin = smallest t with value <= thr[t]  (FeatureHistogram.java:88-107), stored as uint16; also the
// (non-cumulative) root count histogram.
__global__ __launch_bounds__(kThreads) void k_binning(const float *Xt, int N, int Npad, int TS, const float *thr,
                                                      const int32_t *nthr, uint16_t *bins, uint16_t *gbins, int32_t *rootcnt, const int32_t *vcol)
{
    extern __shared__ unsigned char sraw[];
    float *sthr = (float *)sraw;
    unsigned *scnt = (unsigned *)(sthr + TS);
    const int f = blockIdx.x;
    const int T = nthr[f];
    for (int i = threadIdx.x; i < T; i += kThreads) { sthr[i] = thr[(size_t)f * TS + i]; scnt[i] = 0; }
    __syncthreads();
    const float *col = Xt + (size_t)(vcol ? vcol[f] : f) * Npad;        // (several virtual features read one column: rl_init)
    uint16_t *bo = bins + (size_t)f * Npad;
    const int per = (N + gridDim.y - 1) / gridDim.y;
    const int k0 = blockIdx.y * per, k1 = min(N, k0 + per);
    // Infinite values (the reference accepts them, learning/tree/LambdaMART.java:108-149): a table of distinct values simply holds +-Infinity as a
    // value ([.., +Inf, MAX_VALUE]: the search below still lands on the first t with v <= thr[t]); a 256-step table of a column whose maximum is
    // +Infinity is [fmin, Inf, Inf, .., MAX_VALUE]; and one whose minimum is -Infinity is [-Inf, NaN, NaN, .., MAX_VALUE] (step = Inf, -Inf + Inf):
    // the Java's loop `value > threshold` never breaks on a NaN, so every document above -Infinity lands in bin 1.
    const bool nan_table = T > 2 && sthr[1] != sthr[1];
    for (int k = k0 + threadIdx.x; k < k1; k += kThreads) {
        const float v = col[k];
        int lo = 0, hi = T - 1;                 // thr[T-1] = MAX_VALUE >= every finite v
        if (nan_table) lo = hi = (v <= sthr[0]) ? 0 : 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (v <= sthr[mid]) hi = mid; else lo = mid + 1; }
        bo[k] = (uint16_t)lo;
        gbins[((size_t)(f / kHistFG) * Npad + k) * kHistFG + (f % kHistFG)] = (uint16_t)(lo * 8);     // histogram layout: pre-scaled (k_hist)
        atomicAdd(&scnt[lo], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += kThreads) if (scnt[i]) atomicAdd(&rootcnt[(size_t)f * TS + i], (int)scnt[i]);
}

// dbins[k][g][0..15] = gbins[g][k][0..15]; a document's row is `gstride` groups long (numFG rounded up so that rows start on 128-byte lines)
__global__ __launch_bounds__(kThreads) void k_docmajor(const uint16_t *gbins, uint16_t *dbins, int Npad, int numFG, int gstride)
{
    const size_t total = (size_t)Npad * numFG;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const size_t k = i / numFG; const int g = (int)(i - k * numFG);
        const uint4 *src = (const uint4 *)(gbins + ((size_t)g * Npad + k) * kHistFG);
        uint4 *dst = (uint4 *)(dbins + (k * gstride + g) * kHistFG);
        dst[0] = src[0]; dst[1] = src[1];
    }
}

// compact rows (rl_k_hist.inc, hist_chunk<.., CR>): per (document, group) the entries outside the columns' mode bins as 16-bit words
// (column-in-group << 12 | bin), ascending, padded with 0xffff; more than eight entries: first word 0xfffe (the dense row is read instead).
// crows [Npad][cr_stride] uint4, document-major.  stats[2 g] += entries of group g, stats[2 g + 1] += its rows with more than eight
// (a thread walks consecutive (document, group) pairs of ONE group stripe: i = g * Npad + k, so a wavefront's counts belong to one group
// except at a stripe's end).
__global__ __launch_bounds__(kThreads) void k_compact_rows(const uint16_t *gbins, const int32_t *mode, uint4 *crows, int N, int Npad, int numFG, int cr_stride, int F,
                                                           unsigned long long *stats)
{
    const size_t total = (size_t)Npad * numFG;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int g = (int)(i / Npad); const size_t k = i - (size_t)g * Npad;
        unsigned long long ents = 0, over = 0;
        unsigned short e[8];
#pragma unroll
        for (int u = 0; u < 8; u++) e[u] = 0xffffu;
        int n = 0;
        if ((int)k < N) {
            const uint16_t *row = gbins + ((size_t)g * Npad + k) * kHistFG;
            for (int j = 0; j < kHistFG; j++) {
                const int f = g * kHistFG + j;
                if (f >= F) break;
                const int bin = row[j] >> 3;                    // gbins holds 8 * bin
                if (bin != mode[f]) { if (n < 8) e[n] = (unsigned short)((j << 12) | bin); n++; }
            }
        }
        if (n > 8) { e[0] = 0xfffeu; over++; }
        ents += (unsigned long long)n;
        uint4 v;
        v.x = (unsigned)e[0] | ((unsigned)e[1] << 16); v.y = (unsigned)e[2] | ((unsigned)e[3] << 16);
        v.z = (unsigned)e[4] | ((unsigned)e[5] << 16); v.w = (unsigned)e[6] | ((unsigned)e[7] << 16);
        crows[k * (size_t)cr_stride + g] = v;
        // per-group totals: lanes of the same group fold first (Npad is a multiple of 64: a wavefront never straddles two stripes)
        for (int o = 32; o > 0; o >>= 1) { ents += __shfl_xor(ents, o); over += __shfl_xor(over, o); }
        if (lane_id() == 0) { atomicAdd(&stats[2 * g], ents); atomicAdd(&stats[2 * g + 1], over); }
    }
}

// packed rows from the (pre-scaled) 16-bit rows: pbins / phib group-major, pdbins document-major (rl_k_hist.inc pbin8_of)
__global__ __launch_bounds__(kThreads) void k_pack_rows(const uint16_t *gbins, unsigned char *pbins, uint16_t *phib, unsigned char *pdbins, int Npad, int numFG, int pd_stride)
{
    const size_t total = (size_t)Npad * numFG;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const size_t k = i % Npad; const int g = (int)(i / Npad);
        const uint4 *src = (const uint4 *)(gbins + ((size_t)g * Npad + k) * kHistFG);
        const uint4 a = src[0], b = src[1];
        const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        unsigned lo[4] = {0u, 0u, 0u, 0u}, mask = 0u;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const unsigned bin = (((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu)) >> 3);       // gbins holds 8 * bin
            const unsigned bit = bin >> 8;                                                           // only bin 256 can exceed a byte
            lo[j >> 2] |= (bin - bit) << (8 * (j & 3));
            mask |= bit << j;
        }
        const uint4 v = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        *(uint4 *)(pbins + ((size_t)g * Npad + k) * 16) = v;
        phib[(size_t)g * Npad + k] = (uint16_t)mask;
        if (pdbins) {
            *(uint4 *)(pdbins + k * (size_t)pd_stride + 16 * g) = v;
            *(uint16_t *)(pdbins + k * (size_t)pd_stride + 16 * numFG + 2 * g) = (uint16_t)mask;
        }
    }
}

__global__ __launch_bounds__(64) void k_cumulate_counts(int TS, const int32_t *nthr, int32_t *rootcnt, int32_t *mode)
{
    if (threadIdx.x != 0) return;
    int32_t *c = rootcnt + (size_t)blockIdx.x * TS;
    const int T = nthr[blockIdx.x];
    int best = 0;
    for (int t = 1; t < T; t++) if (c[t] > c[best]) best = t;     // most populated bin (lowest index on ties)
    mode[blockIdx.x] = best;
    for (int t = 1; t < T; t++) c[t] += c[t - 1];
}

// Which columns come in RUNS: of the documents outside the column's mode bin, how many are followed (in document order) by a document with
// the same bin.  Query-level features (one value per query: query length, IDF sums, ...) are runs of a whole ranked list; k_hist<.., RUNS>
// folds the four samples of a quad into one LDS atomic for such columns.  grid F, out[f] = (documents outside the mode, of them followed by an equal bin)
__global__ __launch_bounds__(kThreads) void k_run_stats(const uint16_t *bins, const int32_t *mode, int N, int Npad, unsigned long long *out)
{
    const int f = blockIdx.x;
    const uint16_t *b = bins + (size_t)f * Npad;
    const unsigned m = (unsigned)mode[f];
    unsigned long long tot = 0, same = 0;
    for (int k = threadIdx.x; k + 1 < N; k += kThreads) {
        const unsigned x = b[k];
        if (x != m) { tot++; same += (x == (unsigned)b[k + 1]); }
    }
    for (int o = 32; o > 0; o >>= 1) { tot += __shfl_xor(tot, o); same += __shfl_xor(same, o); }
    __shared__ unsigned long long sh[2 * (kThreads / 64)];
    if (lane_id() == 0) { sh[2 * (threadIdx.x >> 6)] = tot; sh[2 * (threadIdx.x >> 6) + 1] = same; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; w++) { tot += sh[2 * w]; same += sh[2 * w + 1]; }
        out[2 * f] = tot; out[2 * f + 1] = same;
    }
}

}  // namespace rl
