// rl_ale.inc -- accumulated local effects (ALE) of a tree model in one pass over a file: per column every document is scored at the two
// edges of the interval its own value lies in, and the differences are counted and summed per interval in one fixed order, without a
// substituted copy of the rows and without the K + 1 cells per document a grid of all edges would walk.  DESIGN.md 39.
// Included at the end of rl_trainer.hip, after rl_partial2.inc (it uses DevPool, StageEvents and kStageScratchDefault).  The integer
// bookkeeping of a call -- checks, chunks, batches, uses -- is rl_ale_host.h's.
//
//   k_model_ale_scores<B>   one lane per document, blockIdx.y over the chunk's batches.  A batch is up to B consecutive COLUMNS; their ids
//                           and edge counts are wave-uniform scalars, their edges are staged in the LDS once per block.  Per document and
//                           column the lane finds its interval by a binary search there and keeps the two edges z_lo, z_hi and two float
//                           chains in registers: 2 B chains per lane.  A document outside the edges takes its own value for both, so it
//                           can never part and scores its base twice.  Per tree:
//                             * uses[batch][tree] == 0 (exact: no node of the tree tests a column of the batch): one walk, its output
//                               joins all 2 B chains;
//                             * otherwise the base walk is made once on the document's own row.  At a node on it that tests column u of
//                               the batch both substitutes are compared with the threshold too; a side that goes the other way walks on
//                               from the other child with its substitute standing in at every later node that tests the column -- the
//                               parting rule of k_model_partial_scores, with lane-private values.  Sides that never part take the base
//                               output; the bits of uses say which columns can have parted at all.
//                           The own value lies between the two substitutes, so with narrow intervals a side parts rarely and a batch costs
//                           little more than one walk of these arrays (measured: DESIGN.md 39.4).  The base, where asked for, is one
//                           launch more with an empty batch.  Each
//                           chain is Ensemble.eval's statement s = (float)((double)s + (double)out * (double)w[t]).  It walks the EnsTree
//                           arrays, so it serves every model, packed or not.  Results land as lo / hi / interval [column in chunk][doc].
//   k_ale_reduce            one block per column, no atomic, no scatter: count and S of every interval in the order include/rlhip.h
//                           defines.  A tile of 256 documents' d = (double)hi - (double)lo and interval is staged in the LDS; lane k owns
//                           interval k and runs its serial chain over the tile in document order -- every lane reads the same LDS word, a
//                           broadcast -- and counts.  The lanes 0 .. K take W = ceil((K + 1) / 64) wavefronts, so the block's 4 wavefronts
//                           form 4 / W groups that take consecutive tiles at the same time; the groups' partials go through the LDS and
//                           the first group chains them in tile order.
//   Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_ale_host.h"

namespace rl {

constexpr int kAleBatch = RL_ALE_BATCH;
constexpr int kAleSum = RL_PARTIAL_SUM_BLOCK;                // the definition's block of documents
constexpr int kAleWaves = kThreads / 64;
static_assert(kAleBatch >= 1 && kAleBatch <= 32, "uses holds a bit per column of a batch");
static_assert(kAleMaxEdges == RL_ALE_MAX_INTERVALS + 1 && kAleMaxEdges <= kThreads, "lane k of k_ale_reduce owns interval k");
static_assert(kAleSum == 256 && kThreads % 64 == 0, "accumulated local effects geometry");

struct AleArgs {
    EnsTree e; const float *w; int MAXN, nt;
    const float *X; int64_t n; int stride;
    const int32_t *cols;                                       // [n_columns]
    const int32_t *eoff;                                       // [n_columns + 1]
    const float *edges;                                        // [eoff[n_columns]]
    const uint32_t *uses;                                      // [batches of the chunk][nt]
    int32_t c0, c1;                                            // the chunk's columns; c0 == c1: the base launch
    float *lo, *hi; int32_t *iv;                               // [columns of the chunk][n]
    float *base;                                               // [n], the base launch's
};

template <int B>
__global__ __launch_bounds__(kThreads) void k_model_ale_scores(const AleArgs a)
{
    __shared__ float l_edge[B * kAleMaxEdges];
    const int cb = a.c0 + (int)blockIdx.y * B;                 // wave-uniform, like everything read through blockIdx.y
    const int cnt = min(B, a.c1 - cb);
    const uint32_t *uses = a.uses + (size_t)blockIdx.y * a.nt;
    int col[B], ne[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
        col[u] = -1; ne[u] = 0;                                // (a slot past cnt: -1 is no node's column, so it never parts)
        if (u < cnt) {
            col[u] = a.cols[cb + u];
            const int e0 = a.eoff[cb + u];
            ne[u] = a.eoff[cb + u + 1] - e0;
            for (int j = threadIdx.x; j < ne[u]; j += kThreads) l_edge[u * kAleMaxEdges + j] = a.edges[e0 + j];
        }
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = a.X + (size_t)i * a.stride;
        float zl[B], zh[B], sl[B], sh[B];
        int iv[B];
#pragma unroll
        for (int u = 0; u < B; u++) {
            const float v = (col[u] >= 0 && col[u] < a.stride) ? row[col[u]] : 0.f;
            zl[u] = zh[u] = v; iv[u] = 0; sl[u] = sh[u] = 0.f;
            if (u < cnt) {
                const float *z = l_edge + u * kAleMaxEdges;
                const int K = ne[u] - 1;
                if (z[0] <= v && v <= z[K]) {                  // (a NaN is outside)
                    int b = 1, e = K;                          // the first j in [1, K) with !(z[j] < v), K where there is none
                    while (b < e) {
                        const int mid = (b + e) >> 1;
                        if (z[mid] < v) b = mid + 1; else e = mid;
                    }
                    iv[u] = b; zl[u] = z[b - 1]; zh[u] = z[b];
                }
            }
        }
        for (int t = 0; t < a.nt; t++) {
            const size_t o = (size_t)t * a.MAXN;
            const double wt = (double)a.w[t];
            const uint32_t mask = cnt ? uses[t] : 0u;
            int nd = 0, fc;
            if (!mask) {
                while ((fc = a.e.feat_idx[o + nd]) != -1) {
                    const float v = (fc < a.stride) ? row[fc] : 0.f;           // -missingZero  DenseDataPoint.java:22-25
                    nd = (v <= a.e.thr[o + nd]) ? a.e.left[o + nd] : a.e.right[o + nd];
                }
                const double ow = (double)a.e.out[o + nd] * wt;
#pragma unroll
                for (int u = 0; u < B; u++) {
                    sl[u] = (float)((double)sl[u] + ow);                       // Ensemble.java:113
                    sh[u] = (float)((double)sh[u] + ow);
                }
                continue;
            }
            int pl[B], ph[B];                                  // where a side's path leaves the base path (-1: nowhere)
#pragma unroll
            for (int u = 0; u < B; u++) pl[u] = ph[u] = -1;
            while ((fc = a.e.feat_idx[o + nd]) != -1) {
                const float v = (fc < a.stride) ? row[fc] : 0.f;
                const float th = a.e.thr[o + nd];
                const int le = a.e.left[o + nd], ri = a.e.right[o + nd];
                const bool go_left = v <= th;
#pragma unroll
                for (int u = 0; u < B; u++)
                    if (fc == col[u]) {
                        if (pl[u] < 0 && (zl[u] <= th) != go_left) pl[u] = go_left ? ri : le;
                        if (ph[u] < 0 && (zh[u] <= th) != go_left) ph[u] = go_left ? ri : le;
                    }
                nd = go_left ? le : ri;
            }
            const float base_out = a.e.out[o + nd];
#pragma unroll
            for (int u = 0; u < B; u++) {
                float ol = base_out, oh = base_out;
                if (mask & (1u << u)) {
                    if (pl[u] >= 0) {
                        int pn = pl[u], pf;
                        while ((pf = a.e.feat_idx[o + pn]) != -1) {
                            const float v = (pf == col[u]) ? zl[u] : (pf < a.stride) ? row[pf] : 0.f;
                            pn = (v <= a.e.thr[o + pn]) ? a.e.left[o + pn] : a.e.right[o + pn];
                        }
                        ol = a.e.out[o + pn];
                    }
                    if (ph[u] >= 0) {
                        int pn = ph[u], pf;
                        while ((pf = a.e.feat_idx[o + pn]) != -1) {
                            const float v = (pf == col[u]) ? zh[u] : (pf < a.stride) ? row[pf] : 0.f;
                            pn = (v <= a.e.thr[o + pn]) ? a.e.left[o + pn] : a.e.right[o + pn];
                        }
                        oh = a.e.out[o + pn];
                    }
                }
                sl[u] = (float)((double)sl[u] + (double)ol * wt);              // Ensemble.java:113
                sh[u] = (float)((double)sh[u] + (double)oh * wt);
            }
        }
        if (!cnt) { a.base[i] = sl[0]; continue; }
#pragma unroll
        for (int u = 0; u < B; u++)
            if (u < cnt) {
                const size_t at = (size_t)(cb - a.c0 + u) * a.n + i;
                a.lo[at] = sl[u]; a.hi[at] = sh[u]; a.iv[at] = iv[u];
            }
    }
}

// count and S of every interval of the chunk's columns; blockIdx.x is the column in the chunk
__global__ __launch_bounds__(kThreads) void k_ale_reduce(const float *lo, const float *hi, const int32_t *iv, int64_t n, const int32_t *eoff,
                                                         int32_t c0, double *S, long long *N)
{
    __shared__ double l_d[kAleWaves * kAleSum], l_p[kThreads];
    __shared__ int32_t l_iv[kAleWaves * kAleSum], l_c[kThreads];
    const int c = c0 + (int)blockIdx.x;
    const int K = eoff[c + 1] - eoff[c] - 1;
    const int GW = (K + 1 + 63) / 64 * 64;                     // the lanes of a group: whole wavefronts that hold the lanes 0 .. K
    const int G = kThreads / GW;                               // groups: 4, 2, 1 or 1 tiles at a time
    const int g = threadIdx.x / GW, k = threadIdx.x - g * GW;
    const bool owner = g < G && k >= 1 && k <= K;
    const size_t at0 = (size_t)blockIdx.x * n;
    double t = 0.0;                                            // the first group's: the totals so far
    long long cnt = 0;
    for (int64_t d0 = 0; d0 < n; d0 += (int64_t)G * kAleSum) {
        const int m = (int)min((int64_t)G * kAleSum, n - d0);
        for (int j = threadIdx.x; j < m; j += kThreads) {
            l_d[j] = (double)hi[at0 + d0 + j] - (double)lo[at0 + d0 + j];
            l_iv[j] = iv[at0 + d0 + j];
        }
        __syncthreads();
        double p = 0.0;
        int pc = 0;
        if (owner && g * kAleSum < m) {
            const int len = min(kAleSum, m - g * kAleSum);
            const double *d = l_d + g * kAleSum;
            const int32_t *v = l_iv + g * kAleSum;
            for (int j = 0; j < len; j++)
                if (v[j] == k) { p = p + d[j]; pc++; }
        }
        l_p[threadIdx.x] = p;
        l_c[threadIdx.x] = pc;
        __syncthreads();                                       // (the next tile's staging waits for the chains, its partials for the first group)
        if (owner && g == 0) {
            const int np = (m + kAleSum - 1) / kAleSum;
            for (int q = 0; q < np; q++) { t = t + l_p[q * GW + k]; cnt += l_c[q * GW + k]; }
        }
    }
    if (owner && g == 0) {
        const int cell = eoff[c] - c + k - 1;
        S[cell] = t; N[cell] = cnt;
    }
}

static thread_local double g_ale_walk_ms = 0.0, g_ale_reduce_ms = 0.0;  // the last ALE call of this thread, device events

}  // namespace rl

extern "C" {

int rl_model_predict_ale(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                         const int32_t *edge_off, const float *edges, int64_t scratch_bytes, float *out_base, int64_t *out_count,
                         double *out_sum, float *out_lo, float *out_hi, int32_t *out_interval)
{
    const std::string w = "rl_model_predict_ale: ";
    std::string err;
    int rc = ale_check(w, X, n_docs, row_stride, columns, n_columns, edge_off, edges, scratch_bytes, out_count, out_sum, err);
    if (rc) return fail(rc, err);
    if (!m) return fail(RL_ERR_INVALID, w + "null model");             // (after the arguments a machine without a device can check)
    if (m->trees.empty()) return fail(RL_ERR_INVALID, w + "the model has no trees");
    g_ale_walk_ms = g_ale_reduce_ms = 0.0;
    RL_HIP(hipSetDevice(m->device));
    const int32_t n_cells = edge_off[n_columns] - n_columns;
    const int32_t chunk = ale_chunk_columns(scratch_bytes, kStageScratchDefault, n_docs, n_columns, kStageMaxChunk);
    const AlePlan plan = ale_plan(m->trees, columns, n_columns, chunk, kAleBatch);
    AleArgs a;
    memset(&a, 0, sizeof(a));
    a.e = m->ens; a.w = m->d_w; a.MAXN = m->maxn; a.nt = plan.n_trees; a.n = n_docs; a.stride = row_stride;
    DevPool pool;
    float *dX = nullptr, *d_edges = nullptr; int32_t *d_cols = nullptr, *d_eoff = nullptr; uint32_t *d_uses = nullptr;
    double *d_sum = nullptr; long long *d_cnt = nullptr;
    RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
    RL_HIP(pool.upload(&d_cols, columns, (size_t)n_columns));
    RL_HIP(pool.upload(&d_eoff, edge_off, (size_t)n_columns + 1));
    RL_HIP(pool.upload(&d_edges, edges, (size_t)edge_off[n_columns]));
    RL_HIP(pool.upload(&d_uses, plan.uses.data(), plan.uses.size()));
    RL_HIP(pool.alloc(&a.lo, (size_t)chunk * n_docs));
    RL_HIP(pool.alloc(&a.hi, (size_t)chunk * n_docs));
    RL_HIP(pool.alloc(&a.iv, (size_t)chunk * n_docs));
    if (out_base) RL_HIP(pool.alloc(&a.base, (size_t)n_docs));
    RL_HIP(pool.alloc(&d_sum, (size_t)n_cells));
    RL_HIP(pool.alloc(&d_cnt, (size_t)n_cells));
    a.X = dX; a.cols = d_cols; a.eoff = d_eoff; a.edges = d_edges; a.uses = d_uses;
    const unsigned gx = (unsigned)std::min<int64_t>(8192, (n_docs + kThreads - 1) / kThreads);
    StageEvents ev;
    RL_HIP(ev.create());
    for (int32_t ci = 0; ci < plan.chunks(); ci++) {
        const int32_t b0 = plan.first[(size_t)ci], nb = plan.first[(size_t)ci + 1] - b0, c0 = plan.col0(ci), nc = plan.col1(ci) - c0;
        RL_HIP(hipEventRecord(ev.e[0], 0));
        if (ci == 0 && out_base) {                             // the base: an empty batch, one plain walk per tree
            a.c0 = a.c1 = 0; a.uses = d_uses;
            hipLaunchKernelGGL((k_model_ale_scores<kAleBatch>), dim3(gx, 1), dim3(kThreads), 0, 0, a);
            RL_HIP(hipGetLastError());
        }
        a.c0 = c0; a.c1 = c0 + nc; a.uses = d_uses + (size_t)b0 * a.nt;
        hipLaunchKernelGGL((k_model_ale_scores<kAleBatch>), dim3(gx, (unsigned)nb), dim3(kThreads), 0, 0, a);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        hipLaunchKernelGGL(k_ale_reduce, dim3((unsigned)nc), dim3(kThreads), 0, 0, (const float *)a.lo, (const float *)a.hi, (const int32_t *)a.iv,
                           n_docs, (const int32_t *)d_eoff, c0, d_sum, d_cnt);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[2], 0));
        const size_t at = (size_t)c0 * n_docs, cnt = (size_t)nc * n_docs;
        if (out_lo) RL_HIP(hipMemcpy(out_lo + at, a.lo, cnt * sizeof(float), hipMemcpyDeviceToHost));
        if (out_hi) RL_HIP(hipMemcpy(out_hi + at, a.hi, cnt * sizeof(float), hipMemcpyDeviceToHost));
        if (out_interval) RL_HIP(hipMemcpy(out_interval + at, a.iv, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (ci == 0 && out_base) RL_HIP(hipMemcpy(out_base, a.base, (size_t)n_docs * sizeof(float), hipMemcpyDeviceToHost));
        RL_HIP(hipDeviceSynchronize());
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_ale_walk_ms += (double)ms;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
        g_ale_reduce_ms += (double)ms;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "out_count");
    RL_HIP(hipMemcpy(out_sum, d_sum, (size_t)n_cells * sizeof(double), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(out_count, d_cnt, (size_t)n_cells * sizeof(int64_t), hipMemcpyDeviceToHost));
    m->last_path = RL_MODEL_PATH_ALE;
    return RL_OK;
}

int rl_debug_ale_times(double *walk_ms, double *reduce_ms)
{
    if (!walk_ms || !reduce_ms) return fail(RL_ERR_INVALID, "rl_debug_ale_times: null argument");
    *walk_ms = g_ale_walk_ms;
    *reduce_ms = g_ale_reduce_ms;
    return RL_OK;
}

}  // extern "C"
