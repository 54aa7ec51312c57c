// rl_partial.inc -- partial dependence and ICE curves of a tree model in one pass over a file: every (column, grid value) cell's scores,
// their mean and their mean squared move away from the base, without a substituted copy of the rows.  DESIGN.md 29.
// Included at the end of rl_trainer.hip, after rl_permimp.inc (it uses DevPool, StageEvents and stage_chunk).  The integer bookkeeping
// of a call -- checks, chunks, batches, uses -- is rl_partial_host.h's.
//
//   k_model_partial_scores<B>   one lane per document, blockIdx.y over the chunk's batches.  A batch is up to B consecutive cells of ONE
//                               column (the host pads the last batch of a column by repeating its last value), so the column, the B
//                               substitute values and the batch's place in the scores are wave-uniform: scalar loads, no gather.  Per
//                               tree:
//                                 * uses[batch][tree] == 0 (exact: no node of the tree tests the column): one walk, its output joins all
//                                   B chains;
//                                 * otherwise the base walk is made once.  At a node on it that tests the column every cell's value is
//                                   compared with the threshold too; a cell that goes the other way walks on from the other child with
//                                   its value standing in at every later node that tests the column.  Cells that never part take the
//                                   base output.
//                               A column at or beyond the row stride needs no special case: the base walk reads 0 there, the cell its
//                               value.  The base is one more batch (column -1, which no node tests) whose one cell goes to its own
//                               buffer.  Each chain is Ensemble.eval's statement s = (float)((double)s + (double)out * (double)w[t]).  It
//                               walks the EnsTree arrays, so it serves every model, packed or not.  Scores land as sc[cell in chunk][doc].
//   k_partial_reduce            one block per cell: S1 and S2 in the order include/rlhip.h defines -- partial p the serial chain over the
//                               documents [256 p, 256 p + 256), the total the serial chain over the partials.  A tile of 16 partials is
//                               staged in the LDS with coalesced loads, 16 lanes run one partial each, lane 0 adds them in order.
//   No cross-block atomic, no spin wait.  Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_partial_host.h"

namespace rl {

constexpr int kPdBatch = RL_PARTIAL_BATCH;
constexpr int kPdSum = RL_PARTIAL_SUM_BLOCK;                 // the definition's block of documents, not a launch width
constexpr int kPdTile = 16;                                  // partials k_partial_reduce stages at a time
static_assert(kPdBatch >= 1 && kPdSum >= 1 && kPdTile <= kThreads, "partial dependence geometry");

struct PartArgs {
    EnsTree e; const float *w; int MAXN, nt;
    const float *X; int64_t n; int stride;
    const PartialBatch *batch;                                 // [batches of the chunk]
    const float *val;                                          // [batches of the chunk][B]
    const uint8_t *uses;                                       // [batches of the chunk][nt]
    float *sc;                                                 // [cells of the chunk][n]
    float *base;                                               // [n]
};

template <int B>
__global__ __launch_bounds__(kThreads) void k_model_partial_scores(const PartArgs a)
{
    const PartialBatch bd = a.batch[blockIdx.y];               // wave-uniform, like everything read through blockIdx.y
    const int col = bd.col;
    const uint8_t *uses = a.uses + (size_t)blockIdx.y * a.nt;
    float gv[B];
#pragma unroll
    for (int u = 0; u < B; u++) gv[u] = a.val[(size_t)blockIdx.y * B + u];
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = a.X + (size_t)i * a.stride;
        float s[B];
#pragma unroll
        for (int u = 0; u < B; u++) s[u] = 0.f;
        for (int t = 0; t < a.nt; t++) {
            const size_t o = (size_t)t * a.MAXN;
            const double wt = (double)a.w[t];
            int nd = 0;
            if (!uses[t]) {
                int fc;
                while ((fc = a.e.feat_idx[o + nd]) != -1) {
                    const float v = (fc < a.stride) ? row[fc] : 0.f;           // -missingZero  DenseDataPoint.java:22-25
                    nd = (v <= a.e.thr[o + nd]) ? a.e.left[o + nd] : a.e.right[o + nd];
                }
                const double ow = (double)a.e.out[o + nd] * wt;
#pragma unroll
                for (int u = 0; u < B; u++) s[u] = (float)((double)s[u] + ow);  // Ensemble.java:113
                continue;
            }
            int part[B];                                       // where the cell's path leaves the base path (-1: nowhere)
#pragma unroll
            for (int u = 0; u < B; u++) part[u] = -1;
            int fc;
            while ((fc = a.e.feat_idx[o + nd]) != -1) {
                const float v = (fc < a.stride) ? row[fc] : 0.f;
                const float th = a.e.thr[o + nd];
                const int le = a.e.left[o + nd], ri = a.e.right[o + nd];
                const bool go_left = v <= th;
                if (fc == col) {
#pragma unroll
                    for (int u = 0; u < B; u++)
                        if (part[u] < 0 && (gv[u] <= th) != go_left) part[u] = go_left ? ri : le;
                }
                nd = go_left ? le : ri;
            }
            const float base_out = a.e.out[o + nd];
#pragma unroll
            for (int u = 0; u < B; u++) {
                float out = base_out;
                if (part[u] >= 0) {
                    int pn = part[u], pf;
                    while ((pf = a.e.feat_idx[o + pn]) != -1) {
                        const float v = (pf == col) ? gv[u] : (pf < a.stride) ? row[pf] : 0.f;
                        pn = (v <= a.e.thr[o + pn]) ? a.e.left[o + pn] : a.e.right[o + pn];
                    }
                    out = a.e.out[o + pn];
                }
                s[u] = (float)((double)s[u] + (double)out * wt);               // Ensemble.java:113
            }
        }
        if (col < 0) { a.base[i] = s[0]; continue; }
#pragma unroll
        for (int u = 0; u < B; u++)
            if (u < bd.cnt) a.sc[(size_t)(bd.cell0 + u) * a.n + i] = s[u];
    }
}

// S1[cell] and S2[cell] of the chunk's cells; blockIdx.x is the cell in the chunk
__global__ __launch_bounds__(kThreads) void k_partial_reduce(const float *sc, const float *base, int64_t n, double *S1, double *S2)
{
    constexpr int W = kPdSum + 1;                            // (the + 1 keeps the 16 lanes' reads off one bank)
    __shared__ float l_ice[kPdTile * W], l_base[kPdTile * W];
    __shared__ double l_p1[kPdTile], l_p2[kPdTile];
    const float *ice = sc + (size_t)blockIdx.x * n;
    double t1 = 0.0, t2 = 0.0;                                 // lane 0's: the totals so far
    for (int64_t d0 = 0; d0 < n; d0 += (int64_t)kPdTile * kPdSum) {
        const int m = (int)min((int64_t)kPdTile * kPdSum, n - d0);
        for (int k = threadIdx.x; k < m; k += kThreads) {
            const int at = (k / kPdSum) * W + k % kPdSum;
            l_ice[at] = ice[d0 + k];
            l_base[at] = base[d0 + k];
        }
        __syncthreads();
        const int np = (m + kPdSum - 1) / kPdSum;
        if ((int)threadIdx.x < np) {
            const int len = min(kPdSum, m - (int)threadIdx.x * kPdSum);
            double p1 = 0.0, p2 = 0.0;
            for (int k = 0; k < len; k++) {
                const double x = (double)l_ice[threadIdx.x * W + k];
                const double d = x - (double)l_base[threadIdx.x * W + k];
                p1 = p1 + x;
                p2 = p2 + d * d;
            }
            l_p1[threadIdx.x] = p1;
            l_p2[threadIdx.x] = p2;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int p = 0; p < np; p++) { t1 = t1 + l_p1[p]; t2 = t2 + l_p2[p]; }
        __syncthreads();                                       // (the next tile's partials wait for lane 0)
    }
    if (threadIdx.x == 0) { S1[blockIdx.x] = t1; S2[blockIdx.x] = t2; }
}

static thread_local double g_pd_walk_ms = 0.0, g_pd_reduce_ms = 0.0;    // the last partial call of this thread, device events

}  // namespace rl

extern "C" {

int rl_model_predict_partial(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                             const int32_t *grid_off, const float *grid, int64_t scratch_bytes, float *out_base, double *out_mean,
                             double *out_shift2, float *out_ice)
{
    const std::string w = "rl_model_predict_partial: ";
    std::string err;
    int rc = partial_check(w, X, n_docs, row_stride, columns, n_columns, grid_off, grid, scratch_bytes, out_mean, out_shift2, err);
    if (rc) return fail(rc, err);
    if (!m) return fail(RL_ERR_INVALID, w + "null model");             // (after the arguments a machine without a device can check)
    if (m->trees.empty()) return fail(RL_ERR_INVALID, w + "the model has no trees");
    g_pd_walk_ms = g_pd_reduce_ms = 0.0;
    RL_HIP(hipSetDevice(m->device));
    const int32_t n_cells = grid_off[n_columns];
    const int chunk = std::min(kStageMaxChunk - 1,              // (gridDim.y: every cell may be a batch of its own, and the base is one more)
                               stage_chunk(partial_cell_budget(scratch_bytes, kStageScratchDefault, n_docs), n_docs * (int64_t)sizeof(float), n_cells));
    const PartialPlan plan = partial_plan(m->trees, columns, n_columns, grid_off, grid, chunk, kPdBatch);
    PartArgs a;
    memset(&a, 0, sizeof(a));
    a.e = m->ens; a.w = m->d_w; a.MAXN = m->maxn; a.nt = plan.n_trees; a.n = n_docs; a.stride = row_stride;
    DevPool pool;
    float *dX = nullptr, *d_val = nullptr; PartialBatch *d_batch = nullptr; uint8_t *d_uses = nullptr; double *d_s1 = nullptr, *d_s2 = nullptr;
    RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
    RL_HIP(pool.upload(&d_batch, plan.batches.data(), plan.batches.size()));
    RL_HIP(pool.upload(&d_val, plan.values.data(), plan.values.size()));
    RL_HIP(pool.upload(&d_uses, plan.uses.data(), plan.uses.size()));
    RL_HIP(pool.alloc(&a.sc, (size_t)chunk * n_docs));
    RL_HIP(pool.alloc(&a.base, (size_t)n_docs));
    RL_HIP(pool.alloc(&d_s1, (size_t)chunk));
    RL_HIP(pool.alloc(&d_s2, (size_t)chunk));
    a.X = dX;
    std::vector<double> s1((size_t)chunk), s2((size_t)chunk);
    StageEvents ev;
    RL_HIP(ev.create());
    for (int32_t ci = 0; ci < plan.chunks(); ci++) {
        const int32_t b0 = plan.first[(size_t)ci], nb = plan.first[(size_t)ci + 1] - b0, nc = plan.cells_of(ci), c0 = plan.cell0[(size_t)ci];
        a.batch = d_batch + b0; a.val = d_val + (size_t)b0 * kPdBatch; a.uses = d_uses + (size_t)b0 * a.nt;
        RL_HIP(hipEventRecord(ev.e[0], 0));
        const dim3 grid_w((unsigned)std::min<int64_t>(8192, (n_docs + kThreads - 1) / kThreads), (unsigned)nb);
        hipLaunchKernelGGL((k_model_partial_scores<kPdBatch>), grid_w, dim3(kThreads), 0, 0, a);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        hipLaunchKernelGGL(k_partial_reduce, dim3((unsigned)nc), dim3(kThreads), 0, 0, (const float *)a.sc, (const float *)a.base, n_docs, d_s1, d_s2);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[2], 0));
        RL_HIP(hipMemcpy(s1.data(), d_s1, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost));
        RL_HIP(hipMemcpy(s2.data(), d_s2, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost));
        if (out_ice) RL_HIP(hipMemcpy(out_ice + (size_t)c0 * n_docs, a.sc, (size_t)nc * n_docs * sizeof(float), hipMemcpyDeviceToHost));
        if (ci == 0 && out_base) RL_HIP(hipMemcpy(out_base, a.base, (size_t)n_docs * sizeof(float), hipMemcpyDeviceToHost));
        RL_HIP(hipDeviceSynchronize());
        for (int32_t j = 0; j < nc; j++) {
            out_mean[c0 + j] = s1[(size_t)j] / (double)n_docs;
            out_shift2[c0 + j] = s2[(size_t)j] / (double)n_docs;
        }
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_pd_walk_ms += (double)ms;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
        g_pd_reduce_ms += (double)ms;
    }
    m->last_path = RL_MODEL_PATH_PARTIAL;
    return RL_OK;
}

int rl_debug_partial_times(double *walk_ms, double *reduce_ms)
{
    if (!walk_ms || !reduce_ms) return fail(RL_ERR_INVALID, "rl_debug_partial_times: null argument");
    *walk_ms = g_pd_walk_ms;
    *reduce_ms = g_pd_reduce_ms;
    return RL_OK;
}

}  // extern "C"
