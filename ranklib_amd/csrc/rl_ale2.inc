// rl_ale2.inc -- second-order accumulated local effects (Apley and Zhu's two-feature ALE) of a tree model in one pass over a file: per
// pair of columns every document is scored at the four corners of the cell its own two values lie in, and the second differences are
// counted and summed per cell in one fixed order, without the four substituted copies of the rows per pair.  DESIGN.md 40.
// Included at the end of rl_trainer.hip, after rl_ale.inc (it uses DevPool, StageEvents and kStageScratchDefault).  The integer
// bookkeeping of a call -- checks, chunks, batches, uses -- is rl_ale2_host.h's.
//
//   k_model_ale2_scores<P>  one lane per document, blockIdx.y over the chunk's batches.  A batch is up to P consecutive PAIRS; their
//                           columns and edge counts are wave-uniform scalars, both edge slices of every pair are staged in the LDS once
//                           per block.  Per document and pair the lane makes two binary searches there and keeps the four substitutes
//                           za_lo, za_hi, zb_lo, zb_hi and four float chains in registers: 4 P chains per lane.  A document outside
//                           either axis takes its own values for all four substitutes, so it can never part and scores its base four
//                           times.  Per tree:
//                             * uses[batch][tree] == 0 (exact: no node of the tree tests a column of the batch): one walk, its output
//                               joins all 4 P chains;
//                             * otherwise the base walk is made once on the document's own row.  The own value lies between its two
//                               substitutes, so at a node on that path that tests a (or b) at most one of the two sides can go the other
//                               way: the two corners of that side that are still on the path part there.  Corner (ua, ub) keeps the
//                               node it parted to in part[2 ua + ub].  After the base walk the two corners of one side that parted at
//                               the same node walk on TOGETHER from it, both substitutes standing in at every later node that tests
//                               either column, until a node separates them; from there, and where a corner parted alone, a single walk
//                               finishes.  Corners that never part take the base output; the bits of uses say which pairs can have
//                               parted at all.
//                           Each chain is Ensemble.eval's statement s = (float)((double)s + (double)out * (double)w[t]).  It walks the
//                           EnsTree arrays, so it serves every model, packed or not.  Results land as d (f64, the second difference)
//                           and cell (int32, (k - 1) Kb + l - 1, or -1) [pair in chunk][doc], the four corners [pair in chunk][4][doc]
//                           only when asked.  The base, where asked for, is one launch more with an empty batch.
//   k_ale2_reduce           grid (super-block, pair in chunk), no atomic, no scatter.  "Lane k owns interval k" of k_ale_reduce does not
//                           stretch to 4096 cells: here lane j owns the cells c with (c & 255) == j and the accumulators live in the LDS
//                           -- a partial f64 and an int32 count per cell, 48 KB at the cap -- while the running sums, which are only
//                           ever indexed by the fold's unrolled loop, stay in 16 registers a lane.  A tile of 256 documents' (d, cell)
//                           is staged; the block steps through it in document order, every lane reading the same LDS word (a
//                           broadcast), and only the owner adds d to its cell's partial.  A cell has one owner for the whole block, so
//                           its order is the document order.  After a tile every lane folds its cells' partials into its running sums
//                           and zeroes them; after the super-block's 64 tiles it writes them and the counts as [super-block][cell].
//   k_ale2_finish           one lane per cell: the serial chain over the super-partials in order, the counts added up.
//   Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_ale2_host.h"

namespace rl {

constexpr int kAle2Batch = RL_ALE2_BATCH;
constexpr int kAle2Own = RL_ALE2_MAX_CELLS / kThreads;       // the cells a lane of k_ale2_reduce owns at the most
static_assert(kAle2Batch >= 1 && kAle2Batch <= 16, "uses holds two bits per pair of a batch");
static_assert(kAle2MaxCells == RL_ALE2_MAX_CELLS && kAle2Super == RL_ALE2_SUM_SUPER, "rl_ale2_host.h restates include/rlhip.h");
static_assert(kAleSum == kThreads && kAle2Own * kThreads == RL_ALE2_MAX_CELLS, "a tile is one document a lane; lane j owns the cells j + 256 s");

struct Ale2Args {
    EnsTree e; const float *w; int MAXN, nt;
    const float *X; int64_t n; int stride;
    const int32_t *pairs;                                      // [n_pairs][2]
    const int32_t *eoff;                                       // [2 n_pairs + 1]
    const float *edges;                                        // [eoff[2 n_pairs]]
    const uint32_t *uses;                                      // [batches of the chunk][nt]
    int32_t p0, p1;                                            // the chunk's pairs; p0 == p1: the base launch
    double *d; int32_t *cell;                                  // [pairs of the chunk][n]
    float *corner;                                             // [pairs of the chunk][4][n], or null
    float *base;                                               // [n], the base launch's
};

// the interval of v under the K + 1 staged edges z: 1 + #{j in 1 .. K-1 : z_j < v} where z_0 <= v <= z_K, else 0 (a NaN is outside)
__device__ __forceinline__ int ale2_interval(const float *z, int K, float v)
{
    if (!(z[0] <= v && v <= z[K])) return 0;
    int b = 1, e = K;                                          // the first j in [1, K) with !(z[j] < v), K where there is none
    while (b < e) {
        const int mid = (b + e) >> 1;
        if (z[mid] < v) b = mid + 1; else e = mid;
    }
    return b;
}

// the output of the leaf a walk from node nd reaches with va standing in for column ca and vb for column cb
__device__ __forceinline__ float ale2_walk_on(const Ale2Args &a, size_t o, const float *row, int nd, int ca, int cb, float va, float vb)
{
    int f;
    while ((f = a.e.feat_idx[o + nd]) != -1) {
        const float v = (f == ca) ? va : (f == cb) ? vb : (f < a.stride) ? row[f] : 0.f;
        nd = (v <= a.e.thr[o + nd]) ? a.e.left[o + nd] : a.e.right[o + nd];
    }
    return a.e.out[o + nd];
}

// two corners that parted at the same node nd: one walk while their substitutes agree, two from the node that separates them
__device__ __forceinline__ void ale2_walk_two(const Ale2Args &a, size_t o, const float *row, int nd, int ca, int cb, float va0, float vb0,
                                              float va1, float vb1, float &o0, float &o1)
{
    int f;
    while ((f = a.e.feat_idx[o + nd]) != -1) {
        const float th = a.e.thr[o + nd];
        const int le = a.e.left[o + nd], ri = a.e.right[o + nd];
        const float own = (f < a.stride) ? row[f] : 0.f;
        const bool l0 = ((f == ca) ? va0 : (f == cb) ? vb0 : own) <= th, l1 = ((f == ca) ? va1 : (f == cb) ? vb1 : own) <= th;
        if (l0 != l1) {
            o0 = ale2_walk_on(a, o, row, l0 ? le : ri, ca, cb, va0, vb0);
            o1 = ale2_walk_on(a, o, row, l1 ? le : ri, ca, cb, va1, vb1);
            return;
        }
        nd = l0 ? le : ri;
    }
    o0 = o1 = a.e.out[o + nd];
}

template <int P>
__global__ __launch_bounds__(kThreads) void k_model_ale2_scores(const Ale2Args a)
{
    __shared__ float l_edge[P * 2 * kAleMaxEdges];
    const int pb = a.p0 + (int)blockIdx.y * P;                 // wave-uniform, like everything read through blockIdx.y
    const int cnt = min(P, a.p1 - pb);
    const uint32_t *uses = a.uses + (size_t)blockIdx.y * a.nt;
    int ca[P], cb[P], Ka[P], Kb[P];
#pragma unroll
    for (int u = 0; u < P; u++) {
        ca[u] = cb[u] = -1; Ka[u] = Kb[u] = 0;                 // (a slot past cnt: -1 is no node's column, so it never parts)
        if (u < cnt) {
            ca[u] = a.pairs[2 * (pb + u)]; cb[u] = a.pairs[2 * (pb + u) + 1];
            const int e0 = a.eoff[2 * (pb + u)], e1 = a.eoff[2 * (pb + u) + 1], e2 = a.eoff[2 * (pb + u) + 2];
            Ka[u] = e1 - e0 - 1; Kb[u] = e2 - e1 - 1;
            for (int j = threadIdx.x; j < e1 - e0; j += kThreads) l_edge[(2 * u) * kAleMaxEdges + j] = a.edges[e0 + j];
            for (int j = threadIdx.x; j < e2 - e1; j += kThreads) l_edge[(2 * u + 1) * kAleMaxEdges + j] = a.edges[e1 + j];
        }
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = a.X + (size_t)i * a.stride;
        float za[P][2], zb[P][2], s[P][4];
        int cell[P];
#pragma unroll
        for (int u = 0; u < P; u++) {
            const float va = (ca[u] >= 0 && ca[u] < a.stride) ? row[ca[u]] : 0.f, vb = (cb[u] >= 0 && cb[u] < a.stride) ? row[cb[u]] : 0.f;
            za[u][0] = za[u][1] = va; zb[u][0] = zb[u][1] = vb; cell[u] = -1;
            s[u][0] = s[u][1] = s[u][2] = s[u][3] = 0.f;
            if (u < cnt) {
                const float *ea = l_edge + (2 * u) * kAleMaxEdges, *eb = ea + kAleMaxEdges;
                const int k = ale2_interval(ea, Ka[u], va), l = ale2_interval(eb, Kb[u], vb);
                if (k > 0 && l > 0) {
                    cell[u] = (k - 1) * Kb[u] + (l - 1);
                    za[u][0] = ea[k - 1]; za[u][1] = ea[k]; zb[u][0] = eb[l - 1]; zb[u][1] = eb[l];
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
                for (int u = 0; u < P; u++)
#pragma unroll
                    for (int c = 0; c < 4; c++) s[u][c] = (float)((double)s[u][c] + ow);      // Ensemble.java:113
                continue;
            }
            int part[P][4];                                    // where a corner's path leaves the base path (-1: nowhere)
#pragma unroll
            for (int u = 0; u < P; u++) part[u][0] = part[u][1] = part[u][2] = part[u][3] = -1;
            while ((fc = a.e.feat_idx[o + nd]) != -1) {
                const float v = (fc < a.stride) ? row[fc] : 0.f;
                const float th = a.e.thr[o + nd];
                const int le = a.e.left[o + nd], ri = a.e.right[o + nd];
                const bool go_left = v <= th;
                const int other = go_left ? ri : le;
#pragma unroll
                for (int u = 0; u < P; u++) {
                    if (fc == ca[u]) {
#pragma unroll
                        for (int ua = 0; ua < 2; ua++)
                            if ((za[u][ua] <= th) != go_left) {
                                if (part[u][2 * ua] < 0) part[u][2 * ua] = other;
                                if (part[u][2 * ua + 1] < 0) part[u][2 * ua + 1] = other;
                            }
                    } else if (fc == cb[u]) {
#pragma unroll
                        for (int ub = 0; ub < 2; ub++)
                            if ((zb[u][ub] <= th) != go_left) {
                                if (part[u][ub] < 0) part[u][ub] = other;
                                if (part[u][2 + ub] < 0) part[u][2 + ub] = other;
                            }
                    }
                }
                nd = go_left ? le : ri;
            }
            const float base_out = a.e.out[o + nd];
#pragma unroll
            for (int u = 0; u < P; u++) {
                float oc[4] = {base_out, base_out, base_out, base_out};
                if ((mask >> (2 * u)) & 3u) {
                    bool done[4];
#pragma unroll
                    for (int c = 0; c < 4; c++) done[c] = part[u][c] < 0;
                    // the sides that can have parted together: (0, 1) and (2, 3) at a node on a, (0, 2) and (1, 3) at a node on b
                    const int side[4][2] = {{0, 1}, {2, 3}, {0, 2}, {1, 3}};
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int c0 = side[q][0], c1 = side[q][1];
                        if (!done[c0] && !done[c1] && part[u][c0] == part[u][c1]) {
                            ale2_walk_two(a, o, row, part[u][c0], ca[u], cb[u], za[u][c0 >> 1], zb[u][c0 & 1], za[u][c1 >> 1], zb[u][c1 & 1], oc[c0], oc[c1]);
                            done[c0] = done[c1] = true;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if (!done[c]) oc[c] = ale2_walk_on(a, o, row, part[u][c], ca[u], cb[u], za[u][c >> 1], zb[u][c & 1]);
                }
#pragma unroll
                for (int c = 0; c < 4; c++) s[u][c] = (float)((double)s[u][c] + (double)oc[c] * wt);      // Ensemble.java:113
            }
        }
        if (!cnt) { a.base[i] = s[0][0]; continue; }
#pragma unroll
        for (int u = 0; u < P; u++)
            if (u < cnt) {
                const size_t pc = (size_t)(pb - a.p0 + u);
                a.d[pc * a.n + i] = ((double)s[u][3] - (double)s[u][1]) - ((double)s[u][2] - (double)s[u][0]);
                a.cell[pc * a.n + i] = cell[u];
                if (a.corner) {
#pragma unroll
                    for (int c = 0; c < 4; c++) a.corner[(pc * 4 + c) * a.n + i] = s[u][c];
                }
            }
    }
}

// the super-partials and counts of every cell of the chunk's pairs: blockIdx.x is the super-block, blockIdx.y the pair in the chunk;
// sup_S / sup_N hold per pair [supers][cells of the pair], the pairs laid end to end
__global__ __launch_bounds__(kThreads) void k_ale2_reduce(const double *d, const int32_t *cell, int64_t n, int32_t p0, const int32_t *cell_off,
                                                          double *sup_S, int32_t *sup_N)
{
    __shared__ double l_part[RL_ALE2_MAX_CELLS], l_d[kAleSum];
    __shared__ int32_t l_cnt[RL_ALE2_MAX_CELLS], l_c[kAleSum];
    const int p = p0 + (int)blockIdx.y, lane = (int)threadIdx.x;
    const int cells = cell_off[p + 1] - cell_off[p];
    const int supers = (int)gridDim.x;
    const size_t at0 = (size_t)blockIdx.y * n;
    const int64_t s0 = (int64_t)blockIdx.x * kAle2Super * kAleSum, s1 = min(n, s0 + (int64_t)kAle2Super * kAleSum);
    double run[kAle2Own];
#pragma unroll
    for (int s = 0; s < kAle2Own; s++) run[s] = 0.0;
    for (int c = lane; c < cells; c += kThreads) { l_part[c] = 0.0; l_cnt[c] = 0; }      // (the owner's own cells: no barrier needed)
    for (int64_t d0 = s0; d0 < s1; d0 += kAleSum) {
        const int m = (int)min((int64_t)kAleSum, s1 - d0);
        __syncthreads();                                       // (the last tile's steps are over)
        if (lane < m) { l_d[lane] = d[at0 + d0 + lane]; l_c[lane] = cell[at0 + d0 + lane]; }
        __syncthreads();
        for (int j = 0; j < m; j++) {
            const int c = l_c[j];                              // the same word for every lane: a broadcast
            if (c >= 0 && c < cells && (c & (kThreads - 1)) == lane) { l_part[c] = l_part[c] + l_d[j]; l_cnt[c]++; }
        }
#pragma unroll
        for (int s = 0; s < kAle2Own; s++) {
            const int c = lane + s * kThreads;
            if (c < cells) { run[s] = run[s] + l_part[c]; l_part[c] = 0.0; }
        }
    }
    const size_t out0 = (size_t)(cell_off[p] - cell_off[p0]) * supers + (size_t)blockIdx.x * cells;
#pragma unroll
    for (int s = 0; s < kAle2Own; s++) {
        const int c = lane + s * kThreads;
        if (c < cells) { sup_S[out0 + c] = run[s]; sup_N[out0 + c] = l_cnt[c]; }
    }
}

// blockIdx.y is the pair in the chunk, a lane a cell of it: the chain over the super-partials in order
__global__ __launch_bounds__(kThreads) void k_ale2_finish(const double *sup_S, const int32_t *sup_N, int32_t supers, int32_t p0,
                                                          const int32_t *cell_off, double *S, long long *N)
{
    const int p = p0 + (int)blockIdx.y;
    const int cells = cell_off[p + 1] - cell_off[p];
    const int c = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (c >= cells) return;
    const size_t in0 = (size_t)(cell_off[p] - cell_off[p0]) * supers + c;
    double t = 0.0;
    long long cnt = 0;
    for (int q = 0; q < supers; q++) { t = t + sup_S[in0 + (size_t)q * cells]; cnt += sup_N[in0 + (size_t)q * cells]; }
    S[cell_off[p] + c] = t; N[cell_off[p] + c] = cnt;
}

static thread_local double g_ale2_walk_ms = 0.0, g_ale2_reduce_ms = 0.0;  // the last ALE2 call of this thread, device events

}  // namespace rl

extern "C" {

int rl_model_predict_ale2(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *pairs, int32_t n_pairs,
                          const int32_t *edge_off, const float *edges, int64_t scratch_bytes, float *out_base, int64_t *out_count,
                          double *out_sum, float *out_corner, int32_t *out_cell)
{
    const std::string w = "rl_model_predict_ale2: ";
    std::string err;
    int rc = ale2_check(w, X, n_docs, row_stride, pairs, n_pairs, edge_off, edges, scratch_bytes, out_count, out_sum, err);
    if (rc) return fail(rc, err);
    if (!m) return fail(RL_ERR_INVALID, w + "null model");             // (after the arguments a machine without a device can check)
    if (m->trees.empty()) return fail(RL_ERR_INVALID, w + "the model has no trees");
    g_ale2_walk_ms = g_ale2_reduce_ms = 0.0;
    RL_HIP(hipSetDevice(m->device));
    const int32_t chunk = ale2_chunk_pairs(scratch_bytes, kStageScratchDefault, n_docs, n_pairs, out_corner != nullptr, kStageMaxChunk);
    const Ale2Plan plan = ale2_plan(m->trees, pairs, n_pairs, edge_off, chunk, kAle2Batch);
    const int32_t n_cells = plan.cell_off.back(), supers = ale2_supers(n_docs, kAleSum);
    Ale2Args a;
    memset(&a, 0, sizeof(a));
    a.e = m->ens; a.w = m->d_w; a.MAXN = m->maxn; a.nt = plan.n_trees; a.n = n_docs; a.stride = row_stride;
    DevPool pool;
    float *dX = nullptr, *d_edges = nullptr; int32_t *d_pairs = nullptr, *d_eoff = nullptr, *d_coff = nullptr, *d_supn = nullptr;
    uint32_t *d_uses = nullptr; double *d_sum = nullptr, *d_sups = nullptr; long long *d_cnt = nullptr;
    RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
    RL_HIP(pool.upload(&d_pairs, pairs, (size_t)2 * n_pairs));
    RL_HIP(pool.upload(&d_eoff, edge_off, (size_t)2 * n_pairs + 1));
    RL_HIP(pool.upload(&d_edges, edges, (size_t)edge_off[2 * n_pairs]));
    RL_HIP(pool.upload(&d_coff, plan.cell_off.data(), plan.cell_off.size()));
    RL_HIP(pool.upload(&d_uses, plan.uses.data(), plan.uses.size()));
    RL_HIP(pool.alloc(&a.d, (size_t)chunk * n_docs));
    RL_HIP(pool.alloc(&a.cell, (size_t)chunk * n_docs));
    if (out_corner) RL_HIP(pool.alloc(&a.corner, (size_t)chunk * 4 * n_docs));
    if (out_base) RL_HIP(pool.alloc(&a.base, (size_t)n_docs));
    RL_HIP(pool.alloc(&d_sups, (size_t)plan.max_cells * supers));
    RL_HIP(pool.alloc(&d_supn, (size_t)plan.max_cells * supers));
    RL_HIP(pool.alloc(&d_sum, (size_t)n_cells));
    RL_HIP(pool.alloc(&d_cnt, (size_t)n_cells));
    a.X = dX; a.pairs = d_pairs; a.eoff = d_eoff; a.edges = d_edges; a.uses = d_uses;
    const unsigned gx = (unsigned)std::min<int64_t>(8192, (n_docs + kThreads - 1) / kThreads);
    StageEvents ev;
    RL_HIP(ev.create());
    for (int32_t ci = 0; ci < plan.chunks(); ci++) {
        const int32_t b0 = plan.first[(size_t)ci], nb = plan.first[(size_t)ci + 1] - b0, p0 = plan.pair0(ci), np = plan.pair1(ci) - p0;
        RL_HIP(hipEventRecord(ev.e[0], 0));
        if (ci == 0 && out_base) {                             // the base: an empty batch, one plain walk per tree
            a.p0 = a.p1 = 0; a.uses = d_uses;
            hipLaunchKernelGGL((k_model_ale2_scores<kAle2Batch>), dim3(gx, 1), dim3(kThreads), 0, 0, a);
            RL_HIP(hipGetLastError());
        }
        a.p0 = p0; a.p1 = p0 + np; a.uses = d_uses + (size_t)b0 * a.nt;
        hipLaunchKernelGGL((k_model_ale2_scores<kAle2Batch>), dim3(gx, (unsigned)nb), dim3(kThreads), 0, 0, a);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        hipLaunchKernelGGL(k_ale2_reduce, dim3((unsigned)supers, (unsigned)np), dim3(kThreads), 0, 0, (const double *)a.d, (const int32_t *)a.cell,
                           n_docs, p0, (const int32_t *)d_coff, d_sups, d_supn);
        RL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ale2_finish, dim3((unsigned)(kAle2MaxCells / kThreads), (unsigned)np), dim3(kThreads), 0, 0, (const double *)d_sups,
                           (const int32_t *)d_supn, supers, p0, (const int32_t *)d_coff, d_sum, d_cnt);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[2], 0));
        const size_t at = (size_t)p0 * n_docs, cnt = (size_t)np * n_docs;
        if (out_corner) RL_HIP(hipMemcpy(out_corner + 4 * at, a.corner, 4 * cnt * sizeof(float), hipMemcpyDeviceToHost));
        if (out_cell) RL_HIP(hipMemcpy(out_cell + at, a.cell, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (ci == 0 && out_base) RL_HIP(hipMemcpy(out_base, a.base, (size_t)n_docs * sizeof(float), hipMemcpyDeviceToHost));
        RL_HIP(hipDeviceSynchronize());
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_ale2_walk_ms += (double)ms;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
        g_ale2_reduce_ms += (double)ms;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "out_count");
    RL_HIP(hipMemcpy(out_sum, d_sum, (size_t)n_cells * sizeof(double), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(out_count, d_cnt, (size_t)n_cells * sizeof(int64_t), hipMemcpyDeviceToHost));
    m->last_path = RL_MODEL_PATH_ALE2;
    return RL_OK;
}

int rl_debug_ale2_times(double *walk_ms, double *reduce_ms)
{
    if (!walk_ms || !reduce_ms) return fail(RL_ERR_INVALID, "rl_debug_ale2_times: null argument");
    *walk_ms = g_ale2_walk_ms;
    *reduce_ms = g_ale2_reduce_ms;
    return RL_OK;
}

}  // extern "C"
