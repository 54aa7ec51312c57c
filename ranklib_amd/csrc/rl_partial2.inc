// rl_partial2.inc -- two-feature partial dependence of a tree model in one pass over a file: for every pair of columns (a, b) the score
// surface over both grids at once -- every (pair, value of a, value of b) cell's scores, their mean and their mean squared move away
// from the base -- without a substituted copy of the rows.  DESIGN.md 35.
// Included at the end of rl_trainer.hip, after rl_partial.inc (it uses DevPool, StageEvents, stage_chunk and k_partial_reduce).  The
// integer bookkeeping of a call -- checks, tiles, chunks, uses -- is rl_partial2_host.h's.
//
//   k_model_partial2_scores<TA, TB>   one lane per document, blockIdx.y over the chunk's tiles.  A tile is up to TA x TB cells of ONE pair:
//                               TA consecutive values of a, TB of b (the host pads an edge tile by repeating the last value; padded cells
//                               are never stored), so the two columns and the TA + TB values are wave-uniform.  The tile's TA * TB
//                               float chains live in the LDS as [cell][lane] -- lane fastest, so no bank conflict -- for the whole tree
//                               loop.  Per tree:
//                                 * uses[tile][tree] == 0 (exact: no node of the tree tests a or b): one walk, its output joins all chains;
//                                 * otherwise a RECTANGLE DESCENT: the lane descends the tree carrying the index rectangle [u0, u1) x [v0, v1)
//                                   of the tile's cells that reach the node.  A node on another column takes the row's own value and keeps
//                                   the rectangle.  A node on a with threshold th splits the a range at #{u : grid_a[u] <= th} -- the grid
//                                   ascends, so those are a prefix -- clipped to the range; a node on b splits the b range likewise.  An
//                                   empty side is not visited; where both sides hold cells the right one waits on a stack.  A leaf gives
//                                   its output to the cells of its rectangle; the rectangles that reach leaves partition the tile.
//                               The work per (document, tree) is bounded by the tree -- at most its leaves -- not by TA * TB.
//                               Along one path every split that pushes strictly shrinks one of the two ranges, so at most TA + TB - 2
//                               entries wait at a time, whatever the tree's depth.  The stack is lane-private, [entry][lane] in the LDS,
//                               two 32-bit words per entry (rl_partial2_host.h).
//                               A column at or beyond the row stride needs no special case: a node on another column reads 0 there, a
//                               node on a or b never reads the row.  The base is a tile of its own (columns -1, which no node tests),
//                               launched once per call; its cell 0 goes to the base buffer.  Each chain is Ensemble.eval's statement
//                               s = (float)((double)s + (double)out * (double)w[t]), once per tree in tree order.  It walks the
//                               EnsTree arrays, so it serves every model, packed or not.  Scores land as sc[slot in chunk][doc].
//   k_partial_reduce            rl_partial.inc's, unchanged: S1 and S2 of every slot in the fixed order include/rlhip.h defines.
//   No cross-block atomic, no barrier (a lane only ever touches its own LDS column).  Built with -ffp-contract=off.  No CPU fallback.
#include "rl_partial2_host.h"

namespace rl {

constexpr int kP2A = RL_PARTIAL2_TILE_A, kP2B = RL_PARTIAL2_TILE_B;
constexpr int kP2Threads = 64;                               // one wavefront: LDS per lane is what bounds the occupancy, not the block
static_assert(kP2A >= 1 && kP2B >= 1 && kP2A <= kPartial2MaxSide && kP2B <= kPartial2MaxSide, "two-feature partial dependence geometry");

struct Part2Args {
    EnsTree e; const float *w; int MAXN, nt;
    const float *X; int64_t n; int stride;
    const Partial2Tile *tile;                                  // [tiles of the launch]
    const float *val;                                          // [tiles of the launch][TA + TB]
    const uint8_t *uses;                                       // [tiles of the launch][nt]
    float *sc;                                                 // [slots of the chunk][n]
    float *base;                                               // [n]
};

template <int TA, int TB>
__global__ __launch_bounds__(kP2Threads) void k_model_partial2_scores(const Part2Args a)
{
    constexpr int NS = (TA + TB - 2 > 0) ? TA + TB - 2 : 1;
    __shared__ float l_s[TA * TB][kP2Threads];                 // the tile's chains
    __shared__ int32_t l_nd[NS][kP2Threads];                   // the pending siblings: node
    __shared__ uint32_t l_rc[NS][kP2Threads];                  //                       and rectangle
    const Partial2Tile td = a.tile[blockIdx.y];                // wave-uniform, like everything read through blockIdx.y
    const int ca = td.col_a, cb = td.col_b;
    const uint8_t *uses = a.uses + (size_t)blockIdx.y * a.nt;
    float ga[TA], gb[TB];
#pragma unroll
    for (int u = 0; u < TA; u++) ga[u] = a.val[(size_t)blockIdx.y * (TA + TB) + u];
#pragma unroll
    for (int v = 0; v < TB; v++) gb[v] = a.val[(size_t)blockIdx.y * (TA + TB) + TA + v];
    const int ln = threadIdx.x;
    for (int64_t i = (int64_t)blockIdx.x * kP2Threads + ln; i < a.n; i += (int64_t)gridDim.x * kP2Threads) {
        const float *row = a.X + (size_t)i * a.stride;
        for (int c = 0; c < TA * TB; c++) l_s[c][ln] = 0.f;
        for (int t = 0; t < a.nt; t++) {
            const size_t o = (size_t)t * a.MAXN;
            const double wt = (double)a.w[t];
            int nd = 0, fc;
            if (!uses[t]) {
                while ((fc = a.e.feat_idx[o + nd]) != -1) {
                    const float v = (fc < a.stride) ? row[fc] : 0.f;           // -missingZero  DenseDataPoint.java:22-25
                    nd = (v <= a.e.thr[o + nd]) ? a.e.left[o + nd] : a.e.right[o + nd];
                }
                const double ow = (double)a.e.out[o + nd] * wt;
                for (int c = 0; c < TA * TB; c++) l_s[c][ln] = (float)((double)l_s[c][ln] + ow);      // Ensemble.java:113
                continue;
            }
            int u0 = 0, u1 = TA, v0 = 0, v1 = TB, sp = 0;
            for (;;) {
                fc = a.e.feat_idx[o + nd];
                if (fc == -1) {
                    const double ow = (double)a.e.out[o + nd] * wt;
                    for (int u = u0; u < u1; u++)
                        for (int v = v0; v < v1; v++) l_s[u * TB + v][ln] = (float)((double)l_s[u * TB + v][ln] + ow);      // Ensemble.java:113
                    if (sp == 0) break;
                    sp--;
                    nd = l_nd[sp][ln];
                    const uint32_t rc = l_rc[sp][ln];
                    u0 = (int)(rc & 255u); u1 = (int)((rc >> 8) & 255u); v0 = (int)((rc >> 16) & 255u); v1 = (int)(rc >> 24);
                    continue;
                }
                const float th = a.e.thr[o + nd];
                const int le = a.e.left[o + nd], ri = a.e.right[o + nd];
                if (fc == ca) {
                    int p = 0;                                 // the values of a that go left: a prefix of the tile's
#pragma unroll
                    for (int u = 0; u < TA; u++) p += (ga[u] <= th) ? 1 : 0;
                    const int m = min(max(p, u0), u1);
                    if (m == u0) nd = ri;
                    else if (m == u1) nd = le;
                    else {
                        l_nd[sp][ln] = ri;
                        l_rc[sp][ln] = (uint32_t)m | (uint32_t)u1 << 8 | (uint32_t)v0 << 16 | (uint32_t)v1 << 24;
                        sp++;
                        nd = le; u1 = m;
                    }
                } else if (fc == cb) {
                    int p = 0;
#pragma unroll
                    for (int v = 0; v < TB; v++) p += (gb[v] <= th) ? 1 : 0;
                    const int m = min(max(p, v0), v1);
                    if (m == v0) nd = ri;
                    else if (m == v1) nd = le;
                    else {
                        l_nd[sp][ln] = ri;
                        l_rc[sp][ln] = (uint32_t)u0 | (uint32_t)u1 << 8 | (uint32_t)m << 16 | (uint32_t)v1 << 24;
                        sp++;
                        nd = le; v1 = m;
                    }
                } else {
                    const float v = (fc < a.stride) ? row[fc] : 0.f;
                    nd = (v <= th) ? le : ri;
                }
            }
        }
        if (ca < 0) { a.base[i] = l_s[0][ln]; continue; }
        for (int u = 0; u < td.cnt_a; u++)
            for (int v = 0; v < td.cnt_b; v++) a.sc[(size_t)(td.slot0 + u * td.cnt_b + v) * a.n + i] = l_s[u * TB + v][ln];
    }
}

static thread_local double g_pd2_walk_ms = 0.0, g_pd2_reduce_ms = 0.0;  // the last partial2 call of this thread, device events

}  // namespace rl

extern "C" {

int rl_model_predict_partial2(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *pairs, int32_t n_pairs,
                              const int32_t *grid_off, const float *grid, int64_t scratch_bytes, float *out_base, double *out_mean,
                              double *out_shift2, float *out_ice)
{
    const std::string w = "rl_model_predict_partial2: ";
    std::string err;
    int rc = partial2_check(w, X, n_docs, row_stride, pairs, n_pairs, grid_off, grid, scratch_bytes, out_mean, out_shift2, err);
    if (rc) return fail(rc, err);
    if (!m) return fail(RL_ERR_INVALID, w + "null model");             // (after the arguments a machine without a device can check)
    if (m->trees.empty()) return fail(RL_ERR_INVALID, w + "the model has no trees");
    g_pd2_walk_ms = g_pd2_reduce_ms = 0.0;
    RL_HIP(hipSetDevice(m->device));
    int64_t n_cells = 0;
    for (int32_t p = 0; p < n_pairs; p++)
        n_cells += (int64_t)(grid_off[2 * p + 1] - grid_off[2 * p]) * (int64_t)(grid_off[2 * p + 2] - grid_off[2 * p + 1]);
    const int chunk = stage_chunk(partial_cell_budget(scratch_bytes, kStageScratchDefault, n_docs), n_docs * (int64_t)sizeof(float), (int32_t)n_cells);
    const Partial2Plan plan = partial2_plan(m->trees, pairs, n_pairs, grid_off, grid, chunk, kP2A, kP2B);
    Part2Args a;
    memset(&a, 0, sizeof(a));
    a.e = m->ens; a.w = m->d_w; a.MAXN = m->maxn; a.nt = plan.n_trees; a.n = n_docs; a.stride = row_stride;
    DevPool pool;
    float *dX = nullptr, *d_val = nullptr; Partial2Tile *d_tile = nullptr; uint8_t *d_uses = nullptr; double *d_s1 = nullptr, *d_s2 = nullptr;
    RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
    RL_HIP(pool.upload(&d_tile, plan.tiles.data(), plan.tiles.size()));
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
    const unsigned gx = (unsigned)std::min<int64_t>(8192, (n_docs + kP2Threads - 1) / kP2Threads);
    auto walk = [&](int32_t t0, int32_t nt) {                            // the tiles t0 .. t0 + nt - 1 in one launch
        a.tile = d_tile + t0; a.val = d_val + (size_t)t0 * (kP2A + kP2B); a.uses = d_uses + (size_t)t0 * a.nt;
        hipLaunchKernelGGL((k_model_partial2_scores<kP2A, kP2B>), dim3(gx, (unsigned)nt), dim3(kP2Threads), 0, 0, a);
        return hipGetLastError();
    };
    for (int32_t ci = 0; ci < plan.chunks(); ci++) {
        const int32_t t0 = plan.first[(size_t)ci], nt = plan.first[(size_t)ci + 1] - t0, ns = plan.slots[(size_t)ci];
        RL_HIP(hipEventRecord(ev.e[0], 0));
        if (ci == 0) RL_HIP(walk(0, 1));                                 // the base: tile 0, once per call
        RL_HIP(walk(t0, nt));
        RL_HIP(hipEventRecord(ev.e[1], 0));
        hipLaunchKernelGGL(k_partial_reduce, dim3((unsigned)ns), dim3(kThreads), 0, 0, (const float *)a.sc, (const float *)a.base, n_docs, d_s1, d_s2);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[2], 0));
        RL_HIP(hipMemcpy(s1.data(), d_s1, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
        RL_HIP(hipMemcpy(s2.data(), d_s2, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
        if (ci == 0 && out_base) RL_HIP(hipMemcpy(out_base, a.base, (size_t)n_docs * sizeof(float), hipMemcpyDeviceToHost));
        for (int32_t t = t0; t < t0 + nt; t++) {                         // a tile's row of cells is a run of the call's cells
            const Partial2Tile &td = plan.tiles[(size_t)t];
            for (int32_t u = 0; u < td.cnt_a; u++) {
                const int32_t slot = td.slot0 + u * td.cnt_b, cell = td.cell + u * td.gb;
                if (out_ice)
                    RL_HIP(hipMemcpy(out_ice + (size_t)cell * n_docs, a.sc + (size_t)slot * n_docs, (size_t)td.cnt_b * n_docs * sizeof(float), hipMemcpyDeviceToHost));
                for (int32_t v = 0; v < td.cnt_b; v++) {
                    out_mean[cell + v] = s1[(size_t)(slot + v)] / (double)n_docs;
                    out_shift2[cell + v] = s2[(size_t)(slot + v)] / (double)n_docs;
                }
            }
        }
        RL_HIP(hipDeviceSynchronize());
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_pd2_walk_ms += (double)ms;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
        g_pd2_reduce_ms += (double)ms;
    }
    m->last_path = RL_MODEL_PATH_PARTIAL2;
    return RL_OK;
}

int rl_debug_partial2_times(double *walk_ms, double *reduce_ms)
{
    if (!walk_ms || !reduce_ms) return fail(RL_ERR_INVALID, "rl_debug_partial2_times: null argument");
    *walk_ms = g_pd2_walk_ms;
    *reduce_ms = g_pd2_reduce_ms;
    return RL_OK;
}

}  // extern "C"
