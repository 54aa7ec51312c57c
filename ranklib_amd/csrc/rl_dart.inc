// rl_dart.inc -- DART, dropout boosting (rl_set_dart, DESIGN.md 36): the kernels and the trainer's state.  The stages that launch them are
// enqueue_dart_drop and enqueue_dart_restore (rl_round.inc); the draw and the weight arithmetic are rl_dart_host.h.  Included by rl_trainer.hip
// behind rl_kernels_round.inc (Ctx, EnsTree, kThreads).
//
// Round m takes the trees of its drop set D out of modelScores before the lambdas are computed and puts them back, rescaled, before the new
// tree is added.  The trainer knows where every document ended up in every tree it grew (Ctx::leaf_of, left behind by the leaf sums' gather),
// so it keeps that: hist[tree][document], 2 bytes each, the NODE of the exported tree (EnsTree) the document sits in.  The output such an entry
// indexes is EnsTree::out[tree][node] -- the exported trees are the output tables, no copy of them is kept.  Taking a tree out of a document's
// score is then one 2-byte read and one LDS lookup instead of a walk of the tree on the document's row.
//
//   k_dart_record        hist[m][d] of the training rows from leaf_of: leaf-table position -> node -> its id in the exported tree
//   k_valid_update_rec   k_valid_update (rl_k_ensemble.inc) that also leaves the node of every validation row in hist[m][.]
//   k_dart_drop<TRAIN>   per document, in f64 with a rounding after every product and every sum (the products of two floats are exact):
//                            s' = s;  s' -= (double)w_i * (double)o_i     for i in D ascending        the thinned score
//                            r  = 0;  r  += (double)w_i' * (double)o_i    for i in D ascending        what goes back in
//                        TRAIN: scores = s' (the rank and lambda kernels read it), base = s' + r;  !TRAIN (validation rows): scores = s' + r
//   k_dart_weights       the per-tree weight array behind k_ensemble_eval: w[i] = w_i' for i in D, w[m] = w_m
//
// k_dart_drop: a block owns a tile of 256 lanes x 4 consecutive documents.  A lane reads its four history entries of a dropped tree as one
// 8-byte load (a wavefront: 512 contiguous bytes per tree); the tree's id and its two weights come from the round's argument table at a
// wave-uniform index, i.e. through the scalar cache.  The dropped trees' output tables are staged into LDS in chunks of as many trees as fit
// half of the block's LDS: the two halves alternate, so a chunk costs ONE barrier (a thread that has passed the barrier of chunk j + 1 has
// finished its reads of chunk j, whose half chunk j + 2 overwrites).  Every document keeps its two chains in registers across the chunks: the
// chunk size (RLHIP_DART_CHUNK) cannot change a bit.  The tables' LDS stride is odd, so equal nodes of neighbouring trees sit on different
// banks.  No atomics, nothing crosses a block; lanes behind the last document load and store nothing.
//
//   -Rpass-analysis=kernel-resource-usage, gfx950:
//     k_dart_drop<true>    TotalSGPRs: 88  VGPRs: 60  AGPRs: 0  ScratchSize: 0  Occupancy [waves/SIMD]: 8  spills: 0  LDS Size [bytes/block]: 0 (+ dynamic)
//     k_dart_drop<false>   TotalSGPRs: 86  VGPRs: 60  AGPRs: 0  ScratchSize: 0  Occupancy [waves/SIMD]: 8  spills: 0  LDS Size [bytes/block]: 0 (+ dynamic)
//   (at the default chunk the dynamic 64 KB, not the registers, bound a CU at two blocks; a round that drops few trees asks for as much as it uses)

namespace rl {

constexpr int kDartLanes = 256, kDartDocs = 4, kDartTile = kDartLanes * kDartDocs;
constexpr size_t kDartLdsBytes = 64 * 1024;                       // both halves together

__host__ __device__ __forceinline__ int dart_lds_stride(int MAXN) { return MAXN | 1; }
// trees a chunk holds: what fits half the LDS, or the knob's value where that is smaller (0: unset)
static int dart_chunk_trees(int MAXN, int knob) { const int fit = std::max(1, (int)(kDartLdsBytes / 2 / ((size_t)dart_lds_stride(MAXN) * sizeof(float)))); return knob > 0 ? std::min(knob, fit) : fit; }

__global__ __launch_bounds__(kThreads) void k_dart_record(const Ctx c, uint16_t *row)
{
    __shared__ uint16_t s_node[1024];                             // (round_streams_scores: at most 1024 leaves)
    const int nl = min(c.st->n_leaves, 1024);
    for (int i = threadIdx.x; i < nl; i += kThreads) s_node[i] = (uint16_t)c.nodes[c.leaf_node[i]].fid;
    __syncthreads();
    for (int d = blockIdx.x * kThreads + threadIdx.x; d < c.N; d += gridDim.x * kThreads) row[d] = s_node[min((int)c.leaf_of[d], nl - 1)];
}

__global__ __launch_bounds__(kThreads) void k_valid_update_rec(const EnsTree e, int MAXN, int tree, const float *X, int n, int F, float w, double *vscores, uint16_t *row)
{
    const size_t o = (size_t)tree * MAXN;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const float *x = X + (size_t)i * F;
        int nd = 0;
        while (e.feat_idx[o + nd] != -1) nd = (x[e.feat_idx[o + nd]] <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
        vscores[i] += (double)w * (double)e.out[o + nd];
        row[i] = (uint16_t)nd;
    }
}

// the round's argument table, k entries each: the dropped trees ascending, their weights before and after the round
struct DartArgs { const int32_t *ids; const float *w_old, *w_new; int32_t k; };

template <bool TRAIN>
__global__ __launch_bounds__(kDartLanes) void k_dart_drop(const uint16_t *__restrict__ hist, size_t row_stride, const float *__restrict__ out_tab, int MAXN,
                                                          const DartArgs a, int chunk, int n, double *__restrict__ scores, double *__restrict__ base)
{
    extern __shared__ float s_out[];                              // [2][chunk][stride]
    const int stride = dart_lds_stride(MAXN);
    const int d0 = ((int)blockIdx.x * kDartLanes + (int)threadIdx.x) * kDartDocs;       // (n < 2^31 - 4096: no overflow)
    const bool live = d0 < n;
    double sp[kDartDocs], r[kDartDocs];
#pragma unroll
    for (int u = 0; u < kDartDocs; u++) { sp[u] = (d0 + u < n) ? scores[d0 + u] : 0.0; r[u] = 0.0; }
    for (int c0 = 0, half = 0; c0 < a.k; c0 += chunk, half ^= 1) {
        const int nc = min(chunk, a.k - c0);
        float *tab = s_out + (size_t)half * chunk * stride;
        for (int i = threadIdx.x; i < nc * MAXN; i += kDartLanes) {
            const int j = i / MAXN, nd = i - j * MAXN;
            tab[j * stride + nd] = out_tab[(size_t)a.ids[c0 + j] * MAXN + nd];
        }
        __syncthreads();
        if (!live) continue;                                      // (the barrier above is reached by every lane of the block)
        for (int j = 0; j < nc; j++) {
            const int id = a.ids[c0 + j];
            const double wo = (double)a.w_old[c0 + j], wn = (double)a.w_new[c0 + j];
            const uint2 e = *(const uint2 *)(hist + (size_t)id * row_stride + d0);       // (rows are padded to a multiple of four entries)
            const int nd[kDartDocs] = {(int)(e.x & 0xffffu), (int)(e.x >> 16), (int)(e.y & 0xffffu), (int)(e.y >> 16)};
#pragma unroll
            for (int u = 0; u < kDartDocs; u++) {
                const double o = (double)tab[j * stride + min(nd[u], MAXN - 1)];
                sp[u] = sp[u] - wo * o;
                r[u] = r[u] + wn * o;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kDartDocs; u++) {
        if (d0 + u >= n) continue;
        if (TRAIN) { scores[d0 + u] = sp[u]; base[d0 + u] = sp[u] + r[u]; }
        else scores[d0 + u] = sp[u] + r[u];
    }
}

__global__ __launch_bounds__(kThreads) void k_dart_weights(float *w, const DartArgs a, int m, float w_m)
{
    for (int j = threadIdx.x; j < a.k; j += kThreads) w[a.ids[j]] = a.w_new[j];
    if (threadIdx.x == 0) w[m] = w_m;
}

// the trainer's DART state (rl_trainer::dart); `on` is decided by rl_set_dart, everything on the device by init_dart (rl_init.inc)
struct DartState {
    bool on = false;
    float rate = 0.f; int32_t max_drop = 0; uint64_t seed = 0;
    uint16_t *hist_tr = nullptr, *hist_va = nullptr;              // [n_trees][stride_*]: the node of every document in every tree grown so far
    size_t stride_tr = 0, stride_va = 0;
    double *d_base = nullptr;                                     // [N] the training rows' s' + r between the two stages of a round
    int32_t *d_args = nullptr;                                    // the round's argument table: ids [k], w_old [k], w_new [k]
    // pinned staging of the table, a ring: rounds may be enqueued ahead of the device (rl_boost_rounds_async), a slot is written again only after
    // the copy out of it has run
    static constexpr int kSlots = 4;
    int32_t *h_args[kSlots] = {nullptr, nullptr, nullptr, nullptr}; hipEvent_t ev[kSlots] = {nullptr, nullptr, nullptr, nullptr}; bool used[kSlots] = {false, false, false, false};
    int chunk = 1;
    std::vector<std::vector<int32_t>> dropped;                    // [round] its drop set
    // the round between its two stages
    DartArgs cur{nullptr, nullptr, nullptr, 0}; float w_m = 0.f;
};

}  // namespace rl
