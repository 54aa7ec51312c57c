// rl_leaves.inc -- the leaf every document reaches in every tree of a model, as small integers: pred_leaf / apply() (rl_model_predict_leaves,
// DESIGN.md 38).  Included at the end of rl_trainer.hip, after rl_contrib.inc (it uses rl_model, RowStream, StageEvents and the tiled
// packing of rl_eval_pack_host.h).  Two kernels:
//   k_model_leaves_tiled  k_model_eval_tiled's walk -- the same packed nodes, the same deal and phases -- over nodes whose leaves hold their
//                         NUMBER where the scorer's hold their output, so a chain ends with the result in a register: no node -> leaf table
//                         and no further LDS read.  The scorer's fifth wavefront, which ran Ensemble.eval's serial float chain, is a WRITER
//                         here: it transposes the previous tile's numbers out of LDS into the layout asked for while the next tile is walked.
//   k_model_leaves        the generic kernel for models the packing refuses (and under RLHIP_EVAL_GENERIC): one chain at a time over the
//                         EnsTree arrays and a node -> leaf-number table, a block per (64 documents, tile of trees), the same writer.
// The output is n_docs x n_trees uint16_t: the kernels are made around their STORES.
//   BY_TREE  out[tree][doc]: a tree's row of a document tile is 128 contiguous bytes.  With an even row length two documents go into one
//            32-bit store and a wavefront stores two trees' rows at once; an odd length takes 16-bit stores, lane = document.
//   BY_ROW   out[doc][tree]: a document's part of a tile is 2 * kEvalTreeTile contiguous bytes.  A lane packs four leaf numbers into one
//            64-bit store, kEvalTreeTile / 4 neighbouring lanes cover a document's run and a wavefront covers the runs of 64 / (kEvalTreeTile / 4)
//            documents with one instruction.  That needs runs that start on 8 bytes (n_trees a multiple of 4) and a whole tile; the last,
//            partial tile of a window and other tree counts take the tail path, 16-bit stores with the lanes still along a document's run.
//            No lane ever stores two bytes at a stride of 2 * n_trees.
#include "rl_leaves_host.h"

namespace rl {

// ---- the writer: a walked tile, sl [tree in tile][kLeavesRow] u16, to global memory.  Wavefront wv of nwv takes every nwv-th store. ----
// out[(t0 + t) * ld + d0 + doc]; d0 is a multiple of 64 and out is aligned, so with an even ld every pair of documents is one aligned word
__device__ __forceinline__ void leaves_write_by_tree(const uint16_t *sl, int tt, int nd, uint16_t *out, int64_t ld, int64_t t0, int64_t d0,
                                                     int lane, int wv, int nwv)
{
    if ((ld & 1) == 0) {
        const int p = (lane & 31) * 2, half = lane >> 5;
        for (int t = 2 * wv + half; t < tt; t += 2 * nwv) {
            uint16_t *dst = out + (size_t)(t0 + t) * (size_t)ld + (size_t)(d0 + p);
            if (p + 1 < nd) *(uint32_t *)dst = *(const uint32_t *)(sl + t * kLeavesRow + p);
            else if (p < nd) *dst = sl[t * kLeavesRow + p];
        }
    } else {
        for (int t = wv; t < tt; t += nwv)
            if (lane < nd) out[(size_t)(t0 + t) * (size_t)ld + (size_t)(d0 + lane)] = sl[t * kLeavesRow + lane];
    }
}

// out[(d0 + doc) * nt + t0 + t]
__device__ __forceinline__ void leaves_write_by_row(const uint16_t *sl, int tt, int nd, uint16_t *out, int64_t nt, int64_t t0, int64_t d0,
                                                    int lane, int wv, int nwv)
{
    if (tt == kEvalTreeTile && (nt & 3) == 0) {
        constexpr int kQ = kEvalTreeTile / 4, kDocs = kWave / kQ;               // lanes of a document's run, documents of one store
        const int q = lane % kQ, ds = lane / kQ;
        for (int i = wv; i * kDocs < kEvalDocs; i += nwv) {
            const int doc = i * kDocs + ds;
            if (ds < kDocs && doc < nd) {
                const uint16_t *s = sl + (4 * q) * kLeavesRow + doc;
                uint2 v;
                v.x = (unsigned)s[0] | ((unsigned)s[kLeavesRow] << 16);
                v.y = (unsigned)s[2 * kLeavesRow] | ((unsigned)s[3 * kLeavesRow] << 16);
                *(uint2 *)(out + (size_t)(d0 + doc) * (size_t)nt + (size_t)(t0 + 4 * q)) = v;
            }
        }
    } else {                                                                    // the tail: a partial tile, or runs that do not start on 8 bytes
        constexpr int kDocs = kWave / kEvalTreeTile;
        const int t = lane % kEvalTreeTile, ds = lane / kEvalTreeTile;
        for (int i = wv; i * kDocs < kEvalDocs; i += nwv) {
            const int doc = i * kDocs + ds;
            if (ds < kDocs && t < tt && doc < nd) out[(size_t)(d0 + doc) * (size_t)nt + (size_t)(t0 + t)] = sl[t * kLeavesRow + doc];
        }
    }
}

template <bool BY_TREE>
__device__ __forceinline__ void leaves_write(const uint16_t *sl, int tt, int nd, uint16_t *out, int64_t ld, int64_t t0, int64_t d0, int lane, int wv,
                                             int nwv)
{
    if (BY_TREE) leaves_write_by_tree(sl, tt, nd, out, ld, t0, d0, lane, wv, nwv);
    else leaves_write_by_row(sl, tt, nd, out, ld, t0, d0, lane, wv, nwv);
}

// ---- the walk of one tile by walker `part`: k_model_eval_tiled's (rl_model_eval.inc), ending in leaf numbers ----
// sT: the tile's packed trees; sXb: the staged rows at this lane's document; pp: the tile's perm and meta; so: the tile's numbers at this lane's document
__device__ __forceinline__ void leaves_walk_tile(const unsigned long long *sT, int MAXN, const unsigned char *sXb, const unsigned char *pp, int part,
                                                 int tt, bool live, uint16_t *so)
{
    const int depth = __builtin_amdgcn_readfirstlane((int)pp[kEvalTreeTile + part]);       // wave-uniform: a scalar loop bound
    if (depth <= 0) return;                                                             // this walker has no tree in the tile
    const unsigned char *tb[kEvalPer];
    unsigned long long v[kEvalPer];
    int li[kEvalPer];
#pragma unroll
    for (int u = 0; u < kEvalPer; u++) {
        li[u] = __builtin_amdgcn_readfirstlane((int)pp[part * kEvalPer + u]);           // 255: no such tree in this (last) tile -- the chain walks tree 0 again, unstored
        tb[u] = (const unsigned char *)(sT + (size_t)(li[u] < tt ? li[u] : 0) * MAXN);
        v[u] = *(const unsigned long long *)tb[u];
    }
    // all chains to the depth of the walker's (kEvalPh1 + 1)-th tree, then the kEvalPh1 deepest, .. as the scorer drops them
    int step = 0;
#define RL_LEAVES_PHASE(NCH, UNTIL)                                                                                                        \
    for (; step < (UNTIL); step++) {                                                                                                       \
        float x[NCH];                                                                                                                      \
        _Pragma("unroll") for (int u = 0; u < NCH; u++) x[u] = *(const float *)(sXb + ((unsigned)(v[u] >> 32) & 0xffffu));                 \
        _Pragma("unroll") for (int u = 0; u < NCH; u++) {       /* value <= threshold goes left; a leaf (-infinity <= its number's bits) stays */ \
            const unsigned off = (unsigned)(v[u] >> 48) + ((x[u] <= __uint_as_float((unsigned)v[u])) ? 0u : 8u);                           \
            v[u] = *(const unsigned long long *)(tb[u] + off);                                                                             \
        }                                                                                                                                  \
    }
    const unsigned char *pd = pp + kEvalTreeTile + kEvalParts + part * kEvalPhases;
    const int end0 = __builtin_amdgcn_readfirstlane((int)pd[0]);
    [[maybe_unused]] const int end1 = __builtin_amdgcn_readfirstlane((int)pd[kEvalPhases >= 2 ? 1 : 0]);
    [[maybe_unused]] const int end2 = __builtin_amdgcn_readfirstlane((int)pd[kEvalPhases >= 3 ? 2 : 0]);
    RL_LEAVES_PHASE(kEvalPer, end0)
#if RL_EVAL_PHASES >= 2
    RL_LEAVES_PHASE(kEvalPh1, end1)
#endif
#if RL_EVAL_PHASES >= 3
    RL_LEAVES_PHASE(kEvalPh2, end2)
#endif
    RL_LEAVES_PHASE(kEvalPhLast, depth)
#undef RL_LEAVES_PHASE
    if (live) {
#pragma unroll
        for (int u = 0; u < kEvalPer; u++) if (li[u] < tt) so[li[u] * kLeavesRow] = (uint16_t)(unsigned)v[u];      // perm undone: row = the tree's place in the tile
    }
}

// nodes: the packed trees of the window, [nt][MAXN]; perm / gdepth: the window's own tiles (leaves_deal_window).  X [n][stride], this
// chunk's rows.  out: BY_TREE [nt][ld], ld = n; otherwise [n][ld], ld = nt.
template <bool BY_TREE>
__global__ __launch_bounds__(kEvalThreads) void k_model_leaves_tiled(const unsigned long long *nodes, int MAXN, int nt, const float *X, int64_t n,
                                                                     int stride, int cols, uint16_t *out, int64_t ld, const unsigned char *perm,
                                                                     const unsigned char *gdepth)
{
    extern __shared__ unsigned char lv_raw[];
    float *sX = (float *)lv_raw;                                               // [cols][kEvalDocs]
    unsigned long long *sT = (unsigned long long *)(sX + (size_t)cols * kEvalDocs);   // [kEvalTreeTile][MAXN]
    uint16_t *sL = (uint16_t *)(sT + (size_t)kEvalTreeTile * MAXN);            // [2][kEvalTreeTile][kLeavesRow] leaf numbers (double buffer)
    unsigned char *sP = (unsigned char *)(sL + 2 * kEvalTreeTile * kLeavesRow);       // [kEvalTreeTile + kEvalMetaDepths]: only the walkers read it, one buffer (the writer needs no perm)
    const int tid = threadIdx.x, doc = tid & (kEvalDocs - 1), part = tid / kEvalDocs;
    const bool walker = part < kEvalParts;
    const int tile_words = kEvalTreeTile * MAXN;                               // <= kEvalThreads * kEvalPrefetch (eval_pack checks it)
    const unsigned char *sXb = (const unsigned char *)sX + doc * 4;
    for (int64_t tile = blockIdx.x; tile * kEvalDocs < n; tile += gridDim.x) {
        const int64_t d0 = tile * kEvalDocs;
        const int nd = (int)min((int64_t)kEvalDocs, n - d0);
        __syncthreads();
        const float *src = X + (size_t)d0 * stride;                            // the tile is one contiguous range of X
        for (int e = tid; e < nd * stride; e += kEvalThreads) { const int dd = e / stride, c = e - dd * stride; sX[c * kEvalDocs + dd] = src[e]; }
        for (int e = tid; e < (cols - stride) * kEvalDocs; e += kEvalThreads) sX[stride * kEvalDocs + e] = 0.f;
        unsigned long long pre[kEvalPrefetch];
#pragma unroll
        for (int u = 0; u < kEvalPrefetch; u++) { const int e = tid + u * kEvalThreads; pre[u] = (e < min(tile_words, nt * MAXN)) ? nodes[e] : 0ull; }
        __syncthreads();
        if (tid < kEvalDocs) sX[tid] = -__builtin_inff();                      // column 0: what a leaf "reads"
        int k = 0, tt_prev = 0;
        for (int t0 = 0; t0 < nt; t0 += kEvalTreeTile, k++) {
            const int tt = min(kEvalTreeTile, nt - t0);
            const int cb = k & 1;
            __syncthreads();                                                   // tile k-1 walked (its numbers complete), tile k-2 written, sT free
#pragma unroll
            for (int u = 0; u < kEvalPrefetch; u++) { const int e = tid + u * kEvalThreads; if (e < tile_words) sT[e] = pre[u]; }
            if (tid < kEvalTreeTile) sP[tid] = perm[(size_t)k * kEvalTreeTile + tid];
            else if (tid < kEvalTreeTile + kEvalMetaDepths) sP[tid] = gdepth[(size_t)k * kEvalMetaDepths + (tid - kEvalTreeTile)];
            __syncthreads();
            {   // next tile -> registers (in flight during the walk)
                const size_t nb = (size_t)(t0 + kEvalTreeTile) * MAXN;
                const long long left = (long long)nt * MAXN - (long long)nb;
#pragma unroll
                for (int u = 0; u < kEvalPrefetch; u++) { const int e = tid + u * kEvalThreads; pre[u] = (e < tile_words && e < left) ? nodes[nb + e] : 0ull; }
            }
            if (walker)
                leaves_walk_tile(sT, MAXN, sXb, sP, part, tt, doc < nd, sL + (size_t)cb * kEvalTreeTile * kLeavesRow + doc);
            else if (k > 0)                                                    // write the previous tile while this one is walked
                leaves_write<BY_TREE>(sL + (size_t)(cb ^ 1) * kEvalTreeTile * kLeavesRow, tt_prev, nd, out, ld, (int64_t)t0 - kEvalTreeTile, d0, doc, 0, 1);
            tt_prev = tt;
        }
        __syncthreads();
        if (k > 0)                                                             // the last tile: nothing is left to walk, all five wavefronts write
            leaves_write<BY_TREE>(sL + (size_t)((k - 1) & 1) * kEvalTreeTile * kLeavesRow, tt_prev, nd, out, ld, (int64_t)(k - 1) * kEvalTreeTile, d0, doc, part,
                                  kEvalParts + 1);
    }
}

// The generic kernel.  Block (x, y): documents [64 x, 64 x + 64) (grid-strided) against the trees [first + y * kEvalTreeTile, ..) of the
// model: wavefront w walks every 4th tree of the tile for lane = document, leafno [trees][MAXN] turns the node reached into its number,
// and the four wavefronts write the tile out as the tiled kernel's writer does.  t0 of `out` counts from the window's first tree.
template <bool BY_TREE>
__global__ __launch_bounds__(kThreads) void k_model_leaves(const EnsTree e, const uint16_t *leafno, int MAXN, int first, int nt, const float *X, int64_t n,
                                                           int stride, uint16_t *out, int64_t ld)
{
    __shared__ alignas(8) uint16_t sl[kEvalTreeTile * kLeavesRow];            // (the writer reads pairs of documents as 32-bit words)
    const int doc = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int t0 = (int)blockIdx.y * kEvalTreeTile, tt = min(kEvalTreeTile, nt - t0);
    for (int64_t tile = blockIdx.x; tile * kEvalDocs < n; tile += gridDim.x) {
        const int64_t d0 = tile * kEvalDocs;
        const int nd = (int)min((int64_t)kEvalDocs, n - d0);
        __syncthreads();                                                       // the tile before is written
        if (doc < nd) {
            const float *row = X + (size_t)(d0 + doc) * stride;
            for (int t = wv; t < tt; t += kThreads / kWave) {
                const size_t o = (size_t)(first + t0 + t) * MAXN;
                int j = 0, fc;
                while ((fc = e.feat_idx[o + j]) != -1) {
                    const float v = (fc < stride) ? row[fc] : 0.f;             // -missingZero  DenseDataPoint.java:22-25
                    j = (v <= e.thr[o + j]) ? e.left[o + j] : e.right[o + j];
                }
                sl[t * kLeavesRow + doc] = leafno[o + j];
            }
        }
        __syncthreads();
        leaves_write<BY_TREE>(sl, tt, nd, out, ld, t0, d0, doc, wv, kThreads / kWave);
    }
}

static thread_local double g_lv_walk_ms = 0.0;                                 // this thread's last rl_model_predict_leaves call, device events

// What the first rl_model_predict_leaves call of a model makes: the node -> leaf-number table of the generic kernel, and -- where the
// tiled packing takes the model -- the packed nodes with leaf numbers for outputs and the trees' depths.
// A handle made under RLHIP_EVAL_GENERIC never takes the tiled kernel and gets no second pack.  A call that fails midway leaves what it
// uploaded on the model and the next call makes only what is missing.  Like rl_model_cover's node copy this is unguarded: one handle is
// not for two threads at once (rlhip.h).
static int leaves_prepare(rl_model *m)
{
    if (m->leaves_ready) return RL_OK;
    const size_t nt = m->trees.size(), en = nt * (size_t)m->maxn;
    if (!m->d_leaf_no) {
        std::vector<uint16_t> no(en, 0);
        for (size_t i = 0; i < nt; i++) leaves_number(m->trees[i], no.data() + i * m->maxn);
        RL_HIP(m->pool.upload(&m->d_leaf_no, no.data(), en));
    }
    const EvalPack pk = m->knobs.generic ? EvalPack() : eval_pack(leaves_as_outputs(m->trees), m->maxn, m->knobs.deal, m->knobs.phased);
    if (pk.ok) {
        m->leaf_depth.resize(nt);
        for (size_t i = 0; i < nt; i++) m->leaf_depth[i] = leaves_tree_depth(m->trees[i]);
        if (!m->d_leaf_pack) RL_HIP(m->pool.upload(&m->d_leaf_pack, pk.nodes.data(), pk.nodes.size()));
        RL_HIP(hipFuncSetAttribute((const void *)k_model_leaves_tiled<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvalLdsBudget));
        RL_HIP(hipFuncSetAttribute((const void *)k_model_leaves_tiled<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvalLdsBudget));
    }
    m->leaves_ready = true;
    return RL_OK;
}

// The walk of a window of trees into DEVICE memory: what rl_model_predict_leaves launches per chunk, and what rl_near.inc launches into
// the leaf-number buffers its match reads.  open() makes the model's tables (leaves_prepare), picks the kernel and deals the window;
// launch() enqueues one walk of nr rows dX [nr][row_stride] on the null stream: out [n_trees][ld] by tree, ld >= nr, or [nr][ld] by row,
// ld >= n_trees -- the writer takes its 64-bit stores where ld is a multiple of 4.
struct LeavesWalk {
    rl_model *m = nullptr;
    bool tiled = false;
    int cols = 0, row_stride = 0, first_tree = 0, n_trees = 0;
    size_t lds = 0;
    int64_t tree_tiles = 0;
    unsigned char *d_perm = nullptr, *d_meta = nullptr;

    int open(rl_model *model, DevPool &pool, const std::string &w, int32_t stride, int32_t first, int32_t nt)
    {
        m = model; row_stride = stride; first_tree = first; n_trees = nt;
        tree_tiles = ((int64_t)nt + kEvalTreeTile - 1) / kEvalTreeTile;
        const int rc = leaves_prepare(m);
        if (rc) return rc;
        cols = (int)std::min<int64_t>(INT32_MAX, std::max<int64_t>(row_stride, (int64_t)m->maxcol + 1));
        lds = leaves_tiled_lds(cols, m->maxn);
        tiled = m->d_leaf_pack && lds <= kEvalLdsBudget && !m->knobs.generic;
        if (!tiled && tree_tiles > 65535) return fail(RL_ERR_UNSUPPORTED, w + "more than 65535 tiles of trees per call of the generic kernel");
        if (tiled) {                                                           // the window as tiles of its own
            std::vector<unsigned char> perm, meta;
            leaves_deal_window(m->leaf_depth.data() + first_tree, n_trees, m->knobs.deal, m->knobs.phased, perm, meta);
            RL_HIP(pool.upload(&d_perm, perm.data(), perm.size()));
            RL_HIP(pool.upload(&d_meta, meta.data(), meta.size()));
        }
        return RL_OK;
    }

    int launch(bool by_tree, const float *dX, int64_t nr, uint16_t *dO, int64_t ld) const
    {
        const int64_t tiles = (nr + kEvalDocs - 1) / kEvalDocs;
        if (tiled) {
            const unsigned long long *nodes = m->d_leaf_pack + (size_t)first_tree * m->maxn;
            auto k = by_tree ? k_model_leaves_tiled<true> : k_model_leaves_tiled<false>;
            hipLaunchKernelGGL(k, dim3((unsigned)std::min<int64_t>(tiles, 256 * 256)), dim3(kEvalThreads), lds, 0, nodes, m->maxn, (int)n_trees,
                               dX, nr, row_stride, cols, dO, ld, (const unsigned char *)d_perm, (const unsigned char *)d_meta);
        } else {
            // (document tiles x tree tiles): a long window fills the chip even with few documents
            auto k = by_tree ? k_model_leaves<true> : k_model_leaves<false>;
            hipLaunchKernelGGL(k, dim3((unsigned)std::min<int64_t>(tiles, 256 * 256), (unsigned)tree_tiles), dim3(kThreads), 0, 0, m->ens,
                               (const uint16_t *)m->d_leaf_no, m->maxn, (int)first_tree, (int)n_trees, dX, nr, row_stride, dO, ld);
        }
        RL_HIP(hipGetLastError());
        return RL_OK;
    }
};

}  // namespace rl

extern "C" {

int rl_model_leaf_counts(const rl_model *m, int32_t *leaves, int32_t cap, int32_t *n)
{
    if (!m) return fail(RL_ERR_INVALID, "rl_model_leaf_counts: null model");
    if (n) *n = (int32_t)m->trees.size();
    if (leaves) for (int i = 0; i < cap && i < (int)m->trees.size(); i++) leaves[i] = leaves_count(m->trees[i]);
    return RL_OK;
}

int rl_model_predict_leaves(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, int32_t first_tree, int32_t n_trees, int32_t layout,
                            uint16_t *out)
{
    static const std::string w = "rl_model_predict_leaves: ";
    static_assert(RL_ERR_INVALID == -1 && RL_ERR_UNSUPPORTED == -4, "leaves_check returns these");
    std::string err;
    int rc = leaves_check(w, m ? (int64_t)m->trees.size() : -1, X, n_docs, row_stride, first_tree, &n_trees, layout, out, err);
    if (rc) return fail(rc, err);
    for (int32_t t = first_tree; t < first_tree + n_trees; t++)
        if (leaves_count(m->trees[t]) > kLeavesMax)
            return fail(RL_ERR_UNSUPPORTED, w + "tree " + std::to_string(t) + " has " + std::to_string(leaves_count(m->trees[t])) +
                                                " leaves: a leaf number is 16 bits, 65536 leaves at most");
    g_lv_walk_ms = 0.0;
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    const bool by_tree = layout == RL_LEAVES_BY_TREE;
    RowStream rows;
    uint16_t *dO = nullptr;
    if ((rc = rows.open(n_docs, row_stride, 0, (int64_t)row_stride * 4 + 2 * (int64_t)n_trees))) return rc;
    // A chunk that is not the whole call holds whole document tiles: its BY_TREE rows are then even (the writer's 32-bit stores) and every
    // tile's part of a row is a whole 128-byte line.  Only the call's last chunk can have an odd length.
    if (rows.chunk < n_docs && rows.chunk >= kEvalDocs) rows.chunk -= rows.chunk % kEvalDocs;
    RL_HIP(rows.pool.alloc(&dO, (size_t)rows.chunk * n_trees));
    LeavesWalk lw;
    if ((rc = lw.open(m, rows.pool, w, row_stride, first_tree, n_trees))) return rc;
    const bool tiled = lw.tiled;
    auto walk = [&](int64_t nr) -> int { return lw.launch(by_tree, rows.dX, nr, dO, by_tree ? nr : (int64_t)n_trees); };
    if (!by_tree) {                                                            // a chunk's rows are one contiguous piece of out
        rc = rows.run(X, n_docs, row_stride, walk, (const uint16_t *)dO, out, (int64_t)n_trees);
        g_lv_walk_ms = rows.ms;
    } else {                                                                   // a chunk is a band of columns of out [n_trees][n_docs]: a pitched copy per chunk
        StageEvents ev;
        RL_HIP(ev.create());
        int64_t r0 = 0;
        rc = rows.run(X, n_docs, row_stride, [&](int64_t nr) -> int {
            RL_HIP(hipEventRecord(ev.e[0], 0));
            const int wrc = walk(nr);
            if (wrc) return wrc;
            RL_HIP(hipEventRecord(ev.e[1], 0));
            RL_HIP(hipEventSynchronize(ev.e[1]));
            RL_HIP(hipMemcpy2D(out + r0, (size_t)n_docs * 2, dO, (size_t)nr * 2, (size_t)nr * 2, (size_t)n_trees, hipMemcpyDeviceToHost));
            float t = 0.f;
            RL_HIP(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
            g_lv_walk_ms += (double)t;
            r0 += nr;
            return RL_OK;
        }, (const uint16_t *)nullptr, (uint16_t *)nullptr, (int64_t)0);
    }
    if (rc) return rc;
    m->last_path = tiled ? RL_MODEL_PATH_TILED : RL_MODEL_PATH_GENERIC;
    return RL_OK;
}

int rl_debug_leaves_times(double *walk_ms)
{
    if (!walk_ms) return fail(RL_ERR_INVALID, "rl_debug_leaves_times: null argument");
    *walk_ms = g_lv_walk_ms;
    return RL_OK;
}

}  // extern "C"
