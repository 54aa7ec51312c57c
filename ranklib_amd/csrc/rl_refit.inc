// rl_refit.inc -- a trainer keeps the structure of a saved model's trees and recomputes their leaf values on its own data (rl_refit_model_text).
// DESIGN.md 33.  Included by rl_trainer.hip behind rl_resume.inc (it uses check_adoptable, upload_adopted and settle_adopted of that file, and
// enqueue_lambdas, enqueue_leaf_outputs and enqueue_scores_and_metrics of rl_round.inc).
//
// A refit round is a boosting round whose tree is GIVEN: the lambdas of the current scores, then every training document is put into its leaf of
// tree r in the layout the leaf machinery reads -- a contiguous range of c.idx[0] per leaf, leaves in left-first DFS order, the documents of a leaf in
// ascending index, which is the order Split.getSamples() has after stable partitions of 0 .. N-1 -- then the round's own leaf evaluator, the blend
// with the old outputs, and the round's score update, ranking and metrics.
//
//   k_refit_route<TILED>  a block is ONE wavefront and owns tiles of kRefitDocs documents, a lane per document.  TILED: the tile's rows are staged
//                         into LDS transposed and rotated -- column c of document dd at sX[c * 64 + ((dd + c) & 63)].  The staging writes of
//                         adjacent lanes are adjacent columns of one row: without the rotation they are 64 words apart, one bank (ds_write banks
//                         are word % 32), and a tile of F columns is written but only a path's few columns are read; with it a write's bank is
//                         (dd + c) % 32, distinct over 32 adjacent lanes.  A read of column c by lane l has bank (l + c) % 32: free of conflicts
//                         while the lanes ask for one column (the root, the upper levels), a few ways where the paths have parted.  The direct
//                         arm reads row[c] from global memory.  The lane walks tree r (value <= threshold goes left, Split.java:118), stores the
//                         rank of its leaf in left-first DFS order to leaf_of and counts it in the tile's LDS counters, which leave as row `tile`
//                         of the [tile][leaf] table.
//   k_refit_offsets       one block per leaf: the exclusive scan of the leaf's column of that table over the tiles, in place (a tile's base inside
//                         the leaf), and the leaf's total.
//   k_refit_nodes         one block: the leaves' starts (the scan of the totals) and the NodeRec of every node of tree r as the leaf machinery
//                         and the score kernels read it.
//   k_refit_scatter       tiles as in k_refit_route: a lane's position inside its tile and leaf is the number of lower lanes with the same leaf
//                         -- a ballot per distinct leaf of the wavefront and a population count below the lane -- so the place of every document
//                         is a function of the data alone.
//   k_refit_store         one block, behind the leaf evaluator: the empty-leaf rule and the blend; outputs and counts go into t->ens and the
//                         NodeRecs the score update reads.
//   No atomic on global memory, no spin wait, no inline assembly.  Built with -ffp-contract=off like the rest: the blend is two double products
//   and a separate add.
namespace rl {

constexpr int kRefitDocs = 64;                                   // documents per tile = lanes of a block
constexpr size_t kRefitLdsMax = (size_t)160 * 1024;              // F <= 640 columns fit a tile
constexpr int kRefitMaxLeaves = kLeafTableCap / 2;               // k_leaf_table lists the leaves of a tree of up to kLeafTableCap nodes by a DFS walk; beyond, it
                                                                 // sorts them by `start`, which the empty leaves of a given tree share with their right neighbours

struct RefitTree {                      // tree r of t->ens and the leaf ranks the host worked out from the text
    const int32_t *feat_idx, *left, *right; const float *thr;       // node i at [i]
    const int32_t *lo, *hi;             // [n_nodes] ranks (in left-first DFS order) of the first and the last leaf below node i; a leaf: lo == hi
    int32_t n_nodes, n_leaves;
};

template <bool TILED>
__global__ __launch_bounds__(kRefitDocs) void k_refit_route(const RefitTree tr, const float *X, int n, int F, uint16_t *leaf_of, int32_t *tile_cnt)
{
    extern __shared__ int32_t rf_lds[];                          // TILED: [F][kRefitDocs] floats while the tile is walked; then [n_leaves] counters
    int32_t *cnt = rf_lds;
    float *sX = (float *)rf_lds;
    const int lane = threadIdx.x;
    const int tiles = (n + kRefitDocs - 1) / kRefitDocs;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int d0 = tile * kRefitDocs;
        const int nd = min(kRefitDocs, n - d0);
        if (TILED) {
            __syncthreads();                                     // the previous tile's counters have been written
            const float *src = X + (size_t)d0 * F;               // the tile is one contiguous range of X
            for (int i = lane; i < nd * F; i += kRefitDocs) { const int dd = i / F, c = i - dd * F; sX[c * kRefitDocs + ((dd + c) & 63)] = src[i]; }
            __syncthreads();
        }
        const bool live = lane < nd;
        const int dl = live ? lane : 0;                          // (idle lanes of the last tile walk document d0 again and store nothing)
        const float *row = X + (size_t)(d0 + dl) * F;
        int node = 0;
        for (;;) {
            const int f = tr.feat_idx[node];
            if (f < 0) break;
            const float v = TILED ? sX[f * kRefitDocs + ((dl + f) & 63)] : row[f];
            node = (v <= tr.thr[node]) ? tr.left[node] : tr.right[node];          // Split.eval: value <= threshold goes left (Split.java:118)
        }
        const int leaf = tr.lo[node];
        __syncthreads();                                         // the tile has been walked (the counters take its place), the previous counters written
        for (int i = lane; i < tr.n_leaves; i += kRefitDocs) cnt[i] = 0;
        __syncthreads();
        if (live) { leaf_of[d0 + lane] = (uint16_t)leaf; atomicAdd(&cnt[leaf], 1); }      // (an LDS counter of this block)
        __syncthreads();
        for (int i = lane; i < tr.n_leaves; i += kRefitDocs) tile_cnt[(size_t)tile * tr.n_leaves + i] = cnt[i];
    }
}

// In: tile_cnt[tile][leaf] documents of the tile in the leaf.  Out, in place: the documents of the leaf in the tiles before; leaf_tot[leaf].
__global__ __launch_bounds__(kScanThreads) void k_refit_offsets(int32_t *tile_cnt, int tiles, int n_leaves, int32_t *leaf_tot)
{
    __shared__ uint32_t sh[kScanThreads / 64];
    const int leaf = blockIdx.x;
    if (leaf >= n_leaves) return;
    const int per = (tiles + kScanThreads - 1) / kScanThreads;   // consecutive tiles of a thread
    const int a = min(tiles, (int)threadIdx.x * per), b = min(tiles, a + per);
    uint32_t mine = 0;
    for (int i = a; i < b; i++) mine += (uint32_t)tile_cnt[(size_t)i * n_leaves + leaf];
    const uint32_t inc = wave_scan_u32(mine);
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t off = inc - mine, tot = 0;
    for (int w2 = 0; w2 < kScanThreads / 64; w2++) { const uint32_t x = sh[w2]; if (w2 < wave) off += x; tot += x; }
    for (int i = a; i < b; i++) {
        const size_t o = (size_t)i * n_leaves + leaf;
        const uint32_t c = (uint32_t)tile_cnt[o];
        tile_cnt[o] = (int32_t)off;
        off += c;
    }
    if (threadIdx.x == 0) leaf_tot[leaf] = (int32_t)tot;
}

// The leaves' starts and the fields of NodeRec that k_leaf_table, the leaf evaluators, k_leaf_output and the score kernels read: left, right, start,
// count, gcount, buf (every list is in c.idx[0]), fid and the old output.  Node i of the tree is node record i; the root is record 0 as in a grown tree.
__global__ __launch_bounds__(kThreads) void k_refit_nodes(const Ctx c, const RefitTree tr, const float *old_out, const int32_t *leaf_tot, int32_t *leaf_start)
{
    __shared__ int32_t s_start[kRefitMaxLeaves + 1];
    if (threadIdx.x == 0) {
        int32_t run = 0;
        for (int l = 0; l < tr.n_leaves; l++) { s_start[l] = run; run += leaf_tot[l]; }
        s_start[tr.n_leaves] = run;
    }
    __syncthreads();
    for (int l = threadIdx.x; l <= tr.n_leaves; l += kThreads) leaf_start[l] = s_start[l];
    for (int i = threadIdx.x; i < tr.n_nodes; i += kThreads) {
        NodeRec &X = c.nodes[i];
        const bool leaf = tr.feat_idx[i] < 0;
        const int32_t start = s_start[tr.lo[i]], count = s_start[tr.hi[i] + 1] - start;
        X.left = leaf ? -1 : tr.left[i]; X.right = leaf ? -1 : tr.right[i];
        X.start = start; X.count = count; X.gcount = count;
        X.buf = 0; X.fid = i;
        X.output = leaf ? old_out[i] : 0.f;
    }
    if (threadIdx.x == 0) { c.st->n_nodes = tr.n_nodes; c.st->n_splits = (tr.n_nodes - 1) / 2; }
}

// tile_base[tile][leaf] and leaf_start[leaf] as the two kernels above left them; idx: c.idx[0]
__global__ __launch_bounds__(kRefitDocs) void k_refit_scatter(const uint16_t *leaf_of, const int32_t *tile_base, const int32_t *leaf_start, int n, int n_leaves, int32_t *idx)
{
    const int lane = threadIdx.x;
    const int tiles = (n + kRefitDocs - 1) / kRefitDocs;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int d = tile * kRefitDocs + lane;
        const bool live = d < n;
        const int leaf = live ? (int)leaf_of[d] : -1;
        int pos = 0;
        unsigned long long todo = __ballot(live);
        while (todo) {                                           // (wave-uniform: one turn per distinct leaf of the wavefront, the lowest open lane's first)
            const int lead = __ffsll((long long)todo) - 1;
            const int want = __shfl(leaf, lead);
            const unsigned long long same = __ballot(live && leaf == want);
            if (leaf == want) pos = __popcll(same & ((1ull << lane) - 1ull));
            todo &= ~same;
        }
        if (live && leaf < n_leaves) {
            const int p = leaf_start[leaf] + tile_base[(size_t)tile * n_leaves + leaf] + pos;
            if (p < n) idx[p] = d;                               // (p < n by construction: the guard keeps a broken table from writing outside the list)
        }
    }
}

// Behind the leaf evaluator: NodeRec::output of a leaf is the new value.  A leaf no document reaches keeps its old output (MART's 0 / 0 must not
// reach a model); decay == 0 stores the new value as it is, no arithmetic; else the blend in double.  The stored value goes to t->ens and back into
// the NodeRec, which the score update reads; every node's count goes to t->ens.  empty[0] = leaves that kept their output.
__global__ __launch_bounds__(kThreads) void k_refit_store(const Ctx c, const RefitTree tr, float *ens_out, int32_t *ens_count, float decay, int32_t *empty)
{
    __shared__ int32_t s_empty;
    if (threadIdx.x == 0) s_empty = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < tr.n_nodes; i += kThreads) {
        NodeRec &X = c.nodes[i];
        ens_count[i] = X.gcount;
        if (tr.feat_idx[i] >= 0) continue;
        const float old = ens_out[i], nw = X.output;
        float v;
        if (X.count == 0) { v = old; atomicAdd(&s_empty, 1); }      // (an LDS counter of this block)
        else if (decay == 0.f) v = nw;
        else v = (float)((double)decay * (double)old + (1.0 - (double)decay) * (double)nw);
        ens_out[i] = v; X.output = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) empty[0] = s_empty;
}

// the rank of every leaf in left-first DFS order (Split.leaves, Split.java:100-113) and, for a split, the ranks of the leaves below it
static int leaf_ranks(const HostTree &h, int32_t *lo, int32_t *hi)
{
    int n = 0;
    std::vector<std::pair<int, int>> stack{{0, 0}};       // (node, 0 = entering / 1 = leaving)
    while (!stack.empty()) {
        const auto [x, leaving] = stack.back(); stack.pop_back();
        if (h.left[x] < 0) { lo[x] = hi[x] = n++; continue; }
        if (leaving) { lo[x] = lo[h.left[x]]; hi[x] = hi[h.right[x]]; continue; }
        stack.push_back({x, 1}); stack.push_back({h.right[x], 0}); stack.push_back({h.left[x], 0});
    }
    return n;
}

static bool refit_tiled_ok(const rl_trainer *t) { return (size_t)t->F * kRefitDocs * sizeof(float) <= kRefitLdsMax && !t->knobs.refit_direct; }

}  // namespace rl

extern "C" int rl_refit_model_text(rl_trainer *t, const char *text, float decay, int32_t *stop)
{
    const std::string w = "rl_refit_model_text: ";
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!(decay >= 0.f && decay < 1.f)) return fail(RL_ERR_INVALID, w + "decay must be in [0, 1) (0: the new values alone)");
    std::vector<HostTree> trees;
    std::map<int32_t, int32_t> col_of;
    int rc = check_adoptable(t, w, text, true, trees, col_of);
    if (rc) return rc;
    Ctx &c = t->ctx;
    const int T0 = (int)trees.size(), MAXN = c.MAXN, N = c.N;
    const int leaf_cap = std::min((int)c.L, kRefitMaxLeaves);
    std::vector<int32_t> lo((size_t)T0 * MAXN, 0), hi((size_t)T0 * MAXN, 0), nl(T0);
    int nl_max = 1;
    for (int r = 0; r < T0; r++) {
        nl[r] = leaf_ranks(trees[r], lo.data() + (size_t)r * MAXN, hi.data() + (size_t)r * MAXN);
        if (nl[r] > leaf_cap)
            return fail(RL_ERR_INVALID, w + "tree " + std::to_string(r) + " has " + std::to_string(nl[r]) + " leaves, the leaf machinery of this trainer takes " +
                                        std::to_string(leaf_cap) + " (its -leaf, and at most " + std::to_string(kRefitMaxLeaves) + ")");
        nl_max = std::max(nl_max, nl[r]);
    }
    RL_HIP(hipSetDevice(t->p.device));
    RL_HIP(hipStreamSynchronize(t->stream));
    rc = upload_adopted(t, trees, col_of);
    if (rc) return rc;
    const int tiles = (N + kRefitDocs - 1) / kRefitDocs;
    DevPool scratch;
    int32_t *d_lo = nullptr, *d_hi = nullptr, *d_cnt = nullptr, *d_tot = nullptr, *d_start = nullptr, *d_empty = nullptr;
    RL_HIP(scratch.upload(&d_lo, (const int32_t *)lo.data(), lo.size()));
    RL_HIP(scratch.upload(&d_hi, (const int32_t *)hi.data(), hi.size()));
    RL_HIP(scratch.alloc(&d_cnt, (size_t)tiles * nl_max));
    RL_HIP(scratch.alloc(&d_tot, (size_t)nl_max));
    RL_HIP(scratch.alloc(&d_start, (size_t)nl_max + 1));
    RL_HIP(scratch.alloc(&d_empty, (size_t)T0));
    RL_HIP(hipMemset(d_empty, 0, (size_t)T0 * sizeof(int32_t)));
    RL_HIP(hipFuncSetAttribute((const void *)k_refit_route<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRefitLdsMax));
    const bool stream_scores = round_streams_scores(t);
    const dim3 grid((unsigned)std::min(tiles, 1 << 20));
    hipStream_t s = t->stream;
    for (int r = 0; r < T0; r++) {
        const size_t o = (size_t)r * MAXN;
        const RefitTree tr{t->ens.feat_idx + o, t->ens.left + o, t->ens.right + o, t->ens.thr + o, d_lo + o, d_hi + o, trees[r].n_nodes, nl[r]};
        int n_max = 0;
        if ((rc = enqueue_lambdas(t, n_max)) != RL_OK) return rc;       // round r's lambdas (MART: residuals) of the current scores; t->round == r
        const size_t cnt_lds = (size_t)nl[r] * sizeof(int32_t);      // (at most 2 KB: a tile of one column is 256 bytes)
        if (refit_tiled_ok(t)) {
            t->refit_stats[0]++;
            hipLaunchKernelGGL(k_refit_route<true>, grid, dim3(kRefitDocs), std::max(cnt_lds, (size_t)t->F * kRefitDocs * sizeof(float)), s, tr, (const float *)t->tr.d_X, N, t->F,
                               c.leaf_of, d_cnt);
        } else {      // more columns than a tile holds (F > 640), or RLHIP_REFIT_DIRECT
            t->refit_stats[1]++;
            hipLaunchKernelGGL(k_refit_route<false>, grid, dim3(kRefitDocs), cnt_lds, s, tr, (const float *)t->tr.d_X, N, t->F, c.leaf_of, d_cnt);
        }
        hipLaunchKernelGGL(k_refit_offsets, dim3(nl[r]), dim3(kScanThreads), 0, s, d_cnt, tiles, nl[r], d_tot);
        hipLaunchKernelGGL(k_refit_nodes, dim3(1), dim3(kThreads), 0, s, c, tr, (const float *)(t->ens.out + o), (const int32_t *)d_tot, d_start);
        hipLaunchKernelGGL(k_refit_scatter, grid, dim3(kRefitDocs), 0, s, (const uint16_t *)c.leaf_of, (const int32_t *)d_cnt, (const int32_t *)d_start, N, nl[r], c.idx[0]);
        RL_HIP(hipGetLastError());
        if ((rc = enqueue_leaf_outputs(t, stream_scores)) != RL_OK) return rc;
        hipLaunchKernelGGL(k_refit_store, dim3(1), dim3(kThreads), 0, s, c, tr, t->ens.out + o, t->ens.count + o, decay, d_empty + r);
        if ((rc = enqueue_scores_and_metrics(t, stream_scores, false)) != RL_OK) return rc;      // (no k_export_tree: tree r is in t->ens already)
    }
    rc = settle_adopted(t, T0, stop);
    if (rc) return rc;
    std::vector<int32_t> empty(T0);
    RL_HIP(hipMemcpy(empty.data(), d_empty, (size_t)T0 * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int r = 0; r < T0; r++) t->refit_stats[2] += empty[r];
    return RL_OK;
}

extern "C" int rl_debug_refit_stats(const rl_trainer *t, int64_t *out)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!out) return fail(RL_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; i++) out[i] = t->refit_stats[i];
    return RL_OK;
}
