// rl_contrib.inc -- per-document feature contributions of a tree model (Saabas path attribution) in one pass over a file.  DESIGN.md 26.
// Included at the end of rl_trainer.hip, after rl_model_rows.inc (it uses rl_model and RowStream, the loop that streams a file's rows
// through its kernels).  SlotPass, SlotPlan and slot_stream -- the column plan of a call and its passes -- are shared with rl_shap.inc.
//
//   k_model_cover     one lane per background row.  A block stages a tile of trees in LDS as 16-byte nodes, walks its rows through the
//                     tile (Split.eval: a column at or beyond row_stride reads 0, `v <= thr` goes left, so a NaN goes right) and counts
//                     the LEAF each walk ends in with a non-returning LDS integer add on uint32 counters [tree of tile][node].  It
//                     strides over all of its row tiles before it flushes its non-zero counters, once per tree tile, with non-returning
//                     64-bit integer global atomics.  Integer sums: the result is exact whatever the grid, the block order and the
//                     chunking.  The inner nodes' covers are c[l] + c[r] on the host afterwards (contrib_fill_inner), and so are the node
//                     values (contrib_node_values): a model has a few thousand nodes.  No f64 atomic anywhere.
//   k_model_contribs  one lane per row, a block of 64, 128 or 256 rows.  LDS holds a tile of trees as 32-byte nodes -- feature,
//                     threshold, children, the node's f64 value and the SLOT of its feature (the place of the feature among the requested
//                     columns, or `rest`: resolved on the host per call, so no lookup by feature id is left in the walk and a feature id
//                     of any size costs nothing) -- and the accumulators [slot of the pass][doc of block] f64.  A lane reads and writes
//                     only its own document's column: no atomics, and the lanes of a wavefront hit consecutive 8-byte words.  Per tree
//                     the bias slot takes W * val[root]; per step of the path slot(feature) takes W * (val[next] - val[node]): every slot
//                     is one serial f64 chain in tree order, then path order.  When all C + 2 slots do not fit beside the tree tile the
//                     host makes several column passes of blocks of 64; a pass walks every tree again and keeps the steps whose slot is
//                     its own -- a slot's chain lies in one pass, so the passes cannot change a bit.  The row values are gathered
//                     from global memory, one per step (staging the rows in LDS as k_model_eval_tiled does was measured and lost:
//                     DESIGN.md 26.4).  The block's result is stored transposed: adjacent lanes write adjacent slots of a document.
//   k_model_leaf_sums the f64 sum of weight * leaf output per row, what a row's slots sum to (rl_model_predict_leaf_sums): the command line's check.
//   No cross-block communication, no spin wait.  Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_contrib_host.h"

namespace rl {

struct alignas(16) CoverNode { int32_t feat; float thr; int32_t left, right; };
struct alignas(16) ContribNode { int32_t feat; float thr; int32_t left, right; double val; int32_t slot, pad; };
static_assert(sizeof(CoverNode) == 16 && sizeof(ContribNode) == kContribNodeBytes, "the LDS budgets count these sizes");

constexpr int kCoverTile = 32, kCoverBlocks = 512;            // trees of a tile at most; blocks of a launch at most (each flushes every node once)

static inline int cover_tree_tile(int maxn)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(kCoverTile, (int64_t)(64 * 1024) / ((int64_t)(sizeof(CoverNode) + 4) * maxn)));
}

__global__ __launch_bounds__(kThreads) void k_model_cover(const CoverNode *nodes, int MAXN, int nt, int tile, const float *X, int64_t n,
                                                           int stride, unsigned long long *cover)
{
    extern __shared__ __align__(16) unsigned char cv_raw[];
    CoverNode *sN = (CoverNode *)cv_raw;                               // [tile][MAXN]
    unsigned *sC = (unsigned *)(sN + (size_t)tile * MAXN);             // [tile][MAXN] rows of this block that end in the node
    const int tid = threadIdx.x;
    for (int t0 = 0; t0 < nt; t0 += tile) {
        const int tt = min(tile, nt - t0), words = tt * MAXN;
        __syncthreads();                                               // the tile before is flushed
        const uint4 *src = (const uint4 *)(nodes + (size_t)t0 * MAXN);
        for (int e = tid; e < words; e += kThreads) { ((uint4 *)sN)[e] = src[e]; sC[e] = 0u; }
        __syncthreads();
        for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < n; i += (int64_t)gridDim.x * kThreads) {
            const float *row = X + (size_t)i * stride;
            for (int t = 0; t < tt; t++) {
                const CoverNode *tn = sN + t * MAXN;
                int nd = 0;
                CoverNode cur = tn[0];
                while (cur.feat != -1) {
                    const float v = (cur.feat < stride) ? row[cur.feat] : 0.f;     // -missingZero  DenseDataPoint.java:22-25
                    nd = (v <= cur.thr) ? cur.left : cur.right;                    // Split.java:118
                    cur = tn[nd];
                }
                atomicAdd(&sC[t * MAXN + nd], 1u);                                 // (the result is not used: no return value is asked for)
            }
        }
        __syncthreads();
        for (int e = tid; e < words; e += kThreads) {
            const unsigned c = sC[e];
            if (c) atomicAdd(&cover[(size_t)t0 * MAXN + e], (unsigned long long)c);
        }
    }
}

// What k_model_contribs and k_model_shap share: one lane per row, a block of D rows, the f64 accumulators sA [slots of the pass][D + 1] in
// LDS (a lane reads and writes only its own column), and the block's result stored transposed.
struct SlotPass {
    const float *X; int64_t n; int stride;                             // the chunk's rows
    int32_t s0, ns, slots, bias;                                       // the pass: slots [s0, s0 + ns) of `slots` = C + 2; bias = C + 1
    double *out;                                                       // [n][slots]
};

struct ContribArgs {
    const ContribNode *nodes; const float *w; int MAXN, nt, tile;
    SlotPass p;
};

__global__ __launch_bounds__(kContribDocsMax) void k_model_contribs(const ContribArgs a)
{
    extern __shared__ __align__(16) unsigned char cb_raw[];
    ContribNode *sN = (ContribNode *)cb_raw;                           // [tile][MAXN]
    double *sA = (double *)(sN + (size_t)a.tile * a.MAXN);             // [ns][D + 1]
    const int D = (int)blockDim.x, AS = D + 1, tid = threadIdx.x;
    const int bias = a.p.bias - a.p.s0;                                // in [0, ns) in the pass that holds it
    const int64_t d0 = (int64_t)blockIdx.x * D;                        // one row tile per block: the grid is ceil(n / D), n < 2^31
    const int nd = (int)min((int64_t)D, a.p.n - d0);
    for (int s = 0; s < a.p.ns; s++) sA[s * AS + tid] = 0.0;
    const float *row = a.p.X + (size_t)(d0 + (tid < nd ? tid : 0)) * a.p.stride;
    for (int t0 = 0; t0 < a.nt; t0 += a.tile) {
        const int tt = min(a.tile, a.nt - t0), words = tt * a.MAXN * (kContribNodeBytes / 16);
        __syncthreads();                                               // the tile before is walked
        const uint4 *src = (const uint4 *)(a.nodes + (size_t)t0 * a.MAXN);
        for (int e = tid; e < words; e += D) ((uint4 *)sN)[e] = src[e];
        __syncthreads();
        if (tid < nd) {
            for (int t = 0; t < tt; t++) {
                const ContribNode *tn = sN + t * a.MAXN;
                const double W = (double)a.w[t0 + t];
                ContribNode cur = tn[0];
                if ((unsigned)bias < (unsigned)a.p.ns) sA[bias * AS + tid] = sA[bias * AS + tid] + W * cur.val;
                while (cur.feat != -1) {
                    const float v = (cur.feat < a.p.stride) ? row[cur.feat] : 0.f;     // -missingZero  DenseDataPoint.java:22-25
                    const ContribNode nx = tn[(v <= cur.thr) ? cur.left : cur.right];   // Split.java:118
                    const double d = W * (nx.val - cur.val);
                    const int s = cur.slot - a.p.s0;
                    if ((unsigned)s < (unsigned)a.p.ns) sA[s * AS + tid] = sA[s * AS + tid] + d;
                    cur = nx;
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < nd * a.p.ns; e += D) {                       // transposed: adjacent lanes, adjacent slots of one document
        const int dd = e / a.p.ns, s = e - dd * a.p.ns;
        a.p.out[(size_t)(d0 + dd) * a.p.slots + a.p.s0 + s] = sA[s * AS + dd];
    }
}

// what a row's slots sum to: s = s + (double)w_t * (double)out of the leaf reached, f64, in tree order.  One lane per row over the
// EnsTree arrays, as k_model_eval walks them; the command line measures local accuracy against it.
__global__ __launch_bounds__(kThreads) void k_model_leaf_sums(const EnsTree e, const float *w, int MAXN, int nt, const float *X, int64_t n,
                                                               int stride, double *out)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = X + (size_t)i * stride;
        double s = 0.0;
        for (int t = 0; t < nt; t++) {
            const size_t o = (size_t)t * MAXN;
            int nd = 0, fc;
            while ((fc = e.feat_idx[o + nd]) != -1) {
                const float v = (fc < stride) ? row[fc] : 0.f;                 // -missingZero  DenseDataPoint.java:22-25
                nd = (v <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
            }
            s = s + (double)w[t] * (double)e.out[o + nd];
        }
        out[i] = s;
    }
}

static thread_local double g_cb_cover_ms = 0.0, g_cb_walk_ms = 0.0;    // the last calls of this thread, device events
static thread_local int32_t g_cb_passes = 0;

// The columns of a contributions call (the arguments', or every feature of the model) as sorted (id, place) pairs, the C + 2 slots they
// make -- the columns, the rest, the bias -- and how the slots go through the kernel: rows of a block and slots of a pass, set by the
// kernel's own plan (contrib_plan, shap_plan).
struct SlotPlan {
    std::vector<std::pair<int32_t, int32_t>> sorted;
    int64_t C = 0, slots = 0, per_pass = 0;
    int docs = 0;
    int32_t passes() const { return (int32_t)((slots + per_pass - 1) / per_pass); }
};

static SlotPlan slot_plan(const rl_model *m, const int32_t *columns, int32_t n_columns)
{
    SlotPlan sp;
    const std::vector<int32_t> cols = columns ? std::vector<int32_t>(columns, columns + n_columns) : m->features;
    sp.C = (int64_t)cols.size(); sp.slots = sp.C + 2;
    sp.sorted.resize((size_t)sp.C);
    for (int64_t c = 0; c < sp.C; c++) sp.sorted[(size_t)c] = {cols[(size_t)c], (int32_t)c};
    std::sort(sp.sorted.begin(), sp.sorted.end());
    return sp;
}

// The rows of a call through `kernel`, whose other arguments a holds: chunks of rows and of their output [chunk][slots] within
// scratch_bytes, and per chunk the column passes, one launch per per_pass slots; lds(ns) is the kernel's dynamic LDS for a pass of ns slots.
template <class Args, class Lds>
static int slot_stream(void (*kernel)(const Args), Args &a, const SlotPlan &sp, const float *X, int64_t n_docs, int32_t row_stride,
                       int64_t scratch_bytes, double *out, RowStream &rows, Lds lds)
{
    const int rc = rows.open(n_docs, row_stride, scratch_bytes, (int64_t)row_stride * 4 + 8 * sp.slots);
    if (rc) return rc;
    RL_HIP(rows.pool.alloc(&a.p.out, (size_t)rows.chunk * sp.slots));
    a.p.X = rows.dX; a.p.stride = row_stride; a.p.slots = (int32_t)sp.slots; a.p.bias = (int32_t)(sp.C + 1);
    return rows.run(X, n_docs, row_stride, [&](int64_t nr) -> int {
        a.p.n = nr;
        for (int64_t s0 = 0; s0 < sp.slots; s0 += sp.per_pass) {
            a.p.s0 = (int32_t)s0; a.p.ns = (int32_t)std::min(sp.per_pass, sp.slots - s0);
            hipLaunchKernelGGL(kernel, dim3((unsigned)((nr + sp.docs - 1) / sp.docs)), dim3(sp.docs), lds(a.p.ns), 0, a);
            RL_HIP(hipGetLastError());
        }
        return RL_OK;
    }, a.p.out, out, sp.slots);
}

// the leaves' counts of n_docs background rows, leaf [trees][maxn]
static int cover_count(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, int tile, size_t lds, std::vector<uint64_t> &leaf)
{
    RL_HIP(hipSetDevice(m->device));
    if (!m->d_cover_nodes) {                                           // the trees as k_model_cover stages them, made by the model's first call
        std::vector<CoverNode> cn(leaf.size(), CoverNode{-1, 0.f, -1, -1});
        for (size_t t = 0; t < m->trees.size(); t++) {
            const HostTree &h = m->trees[t];
            for (int j = 0; j < h.n_nodes; j++) cn[t * m->maxn + j] = CoverNode{h.feature[j], h.threshold[j], h.left[j], h.right[j]};
        }
        CoverNode *d = nullptr;
        RL_HIP(m->pool.upload(&d, cn.data(), cn.size()));
        m->d_cover_nodes = d;
    }
    RL_HIP(hipFuncSetAttribute((const void *)k_model_cover, hipFuncAttributeMaxDynamicSharedMemorySize, kContribLds));
    RowStream rows;
    int rc = rows.open(n_docs, row_stride, 0, (int64_t)row_stride * 4);
    if (rc) return rc;
    unsigned long long *d_cover = nullptr;
    RL_HIP(rows.pool.alloc(&d_cover, leaf.size()));
    RL_HIP(hipMemset(d_cover, 0, leaf.size() * sizeof(unsigned long long)));
    rc = rows.run(X, n_docs, row_stride, [&](int64_t nr) -> int {
        hipLaunchKernelGGL(k_model_cover, dim3((unsigned)std::min<int64_t>(kCoverBlocks, (nr + kThreads - 1) / kThreads)), dim3(kThreads), lds, 0,
                           (const CoverNode *)m->d_cover_nodes, m->maxn, (int)m->trees.size(), tile, (const float *)rows.dX, nr, row_stride, d_cover);
        RL_HIP(hipGetLastError());
        return RL_OK;
    }, (const char *)nullptr, (char *)nullptr, 0);
    g_cb_cover_ms = rows.ms;
    if (rc) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the covers are copied as they are");
    RL_HIP(hipMemcpy(leaf.data(), d_cover, leaf.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RL_OK;
}

}  // namespace rl

extern "C" {

int rl_model_cover(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, int32_t accumulate)
{
    std::string err;
    int rc = contrib_check_rows("rl_model_cover: ", m ? (int64_t)m->trees.size() : -1, X, n_docs, row_stride, err);
    if (rc) return fail(rc, err);
    const size_t T = m->trees.size(), en = T * (size_t)m->maxn;
    const int tile = cover_tree_tile(m->maxn);
    const size_t lds = (size_t)tile * m->maxn * (sizeof(CoverNode) + 4);
    if (lds > (size_t)kContribLds) return fail(RL_ERR_UNSUPPORTED, "rl_model_cover: a tree of " + std::to_string(m->maxn) + " nodes does not fit the LDS");
    g_cb_cover_ms = 0.0;
    std::vector<uint64_t> leaf(en, 0);
    if (n_docs > 0 && (rc = cover_count(m, X, n_docs, row_stride, tile, lds, leaf))) return rc;
    const bool add = accumulate != 0 && !m->cover.empty();
    if (!add) { m->cover.assign(en, 0); m->cover_rows = 0; }
    m->value.assign(en, 0.0);
    for (size_t t = 0; t < T; t++) {
        const HostTree &h = m->trees[t];
        uint64_t *c = m->cover.data() + t * m->maxn;
        for (int j = 0; j < h.n_nodes; j++) {                              // (an inner node's sum is made again from its leaves')
            if (h.feature[j] == -1) c[j] += leaf[t * m->maxn + j];
        }
        contrib_fill_inner(h, c);
        contrib_node_values(h, c, m->value.data() + t * m->maxn);
    }
    m->cover_rows += n_docs;
    m->last_path = RL_MODEL_PATH_COVER;
    return RL_OK;
}

int rl_model_cover_rows(const rl_model *m, int64_t *n_rows)
{
    if (!m || !n_rows) return fail(RL_ERR_INVALID, "rl_model_cover_rows: null argument");
    *n_rows = m->cover_rows;
    return RL_OK;
}

int rl_model_get_cover(const rl_model *m, int32_t tree, uint64_t *count, double *value, int32_t cap, int32_t *n_nodes)
{
    static const std::string w = "rl_model_get_cover: ";
    if (!m) return fail(RL_ERR_INVALID, w + "null model");
    const int32_t T = (int32_t)m->trees.size();
    if (T < 1) return fail(RL_ERR_INVALID, w + "the model has no trees");
    if (tree < 0 || tree >= T) return fail(RL_ERR_INVALID, w + "tree = " + std::to_string(tree) + " is outside [0, " + std::to_string(T) + ")");
    const int32_t nn = m->trees[tree].n_nodes;
    if (n_nodes) *n_nodes = nn;
    if (cap < nn) return fail(RL_ERR_INVALID, w + "cap = " + std::to_string(cap) + " is below the tree's " + std::to_string(nn) + " nodes");
    if (m->cover.empty()) return fail(RL_ERR_STATE, w + "no rl_model_cover call has been made on this model");
    if (count) std::copy_n(m->cover.data() + (size_t)tree * m->maxn, nn, count);
    if (value) std::copy_n(m->value.data() + (size_t)tree * m->maxn, nn, value);
    return RL_OK;
}

int rl_model_predict_contribs(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                              int64_t scratch_bytes, double *out)
{
    static const std::string w = "rl_model_predict_contribs: ";
    std::string err;
    int rc = contrib_check_rows(w, m ? (int64_t)m->trees.size() : -1, X, n_docs, row_stride, err);
    if (!rc) rc = contrib_check_columns(w, columns, n_columns, scratch_bytes, out, err);
    if (rc) return fail(rc, err);
    if (m->cover.empty()) return fail(RL_ERR_STATE, w + "no rl_model_cover call has been made on this model");
    SlotPlan sp = slot_plan(m, columns, n_columns);
    if (!contrib_plan(m->maxn, sp.slots, sp.docs, sp.per_pass))
        return fail(RL_ERR_UNSUPPORTED, w + "a tree of " + std::to_string(m->maxn) + " nodes does not fit the LDS");
    g_cb_walk_ms = 0.0;
    g_cb_passes = sp.passes();
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    const size_t T = m->trees.size(), en = T * (size_t)m->maxn;
    std::vector<ContribNode> cn(en, ContribNode{-1, 0.f, -1, -1, 0.0, -1, 0});
    std::vector<int32_t> slot((size_t)m->maxn);
    for (size_t t = 0; t < T; t++) {
        const HostTree &h = m->trees[t];
        contrib_node_slots(h, sp.sorted, (int32_t)sp.C, slot.data());
        for (int j = 0; j < h.n_nodes; j++)
            cn[t * m->maxn + j] = ContribNode{h.feature[j], h.threshold[j], h.left[j], h.right[j], m->value[t * m->maxn + j], slot[(size_t)j], 0};
    }
    RowStream rows;
    ContribArgs a;
    memset(&a, 0, sizeof(a));
    ContribNode *d_nodes = nullptr;
    RL_HIP(rows.pool.upload(&d_nodes, cn.data(), en));
    RL_HIP(hipFuncSetAttribute((const void *)k_model_contribs, hipFuncAttributeMaxDynamicSharedMemorySize, kContribLds));
    a.nodes = d_nodes; a.w = m->d_w; a.MAXN = m->maxn; a.nt = (int)T; a.tile = contrib_tree_tile(m->maxn);
    const size_t tile_bytes = (size_t)a.tile * m->maxn * sizeof(ContribNode);
    rc = slot_stream(k_model_contribs, a, sp, X, n_docs, row_stride, scratch_bytes, out, rows,
                     [&](int ns) { return tile_bytes + (size_t)ns * (sp.docs + 1) * sizeof(double); });
    g_cb_walk_ms = rows.ms;
    if (rc) return rc;
    m->last_path = RL_MODEL_PATH_CONTRIBS;
    return RL_OK;
}

int rl_model_predict_leaf_sums(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, double *out)
{
    static const std::string w = "rl_model_predict_leaf_sums: ";
    std::string err;
    int rc = contrib_check_rows(w, m ? (int64_t)m->trees.size() : -1, X, n_docs, row_stride, err);
    if (rc) return fail(rc, err);
    if (!out) return fail(RL_ERR_INVALID, w + "null output");
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    RowStream rows;
    double *dO = nullptr;
    if ((rc = rows.open(n_docs, row_stride, 0, (int64_t)row_stride * 4 + 8))) return rc;
    RL_HIP(rows.pool.alloc(&dO, (size_t)rows.chunk));
    return rows.run(X, n_docs, row_stride, [&](int64_t nr) -> int {
        hipLaunchKernelGGL(k_model_leaf_sums, dim3((unsigned)std::min<int64_t>(8192, (nr + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, m->ens,
                           (const float *)m->d_w, m->maxn, (int)m->trees.size(), (const float *)rows.dX, nr, row_stride, dO);
        RL_HIP(hipGetLastError());
        return RL_OK;
    }, dO, out, 1);
}

int rl_debug_contrib_times(double *cover_ms, double *walk_ms)
{
    if (!cover_ms || !walk_ms) return fail(RL_ERR_INVALID, "rl_debug_contrib_times: null argument");
    *cover_ms = g_cb_cover_ms;
    *walk_ms = g_cb_walk_ms;
    return RL_OK;
}

int rl_debug_contrib_passes(int32_t *passes)
{
    if (!passes) return fail(RL_ERR_INVALID, "rl_debug_contrib_passes: null argument");
    *passes = g_cb_passes;
    return RL_OK;
}

}  // extern "C"
