// rl_k_leaf.inc -- K7 and K8: the leaves of the grown tree, their outputs, the score update and the metric's mean (LambdaMART.java:398-415,
// 203-210, 469-483; MART.java:54-65; metric/MetricScorer.java:46-52).  k_leaf_table, k_leaf_output, k_metric_finish, k_leaf_chain, k_score_update,
// k_score_stream, k_float_mean, k_double_mean.  The exact parallel form of the float sums is rl_chain.inc; its host side is rl_chain_host.inc.
// Included by rl_kernels_round.inc; needs rl_chain.inc (ChainBufs and its plan), nothing of rl_kernels_round.inc and none of the other pieces.

namespace rl {

// ------------------------------------------------------------------------------------------------
// K7: leaves.  k_leaf_table lists the leaves in ascending `start` == left-first DFS order
// (Split.leaves, Split.java:100-113): a left child always owns the front part of its parent's range.
// ------------------------------------------------------------------------------------------------
constexpr int kLeafTableCap = 1024;      // node records staged in LDS by k_leaf_table

__global__ __launch_bounds__(kThreads) void k_leaf_table(const Ctx c, const ChainBufs cb, int32_t *seg_buf)
{
    __shared__ int s_left[kLeafTableCap], s_right[kLeafTableCap], s_start[kLeafTableCap], s_buf[kLeafTableCap], s_stack[kLeafTableCap];
    TreeState *st = c.st;
    if (threadIdx.x == 0 && c.grow_docs[8] != 0ull) {       // RL_ARR_BUBBLES: device time between the bookkeeping that ended the tree and this launch
        const unsigned long long now = wall_clock64();
        c.grow_docs[4] += now - c.grow_docs[8]; c.grow_docs[5] += 1ull; c.grow_docs[8] = 0ull;
    }
    const int nn = st->n_nodes;
    if (nn <= kLeafTableCap) {
        // the walk is a chain of dependent reads: stage the few fields it needs in LDS first (one round trip to memory)
        for (int x = threadIdx.x; x < nn; x += kThreads) {
            const NodeRec &X = c.nodes[x];
            s_left[x] = X.left; s_right[x] = X.right; s_start[x] = X.start; s_buf[x] = X.buf;
        }
        __syncthreads();
        if (threadIdx.x != 0) return;
        // pre-order walk, left first; the chain plan (one segment per leaf, rl_chain.inc) is written as the leaves appear
        int n = 0, sp = 0, tiles = 0, prev = 0;
        s_stack[sp++] = 0;
        while (sp > 0) {
            const int x = s_stack[--sp];
            if (s_left[x] < 0) {
                const int start = s_start[x];
                if (n > 0) tiles += (start - prev + kChainTile - 1) / kChainTile;
                c.leaf_node[n] = x; c.leaf_start[n] = start;
                cb.seg_start[n] = start; cb.seg_tile0[n] = tiles;
                seg_buf[n] = (x == 0) ? -1 : s_buf[x];
                prev = start; n++;
            } else { s_stack[sp++] = s_right[x]; s_stack[sp++] = s_left[x]; }      // depth <= splits < nn
        }
        if (n > 0) tiles += (c.N - prev + kChainTile - 1) / kChainTile;
        for (int i = n; i <= c.L + 1; i++) c.leaf_start[i] = c.N;      // unused leaf slots are empty segments
        st->n_leaves = n;
        cb.seg_start[n] = c.N; cb.seg_tile0[n] = tiles;
        cb.plan->n_seg = n; cb.plan->n = c.N; cb.plan->n_tiles = tiles; cb.plan->n_chunks = tiles + n;
        return;
    }
    if (threadIdx.x != 0) return;
    // very large trees: insertion sort of all leaves by start, straight from memory
    int n = 0;
    for (int x = 0; x < nn; x++) if (c.nodes[x].left < 0 && c.nodes[x].fid >= 0) {
        int i = n++;
        while (i > 0 && c.leaf_start[i - 1] > c.nodes[x].start) { c.leaf_start[i] = c.leaf_start[i - 1]; c.leaf_node[i] = c.leaf_node[i - 1]; i--; }
        c.leaf_start[i] = c.nodes[x].start; c.leaf_node[i] = x;
    }
    for (int i = n; i <= c.L + 1; i++) c.leaf_start[i] = c.N;
    st->n_leaves = n;
    int tiles = 0;
    for (int i = 0; i < n; i++) {
        cb.seg_start[i] = c.leaf_start[i];
        cb.seg_tile0[i] = tiles;
        tiles += (c.leaf_start[i + 1] - c.leaf_start[i] + kChainTile - 1) / kChainTile;
        seg_buf[i] = (c.leaf_node[i] == 0) ? -1 : c.nodes[c.leaf_node[i]].buf;
    }
    cb.seg_start[n] = c.N; cb.seg_tile0[n] = tiles;
    cb.plan->n_seg = n; cb.plan->n = c.N; cb.plan->n_tiles = tiles; cb.plan->n_chunks = tiles + n;
}

// leaf output = s1 / s2 in float, 0 when s2 == 0   (LambdaMART.java:409-413)
__global__ __launch_bounds__(kThreads) void k_leaf_output(const Ctx c, const ChainBufs cb)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && cb.stats[3] != 0) {       // RL_ARR_BUBBLES: device time since the chain's last stitch pass ended (10 ns units, 32 bits)
        c.grow_docs[6] += (unsigned long long)(unsigned)((int)wall_clock64() - cb.stats[3]); c.grow_docs[7] += 1ull; cb.stats[3] = 0;
    }
    const int li = blockIdx.x * kThreads + threadIdx.x;
    if (li >= c.st->n_leaves) return;
    const float s1 = cb.result[li], s2 = cb.result[cb.maxseg + li];
    NodeRec &X = c.nodes[c.leaf_node[li]];
    if (c.mart) X.output = s1 / (float)X.gcount;                  // MART.updateTreeOutput (MART.java:54-65): float sum / int count
    else X.output = (s2 == 0.f) ? 0.f : s1 / s2;
}

__global__ void k_metric_finish(const ChainBufs cb, int n, float *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = cb.result[0] / (float)n;    // LambdaMART.java:470
}

// one wavefront per leaf: the two Java float running sums, element by element, in sample order
// (LambdaMART.java:401-413).  64 samples are fetched in parallel, then chained through readlane.
__global__ __launch_bounds__(64) void k_leaf_chain(const Ctx c)
{
    const TreeState *st = c.st;
    const int li = blockIdx.x;
    if (li >= st->n_leaves) return;
    const int node = c.leaf_node[li];
    NodeRec &X = c.nodes[node];
    const bool root = (node == 0);
    const int *idx = root ? nullptr : c.idx[X.buf] + X.start;
    const int cnt = X.count;
    float s1 = 0.f, s2 = 0.f;
    for (int base = 0; base < cnt; base += 64) {
        const int i = base + lane_id();
        double x1 = 0.0, x2 = 0.0;
        if (i < cnt) { const int k = root ? i : idx[i]; const double2 v = c.lw[k]; x1 = v.x; x2 = v.y; }
        const int m = min(64, cnt - base);
        const uint32_t a0 = (uint32_t)d2bits(x1), a1 = (uint32_t)(d2bits(x1) >> 32);
        const uint32_t b0 = (uint32_t)d2bits(x2), b1 = (uint32_t)(d2bits(x2) >> 32);
#pragma unroll
        for (int j = 0; j < 64; j++) {
            if (j < m) {
                const uint64_t ua = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)a1, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)a0, j);
                const uint64_t ub = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)b1, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)b0, j);
                s1 = float_chain_step(s1, bits2d(ua));
                s2 = float_chain_step(s2, bits2d(ub));
            }
        }
    }
    if (lane_id() == 0) X.output = c.mart ? s1 / (float)X.gcount : ((s2 == 0.f) ? 0.f : s1 / s2);     // :409-413 / MART.java:64
}

// A block takes runs of kScoreBatch x kThreads consecutive leaf-order positions: the leaf of a position is a search in the LDS copy of the leaf
// table, whose entries carry the list buffer and the step lr * output of the leaf (no dependent load of the node record), and the kScoreBatch
// document ids, then the kScoreBatch scores, of a thread are requested together (unconditional loads from clamped positions: a load inside a
// per-lane condition is completed before the next one is issued).
constexpr int kScoreBatch = 4;
__global__ __launch_bounds__(kThreads) void k_score_update(const Ctx c)
{
    __shared__ int s_start[1024 + 1];
    __shared__ int s_buf[1024];
    __shared__ double s_step[1024];
    const TreeState *st = c.st;
    const int nl = st->n_leaves;
    const bool use_lds = nl <= 1024;
    if (use_lds) {
        for (int i = threadIdx.x; i <= nl; i += kThreads) s_start[i] = c.leaf_start[i];
        for (int i = threadIdx.x; i < nl; i += kThreads) {
            const int node = c.leaf_node[i];
            const NodeRec &X = c.nodes[node];
            s_buf[i] = (node == 0) ? -1 : X.buf;
            s_step[i] = (double)c.lr * (double)X.output;                  // LambdaMART.java:208
        }
        __syncthreads();
    }
    const int N = c.N;
    if (!use_lds) {
        for (int p = blockIdx.x * kThreads + threadIdx.x; p < N; p += gridDim.x * kThreads) {
            int lo = 0, hi = nl - 1;                       // last leaf with start <= p
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (c.leaf_start[mid] <= p) lo = mid; else hi = mid - 1; }
            const int node = c.leaf_node[lo];
            const NodeRec &X = c.nodes[node];
            const int k = (node == 0) ? p : c.idx[X.buf][p];
            c.scores[k] += (double)c.lr * (double)X.output;
        }
        return;
    }
    constexpr int RUN = kScoreBatch * kThreads;
    for (int base = blockIdx.x * RUN; base < N; base += gridDim.x * RUN) {
        int p[kScoreBatch], k[kScoreBatch]; double step[kScoreBatch], sc[kScoreBatch];
        int buf[kScoreBatch];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) {
            p[u] = min(base + u * kThreads + (int)threadIdx.x, N - 1);
            int lo = 0, hi = nl - 1;                       // last leaf with start <= p
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_start[mid] <= p[u]) lo = mid; else hi = mid - 1; }
            buf[u] = s_buf[lo]; step[u] = s_step[lo];
        }
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) k[u] = c.idx[max(buf[u], 0)][p[u]];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) { if (buf[u] < 0) k[u] = p[u]; }
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) sc[u] = c.scores[k[u]];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++)
            if (base + u * kThreads + (int)threadIdx.x < N) c.scores[k[u]] = sc[u] + step[u];
    }
}

// The same update as a stream over the documents: the leaf of every document was left behind by the gather of the leaf sums (ChainSource::seg_of),
// so a document costs one 2-byte and one 8-byte coalesced read and one coalesced write -- through the leaves' lists every document is an 8-byte
// read-modify-write at a random address, a memory sector each way (68 -> ~20 us at 3.77 M documents).  modelScores[k] += learningRate * output
// (LambdaMART.java:203-210), the same double product.
__global__ __launch_bounds__(kThreads) void k_score_stream(const Ctx c)
{
    __shared__ double s_step[1024];
    const TreeState *st = c.st;
    const int nl = st->n_leaves;
    for (int i = threadIdx.x; i < nl; i += kThreads) s_step[i] = (double)c.lr * (double)c.nodes[c.leaf_node[i]].output;                  // LambdaMART.java:208
    __syncthreads();
    const int N = c.N;
    constexpr int RUN = kScoreBatch * kThreads;
    for (int base = blockIdx.x * RUN; base < N; base += gridDim.x * RUN) {
        int k[kScoreBatch]; unsigned short lf[kScoreBatch]; double sc[kScoreBatch];
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++) { k[u] = min(base + u * kThreads + (int)threadIdx.x, N - 1); lf[u] = c.leaf_of[k[u]]; sc[u] = c.scores[k[u]]; }
#pragma unroll
        for (int u = 0; u < kScoreBatch; u++)
            if (base + u * kThreads + (int)threadIdx.x < N) c.scores[k[u]] = sc[u] + s_step[min((int)lf[u], 1023)];
    }
}

// ------------------------------------------------------------------------------------------------
// K8: per-round metric: NDCG per query comes from k_rank_*, the float running mean is below / in rl_chain.inc
// ------------------------------------------------------------------------------------------------
// float s = 0; for q: s += score_q; s / Q      (LambdaMART.java:469-471,474-483)
__global__ __launch_bounds__(64) void k_float_mean(const double *v, int n, float *out)
{
    float s = 0.f;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane_id();
        const double x = (i < n) ? v[i] : 0.0;
        const uint32_t a0 = (uint32_t)d2bits(x), a1 = (uint32_t)(d2bits(x) >> 32);
        const int m = min(64, n - base);
#pragma unroll
        for (int j = 0; j < 64; j++) {
            if (j < m) {
                const uint64_t ua = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)a1, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)a0, j);
                s = float_chain_step(s, bits2d(ua));
            }
        }
    }
    if (lane_id() == 0) *out = s / (float)n;
}

// double mean in list order  (MetricScorer.score(List), metric/MetricScorer.java:46-52)
__global__ __launch_bounds__(64) void k_double_mean(const double *v, int n, double *out)
{
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n; i++) s += v[i];
    *out = s / n;
}

}  // namespace rl
