// rl_stage.inc -- a tree model evaluated after every requested number of trees ("stages") in one pass over a file.  DESIGN.md 23.
// Included at the end of rl_trainer.hip, after rl_model_eval.inc (it uses rl_model, DevPool and EnsTree).
//
//   k_model_stage_scores  k_model_eval's per-document loop over a chunk of trees [t0, t1): the running float of Ensemble.eval
//                         (s = (float)(s + out * weight), Ensemble.java:110-116) is read from and written back to a carry array [n_docs],
//                         and after every tree that ends a requested stage it is stored to sc[stage in chunk][doc] -- adjacent lanes are
//                         adjacent documents, the stores are coalesced.  It walks the models the tiled kernel cannot pack; every other
//                         model is walked by k_model_eval_tiled<true> (rl_model_eval.inc), whose accumulation wavefront makes the same
//                         stores (StageWalk below; measured: the per-document walk took 2.5 x the ranking's time, DESIGN.md 23.4).
//   k_stage_eval<G, CAP>  a group of G threads owns one (list, stage): blockIdx.x goes over the lists of a length class, blockIdx.y over
//                         the chunk's stages.  The scores are floats, so the rank is counted on integer keys: a score's bits, -0.0 folded
//                         onto +0.0 (they tie: MergeSorter compares doubles), become an order-preserving uint32, and
//                             key = ord << 32 | (0xFFFFFFFF - i)
//                         makes position(i) = #{j : key[j] > key[i]} the stable descending rank -- one 64-bit unsigned compare per pair
//                         where k_eval_lists needs two f64 compares and an index compare.  +-Infinity are ordinary values.  A group
//                         that meets a NaN writes 1 to out_nan and 0.0 to the value and does not rank (the caller's host path takes the
//                         cell).  Then the group's first lane takes the metric with ev_metric (rl_eval_dev.h), the scorers k_eval_lists
//                         uses.  8 B of key + 4 B of ranked label per document is k_eval_lists' LDS footprint, so are the classes:
//                           <= kEvTiny  (16)    G = 16, 16 lists per block
//                           <= kEvWave  (256)   one wavefront per list, 4 lists per block
//                           <= kEvBlock (6144)  one block per list, 72 KiB of LDS
//                           longer              one block per list, keys and ranked labels in global scratch
//   No cross-block atomic, no spin wait: every (list, stage) cell is written by exactly one group.
//
// The host walks the stages in chunks whose float scores [stages of the chunk][n_docs] fit scratch_bytes; the carry array links the
// chunks.  Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_eval_host.h"
#include "rl_eval_dev.h"

namespace rl {

constexpr int64_t kStageScratchDefault = (int64_t)256 << 20;      // scratch_bytes == 0
constexpr int kStageMaxChunk = 65535;                             // gridDim.y

// stages: the chunk's tree counts (ascending, the last one is t1); ns of them
__global__ __launch_bounds__(kThreads) void k_model_stage_scores(const EnsTree e, const float *w, int MAXN, int t0, int t1, const int32_t *stages,
                                                                  int ns, const float *X, int64_t n, int stride, float *carry, float *sc)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = X + (size_t)i * stride;
        float s = carry[i];
        int si = 0;
        for (int t = t0; t < t1; t++) {
            const size_t o = (size_t)t * MAXN;
            int nd = 0;
            while (e.feat_idx[o + nd] != -1) {
                const int fc = e.feat_idx[o + nd];
                const float v = (fc < stride) ? row[fc] : 0.f;                 // -missingZero  DenseDataPoint.java:22-25
                nd = (v <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
            }
            s = (float)((double)s + (double)e.out[o + nd] * (double)w[t]);     // Ensemble.java:113
            if (si < ns && stages[si] == t + 1) { sc[(size_t)si * n + i] = s; si++; }
        }
        carry[i] = s;
    }
}

struct StArgs {
    EvArgs ev;                     // ideal, rd_ext, disc, metric, k, err_max for ev_metric; labels, qoff, qlist, nq for the group
    const float *sc;               // [stages of the chunk][n_docs]
    int64_t n_docs;
    unsigned long long *gkey;      // longest class: keys, [stages of the chunk][n_docs]
    float *glab;                   //                ranked labels, the same shape
    double *out; uint8_t *nan;     // [stages of the chunk][n_lists]
    int32_t n_lists;
};

__device__ __forceinline__ unsigned long long st_key(float f, int i, bool &isnan_)
{
    unsigned u = __float_as_uint(f);
    isnan_ = (u & 0x7fffffffu) > 0x7f800000u;
    if (u == 0x80000000u) u = 0u;                                   // -0.0 == 0.0: a tie, the given order decides
    const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)ord << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}

template <int G, int CAP>
__device__ void st_group(const StArgs &a, int slot, int stage, int tid, unsigned long long *s_key, float *s_lab, int *s_nan)
{
    const int q = a.ev.qlist[slot];
    const int cur = a.ev.qoff[q], n = a.ev.qoff[q + 1] - cur;
    const float *sc = a.sc + (size_t)stage * a.n_docs + cur;
    unsigned long long *key = s_key;
    float *lab = s_lab;
    if (CAP == 0) {
        key = a.gkey + (size_t)stage * a.n_docs + cur;
        lab = a.glab + (size_t)stage * a.n_docs + cur;
    }
    if (tid == 0) *s_nan = 0;
    ca_sync<G>();
    for (int i = tid; i < n; i += G) {
        bool bad;
        key[i] = st_key(sc[i], i, bad);
        if (bad) *s_nan = 1;
    }
    if (CAP == 0) __threadfence_block();
    ca_sync<G>();
    const size_t cell = (size_t)stage * a.n_lists + q;
    if (*s_nan) {
        if (tid == 0) { a.out[cell] = 0.0; a.nan[cell] = 1; }
        return;
    }
    for (int i = tid; i < n; i += G) {
        const unsigned long long v = key[i];
        int p = 0;
#pragma unroll 4
        for (int j = 0; j < n; j++) p += (key[j] > v) ? 1 : 0;
        lab[p] = a.ev.labels[cur + i];
    }
    if (CAP == 0) __threadfence_block();
    ca_sync<G>();
    if (tid == 0) { a.out[cell] = ev_metric(a.ev, q, n, lab); a.nan[cell] = 0; }
}

template <int G, int CAP>
__global__ __launch_bounds__(kThreads) void k_stage_eval(const StArgs a)
{
    constexpr int GPB = kThreads / G;                 // groups per block
    constexpr int LDS = CAP > 0 ? CAP : 1;
    __shared__ unsigned long long s_key[GPB * LDS];
    __shared__ float s_lab[GPB * LDS];
    __shared__ int s_nan[GPB];
    const int grp = threadIdx.x / G, tid = threadIdx.x % G;
    const int64_t g = (int64_t)blockIdx.x * GPB + grp;
    if (g < (int64_t)a.ev.nq) st_group<G, CAP>(a, (int)g, (int)blockIdx.y, tid, s_key + grp * LDS, s_lab + grp * LDS, s_nan + grp);   // G == kThreads: the whole block or none
}

static thread_local double g_st_walk_ms = 0.0, g_st_rank_ms = 0.0;      // the last stage call of this thread, device events

// the checks both entry points share; what names the call
static int stage_check(const char *who, const rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *stages,
                       int32_t n_stages, const void *out)
{
    const std::string w = std::string(who) + ": ";
    if (!m) return fail(RL_ERR_INVALID, w + "null model");
    if (!X) return fail(RL_ERR_INVALID, w + "null X");
    if (!stages) return fail(RL_ERR_INVALID, w + "null stages");
    if (!out) return fail(RL_ERR_INVALID, w + "null output");
    if (n_docs < 0) return fail(RL_ERR_INVALID, w + "n_docs must be >= 0");
    if (row_stride < 1) return fail(RL_ERR_INVALID, w + "row_stride must be >= 1");
    if (n_stages < 1) return fail(RL_ERR_INVALID, w + "n_stages must be >= 1");
    const int32_t T = (int32_t)m->trees.size();
    if (T < 1) return fail(RL_ERR_INVALID, w + "the model has no trees");
    for (int32_t i = 0; i < n_stages; i++) {
        if (stages[i] < 1 || stages[i] > T)
            return fail(RL_ERR_INVALID, w + "stages[" + std::to_string(i) + "] = " + std::to_string(stages[i]) + " is outside [1, " + std::to_string(T) + "]");
        if (i > 0 && stages[i] <= stages[i - 1])
            return fail(RL_ERR_INVALID, w + "stages must be strictly increasing (stages[" + std::to_string(i) + "])");
    }
    return RL_OK;
}

static int stage_chunk(int64_t scratch_bytes, int64_t bytes_per_stage, int32_t n_stages)
{
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : kStageScratchDefault;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_stages, kStageMaxChunk), budget / std::max<int64_t>(1, bytes_per_stage)));
}

// The walk of a call, chunk after chunk.  A model the tiled kernel takes (model_eval_tiled_ok) is walked by k_model_eval_tiled<true>, whose
// accumulation wavefront stores the stages: the carry then holds the sum at the last tile boundary at or before the chunk's end, and the next
// chunk walks again the (at most kEvalTreeTile - 1) trees between that boundary and its first new tree.  Every other model is walked by
// k_model_stage_scores, the carry at the chunk's last tree.
struct StageWalk {
    rl_model *m; const float *dX; int64_t n_docs; int32_t row_stride; float *d_carry, *d_sc;
    bool tiled = false; int cols = 0; size_t lds = 0;
    int carried = 0;               // trees of the model summed in d_carry (tiled: a multiple of kEvalTreeTile)
    StageWalk(rl_model *m_, const float *dX_, int64_t n, int32_t stride, float *carry, float *sc)
        : m(m_), dX(dX_), n_docs(n), row_stride(stride), d_carry(carry), d_sc(sc) { tiled = model_eval_tiled_ok(m, row_stride, cols, lds); }
    // the chunk's stages (device pointer, ns of them), the last of which is t1
    void launch(const int32_t *d_stages, int ns, int t1)
    {
        if (tiled) {
            const int T0 = carried, B = t1 / kEvalTreeTile * kEvalTreeTile;
            const EvalStage st{d_stages, ns, T0, B > T0 ? B : -1, d_carry, d_sc};
            const int64_t tiles = (n_docs + kEvalDocs - 1) / kEvalDocs;
            hipLaunchKernelGGL(k_model_eval_tiled<true>, dim3((unsigned)std::min<int64_t>(tiles, 256 * 256)), dim3(kEvalThreads), lds, 0,
                               (const unsigned long long *)m->d_pack + (size_t)T0 * m->maxn, (const float *)m->d_w + T0, m->maxn, t1 - T0, dX, n_docs,
                               row_stride, cols, (float *)nullptr, (const unsigned char *)m->d_perm + T0,
                               (const unsigned char *)m->d_gdepth + (size_t)(T0 / kEvalTreeTile) * kEvalMetaDepths, st);
            if (B > T0) carried = B;
            m->last_path = RL_MODEL_PATH_TILED;
        } else {
            hipLaunchKernelGGL(k_model_stage_scores, dim3((unsigned)std::min<int64_t>(8192, (n_docs + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0,
                               m->ens, (const float *)m->d_w, m->maxn, carried, t1, d_stages, ns, dX, n_docs, row_stride, d_carry, d_sc);
            carried = t1;
            m->last_path = RL_MODEL_PATH_GENERIC;
        }
    }
};

// The ranking half of a call: the lists by length class, the scorer's tables on the device and the four-class launch of k_stage_eval over
// the `ns` score rows of a chunk -- stages for rl_model_eval_stages, permuted cells for rl_model_eval_permuted (rl_permimp.inc).
struct StageRank {
    std::vector<int32_t> lists[4];
    int32_t *d_qlist[4] = {nullptr, nullptr, nullptr, nullptr};
    StArgs a;
    StageRank() { memset(&a, 0, sizeof(a)); }
    void classify(const int32_t *qoff, int32_t n_lists)
    {
        for (int32_t q = 0; q < n_lists; q++) {
            const int n = qoff[q + 1] - qoff[q];
            lists[n <= kEvTiny ? 0 : n <= kEvWave ? 1 : n <= kEvBlock ? 2 : 3].push_back(q);
        }
    }
    // scratch of one score row: its floats, and where a list is past the LDS class its keys and ranked labels as well
    int64_t bytes_per_row(int64_t n_docs) const
    {
        return n_docs * (int64_t)(sizeof(float) + (lists[3].empty() ? 0 : sizeof(unsigned long long) + sizeof(float)));
    }
    // d_sc: [chunk][n_docs], the rows the walk writes.  Allocates the outputs [chunk][n_lists] (a.out, a.nan).
    int upload(DevPool &pool, const float *d_sc, int chunk, const float *labels, int64_t n_docs, const int32_t *qoff, int32_t n_lists,
               const std::vector<double> &ideal, const std::vector<double> &disc, const int32_t *rel_doc_count, int32_t metric, int32_t k,
               double err_max)
    {
        float *d_lab = nullptr;
        double *d_ideal = nullptr, *d_disc = nullptr;
        int32_t *d_qoff = nullptr, *d_rd = nullptr;
        RL_HIP(pool.upload(&d_lab, labels, (size_t)n_docs));
        RL_HIP(pool.upload(&d_qoff, qoff, (size_t)n_lists + 1));
        RL_HIP(pool.upload(&d_ideal, ideal.data(), (size_t)n_lists));
        RL_HIP(pool.upload(&d_disc, disc.data(), disc.size()));
        RL_HIP(pool.alloc(&a.out, (size_t)chunk * n_lists));
        RL_HIP(pool.alloc(&a.nan, (size_t)chunk * n_lists));
        if (!lists[3].empty()) { RL_HIP(pool.alloc(&a.gkey, (size_t)chunk * n_docs)); RL_HIP(pool.alloc(&a.glab, (size_t)chunk * n_docs)); }
        if (rel_doc_count) RL_HIP(pool.upload(&d_rd, rel_doc_count, (size_t)n_lists));
        for (int c = 0; c < 4; c++)
            if (!lists[c].empty()) RL_HIP(pool.upload(&d_qlist[c], lists[c].data(), lists[c].size()));
        a.ev.labels = d_lab; a.ev.qoff = d_qoff; a.ev.ideal = d_ideal; a.ev.rd_ext = d_rd; a.ev.disc = d_disc;
        a.ev.metric = metric; a.ev.k = k; a.ev.err_max = err_max;
        a.sc = d_sc; a.n_docs = n_docs; a.n_lists = n_lists;
        return RL_OK;
    }
    // every list of every length class under the first ns score rows
    int launch(int ns)
    {
        static const int G[4] = {kEvTiny, kWave, kThreads, kThreads};
        for (int c = 0; c < 4; c++) {
            if (lists[c].empty()) continue;
            a.ev.qlist = d_qlist[c]; a.ev.nq = (int32_t)lists[c].size();
            const int gpb = kThreads / G[c];
            const dim3 grid((unsigned)((a.ev.nq + gpb - 1) / gpb), (unsigned)ns), block(kThreads);
            if (c == 0) hipLaunchKernelGGL((k_stage_eval<kEvTiny, kEvTiny>), grid, block, 0, 0, a);
            else if (c == 1) hipLaunchKernelGGL((k_stage_eval<kWave, kEvWave>), grid, block, 0, 0, a);
            else if (c == 2) hipLaunchKernelGGL((k_stage_eval<kThreads, kEvBlock>), grid, block, 0, 0, a);
            else hipLaunchKernelGGL((k_stage_eval<kThreads, 0>), grid, block, 0, 0, a);
            RL_HIP(hipGetLastError());
        }
        return RL_OK;
    }
};

struct StageEvents {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    hipError_t create() { for (auto &x : e) { hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; } return hipSuccess; }
    ~StageEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

}  // namespace rl

extern "C" {

int rl_model_predict_stages(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *stages, int32_t n_stages, float *out)
{
    int rc = stage_check("rl_model_predict_stages", m, X, n_docs, row_stride, stages, n_stages, out);
    if (rc) return rc;
    g_st_walk_ms = g_st_rank_ms = 0.0;
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    DevPool pool;
    float *dX = nullptr, *d_carry = nullptr, *d_sc = nullptr; int32_t *d_stages = nullptr;
    const int chunk = stage_chunk(0, n_docs * (int64_t)sizeof(float), n_stages);
    RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
    RL_HIP(pool.alloc(&d_carry, (size_t)n_docs));
    RL_HIP(pool.alloc(&d_sc, (size_t)chunk * n_docs));
    RL_HIP(pool.upload(&d_stages, stages, (size_t)n_stages));
    RL_HIP(hipMemset(d_carry, 0, (size_t)n_docs * sizeof(float)));
    StageEvents ev;
    RL_HIP(ev.create());
    StageWalk walk(m, dX, n_docs, row_stride, d_carry, d_sc);
    for (int s0 = 0; s0 < n_stages; s0 += chunk) {
        const int ns = std::min(chunk, n_stages - s0);
        RL_HIP(hipEventRecord(ev.e[0], 0));
        walk.launch(d_stages + s0, ns, stages[s0 + ns - 1]);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        RL_HIP(hipMemcpy(out + (size_t)s0 * n_docs, d_sc, (size_t)ns * n_docs * sizeof(float), hipMemcpyDeviceToHost));
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_st_walk_ms += (double)ms;
    }
    return RL_OK;
}

int rl_model_eval_stages(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const float *labels, const int32_t *qoff,
                         int32_t n_lists, const int32_t *qkey, const double *ideal_dcg, const int32_t *rel_doc_count, int32_t metric, int32_t k,
                         double err_max, const int32_t *stages, int32_t n_stages, int64_t scratch_bytes, double *out_metric, uint8_t *out_nan,
                         double *out_ideal)
{
    static const char *who = "rl_model_eval_stages";
    int rc = stage_check(who, m, X, n_docs, row_stride, stages, n_stages, out_metric);
    if (rc) return rc;
    if (!out_nan) return fail(RL_ERR_INVALID, std::string(who) + ": null out_nan");
    if (scratch_bytes < 0) return fail(RL_ERR_INVALID, std::string(who) + ": scratch_bytes must be >= 0");
    std::vector<double> ideal, disc;
    std::string err;
    rc = eval_prepare_lists(who, metric, k, err_max, nullptr, labels, n_docs, qoff, n_lists, qkey, ideal_dcg, rel_doc_count, out_metric, ideal,
                            disc, err);
    if (rc) return fail(rc, err);
    g_st_walk_ms = g_st_rank_ms = 0.0;
    RL_HIP(hipSetDevice(m->device));
    StageRank rank;
    rank.classify(qoff, n_lists);
    // a stage of the chunk: its float scores, and where a list is past the LDS class its keys and ranked labels as well
    const int chunk = stage_chunk(scratch_bytes, rank.bytes_per_row(n_docs), n_stages);
    DevPool pool;
    float *dX = nullptr, *d_carry = nullptr, *d_sc = nullptr;
    int32_t *d_stages = nullptr;
    RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
    RL_HIP(pool.alloc(&d_carry, (size_t)n_docs));
    RL_HIP(pool.alloc(&d_sc, (size_t)chunk * n_docs));
    RL_HIP(pool.upload(&d_stages, stages, (size_t)n_stages));
    RL_HIP(hipMemset(d_carry, 0, (size_t)n_docs * sizeof(float)));
    rc = rank.upload(pool, d_sc, chunk, labels, n_docs, qoff, n_lists, ideal, disc, rel_doc_count, metric, k, err_max);
    if (rc) return rc;
    StageEvents ev;
    RL_HIP(ev.create());
    StageWalk walk(m, dX, n_docs, row_stride, d_carry, d_sc);
    for (int s0 = 0; s0 < n_stages; s0 += chunk) {
        const int ns = std::min(chunk, n_stages - s0);
        RL_HIP(hipEventRecord(ev.e[0], 0));
        walk.launch(d_stages + s0, ns, stages[s0 + ns - 1]);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        rc = rank.launch(ns);
        if (rc) return rc;
        RL_HIP(hipEventRecord(ev.e[2], 0));
        RL_HIP(hipMemcpy(out_metric + (size_t)s0 * n_lists, rank.a.out, (size_t)ns * n_lists * sizeof(double), hipMemcpyDeviceToHost));
        RL_HIP(hipMemcpy(out_nan + (size_t)s0 * n_lists, rank.a.nan, (size_t)ns * n_lists, hipMemcpyDeviceToHost));
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_st_walk_ms += (double)ms;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
        g_st_rank_ms += (double)ms;
    }
    if (out_ideal) std::copy(ideal.begin(), ideal.end(), out_ideal);
    return RL_OK;
}

int rl_debug_stage_times(double *walk_ms, double *rank_ms)
{
    if (!walk_ms || !rank_ms) return fail(RL_ERR_INVALID, "rl_debug_stage_times: null argument");
    *walk_ms = g_st_walk_ms;
    *rank_ms = g_st_rank_ms;
    return RL_OK;
}

}  // extern "C"
