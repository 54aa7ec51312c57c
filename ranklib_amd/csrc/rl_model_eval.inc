// rl_model_eval.inc -- the scoring-only model: an ensemble loaded from RankLib model text, its two evaluation kernels and the rl_model_* ABI.
// Included at the end of rl_trainer.hip (it uses DevPool, EnsTree and HostTree).  Which models the tiled kernel takes and the
// packed format it walks are stated in rl_eval_pack_host.h, host only; rl_model_from_text uploads what eval_pack returns.
#include "rl_eval_pack_host.h"

struct rl_model {
    int32_t device = 0;
    std::vector<HostTree> trees;
    std::vector<int32_t> features;
    int32_t maxn = 1;
    DevPool pool;
    EnsTree ens;
    float *d_w = nullptr;
    unsigned long long *d_pack = nullptr;   // packed nodes for k_model_eval_tiled (null when the model does not fit the packing)
    unsigned char *d_perm = nullptr;        // EvalPack::perm [tiles][kEvalTreeTile]: chain u of walker p walks tree perm[p * kEvalPer + u] of the tile (255 = none); the tile's trees by descending depth, dealt round the walkers
    unsigned char *d_gdepth = nullptr;      // EvalPack::meta [tiles][kEvalMetaDepths]: every walker's steps (its deepest tree), then per walker the steps at which its phases end
    int32_t maxcol = 0;                     // largest column any node reads
    EvalKnobs knobs;                        // RLHIP_EVAL_*, read by rl_model_from_text
    int32_t last_path = RL_MODEL_PATH_NONE; // the kernel the last predict call took (rl_model_debug_path)
    // contributions (rl_contrib.inc): the background's covers and the node values made from them, [trees][maxn]; empty before rl_model_cover
    std::vector<uint64_t> cover;
    std::vector<double> value;
    int64_t cover_rows = 0;
    void *d_cover_nodes = nullptr;          // the trees as k_model_cover stages them (made by the first rl_model_cover call)
};

namespace rl {
// like k_ensemble_eval but with a weight per tree (Ensemble.weights)
__global__ __launch_bounds__(kThreads) void k_model_eval(const EnsTree e, const float *w, int MAXN, int nt, const float *X, int64_t n,
                                                          int stride, float *out)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = X + (size_t)i * stride;
        float s = 0.f;
        for (int t = 0; t < nt; t++) {
            const size_t o = (size_t)t * MAXN;
            int nd = 0;
            while (e.feat_idx[o + nd] != -1) {
                const int fc = e.feat_idx[o + nd];
                const float v = (fc < stride) ? row[fc] : 0.f;                 // -missingZero  DenseDataPoint.java:22-25
                nd = (v <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
            }
            s = (float)((double)s + (double)e.out[o + nd] * (double)w[t]);     // Ensemble.java:113
        }
        out[i] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// K10 (SURVEY.md 8f-1, config c4): Ensemble.eval for many trees.  One block scores a tile of kEvalDocs documents against
// the whole ensemble:
//   * the tile's feature rows are transposed into LDS once, sX[column][doc] (columns the rows do not have are zero:
//     -missingZero): a lane reads sX[c * kEvalDocs + doc], so the bank is doc % 32 whatever column the lane's path asks
//     for -- conflict-free;
//   * trees stream through LDS in tiles of kEvalTreeTile as packed 8-byte nodes, children adjacent (right = left + 1):
//       bits 0..31 threshold (or leaf output) float bits | 32..47 byte offset of the column in sX (0: a leaf, see the walk below)
//       | 48..63 byte offset of the left child in the tree
//     so a step is: load node, load value, compare, add -- 7 VALU + 2 LDS instructions;
//   * walker wavefront p (of kEvalParts) owns the kEvalPer trees perm[p*kEvalPer .. (p+1)*kEvalPer) of the tile for all documents: kEvalPer
//     chains per lane in lockstep (a leaf is a fixed point of the step, so finished trees idle in place).  The walk is
//     bound by instruction issue (13 per chain step), not by LDS latency.  Measured and dropped: refilling a finished chain
//     with the lane's next tree (fewer steps, but a leaf branch that some lane takes at almost every step: 8.2 M docs/s
//     against 14.8), and a branch-free step with all value loads issued first (22 instructions per step: 9.7 M docs/s);
//   * one more wavefront does nothing but Ensemble.eval's accumulation  s = (float)(s + out * weight)  in tree order
//     (learning/tree/Ensemble.java:110-116) for the PREVIOUS tile (leaf outputs double-buffered in LDS), so the serial
//     float chain of a document overlaps the walk of the next tile instead of stalling the walkers;
//   * the next tile of trees is fetched into registers while the current one is walked.
// Needs: column offsets and child offsets that fit 16 bits, and the LDS budget; otherwise k_model_eval runs.
// ------------------------------------------------------------------------------------------------
// (the tile constants, eval_tiled_lds and the packed format itself: rl_eval_pack_host.h)
//
// The walk (round 4).  A leaf is packed as a node that loops onto itself: it "reads" column 0 -- no RankLib feature has id 0; the staged tile holds
// -infinity there -- so `x <= value` is always true and its left-child offset is its own.  A chain step is then the same eight instructions for
// every node (and, add, ds_read_b32, shift, compare, select, add3, ds_read_b64) with no leaf test and no branch, so the compiler issues the eight
// chains' feature loads back to back and their node loads back to back: the wavefront waits for LDS twice per step of EIGHT chains instead of
// twice per chain (the branchy version spent half of its time in those waits: 2.5 walker wavefronts per SIMD cannot hide them).  The trees of a
// tile, sorted by depth, are dealt round the walkers (perm / gdepth, built with the packing), deepest first inside a walker; a walker's deepest tree sets its
// number of steps, and since round 6 its chains drop out in phases as their trees end -- eight chains to the 7th tree's depth, six to the 5th's, four to the
// 3rd's, two to the deepest's (see kEvalPhases) -- instead of all eight idling on their leaves to the last step: 26.8 -> 28.4 M docs/s.  The accumulator
// adds the outputs in the ensemble's own order whatever walker produced them.
//
// STAGED (rl_stage.inc, DESIGN.md 23): the same walk over the trees [tbase, tbase + nt) of the model, tbase a multiple of the tile; only the
// accumulation wavefront differs.  Its running sum starts from carry[doc] (the model's first tbase trees), it stores the sum to
// sc[stage][doc] after every tree that ends one of the `ns` requested stages, and to carry[doc] after tree carry_at (a tile boundary, or -1).
struct EvalStage {
    const int32_t *stages; int32_t ns, tbase, carry_at;
    float *carry, *sc;
};

// the accumulation of one walked tile: cnt trees whose outputs are at po[tree * kEvalDocs], the first of them tree tglob of the model
template <bool STAGED>
__device__ __forceinline__ void eval_accumulate(float &s, const float *po, const float *pw, int cnt, int tglob, const EvalStage &st, int &si,
                                                int64_t n, int64_t di)
{
    for (int t = 0; t < cnt; t++) {
        s = (float)((double)s + (double)po[t * kEvalDocs] * (double)pw[t]);   // Ensemble.java:113
        if (STAGED) {
            const int done = tglob + t + 1;                                    // trees of the model summed in s
            if (si < st.ns && st.stages[si] == done) { st.sc[(size_t)si * n + di] = s; si++; }
            if (done == st.carry_at) st.carry[di] = s;
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(kEvalThreads) void k_model_eval_tiled(const unsigned long long *nodes, const float *w, int MAXN, int nt,
                                                                   const float *X, int64_t n, int stride, int cols, float *out,
                                                                   const unsigned char *perm, const unsigned char *gdepth, const EvalStage st)
{
    extern __shared__ unsigned char ev_raw[];
    float *sX = (float *)ev_raw;                                               // [cols][kEvalDocs]
    unsigned long long *sT = (unsigned long long *)(sX + (size_t)cols * kEvalDocs);   // [kEvalTreeTile][MAXN]
    float *sO = (float *)(sT + (size_t)kEvalTreeTile * MAXN);                  // [2][kEvalTreeTile][kEvalDocs] leaf outputs (double buffer)
    float *sW = sO + 2 * kEvalTreeTile * kEvalDocs;                            // [2][kEvalTreeTile] tree weights
    unsigned char *sP = (unsigned char *)(sW + 2 * kEvalTreeTile);             // [2][kEvalTreeTile + kEvalMetaDepths] the tile's walker assignment and walk lengths
    const int tid = threadIdx.x, doc = tid & (kEvalDocs - 1), part = tid / kEvalDocs;
    const bool walker = part < kEvalParts;
    const int tile_words = kEvalTreeTile * MAXN;                               // <= kEvalThreads * kEvalPrefetch (checked by the host)
    const unsigned char *sXb = (const unsigned char *)sX + doc * 4;
    for (int64_t tile = blockIdx.x; tile * kEvalDocs < n; tile += gridDim.x) {
        const int64_t d0 = tile * kEvalDocs;
        const int nd = (int)min((int64_t)kEvalDocs, n - d0);
        __syncthreads();
        const float *src = X + (size_t)d0 * stride;                            // the tile is one contiguous range of X
        for (int e = tid; e < nd * stride; e += kEvalThreads) { const int dd = e / stride, c = e - dd * stride; sX[c * kEvalDocs + dd] = src[e]; }
        for (int e = tid; e < (cols - stride) * kEvalDocs; e += kEvalThreads) sX[stride * kEvalDocs + e] = 0.f;
        float s = 0.f;                                                         // the accumulator wavefront's running Ensemble.eval sum
        [[maybe_unused]] int si = 0;                                           // STAGED: the next requested stage
        if (STAGED) { if (!walker && doc < nd) s = st.carry[d0 + doc]; }
        unsigned long long pre[kEvalPrefetch];
#pragma unroll
        for (int u = 0; u < kEvalPrefetch; u++) { const int e = tid + u * kEvalThreads; pre[u] = (e < min(tile_words, nt * MAXN)) ? nodes[e] : 0ull; }
        __syncthreads();
        if (tid < kEvalDocs) sX[tid] = -__builtin_inff();                      // column 0: what a leaf "reads" (after the staging pass wrote the rows' column 0)
        int k = 0, tt_prev = 0;
        for (int t0 = 0; t0 < nt; t0 += kEvalTreeTile, k++) {
            const int tt = min(kEvalTreeTile, nt - t0);
            const int cb = k & 1;
            __syncthreads();                                                   // tile k-1 walked (its outputs complete), sT free
#pragma unroll
            for (int u = 0; u < kEvalPrefetch; u++) { const int e = tid + u * kEvalThreads; if (e < tile_words) sT[e] = pre[u]; }
            if (tid < tt) sW[cb * kEvalTreeTile + tid] = w[t0 + tid];
            if (tid < kEvalTreeTile) sP[cb * (kEvalTreeTile + kEvalMetaDepths) + tid] = perm[(size_t)k * kEvalTreeTile + tid];
            else if (tid < kEvalTreeTile + kEvalMetaDepths) sP[cb * (kEvalTreeTile + kEvalMetaDepths) + tid] = gdepth[(size_t)k * kEvalMetaDepths + (tid - kEvalTreeTile)];
            __syncthreads();
            {   // next tile -> registers (in flight during the walk)
                const size_t nb = (size_t)(t0 + kEvalTreeTile) * MAXN;
                const long long left = (long long)nt * MAXN - (long long)nb;
#pragma unroll
                for (int u = 0; u < kEvalPrefetch; u++) { const int e = tid + u * kEvalThreads; pre[u] = (e < tile_words && e < left) ? nodes[nb + e] : 0ull; }
            }
            if (walker) {
                const unsigned char *pp = sP + cb * (kEvalTreeTile + kEvalMetaDepths);
                const int depth = __builtin_amdgcn_readfirstlane((int)pp[kEvalTreeTile + part]);      // wave-uniform: a scalar loop bound
                if (depth > 0) {
                    float *so = sO + (size_t)cb * kEvalTreeTile * kEvalDocs + doc;
                    const unsigned char *tb[kEvalPer];
                    unsigned long long v[kEvalPer];
                    int li[kEvalPer];
#pragma unroll
                    for (int u = 0; u < kEvalPer; u++) {
                        li[u] = __builtin_amdgcn_readfirstlane((int)pp[part * kEvalPer + u]);         // 255: no such tree in this (last) tile -- the chain walks tree 0 again, unstored
                        tb[u] = (const unsigned char *)(sT + (size_t)(li[u] < tt ? li[u] : 0) * MAXN);
                        v[u] = *(const unsigned long long *)tb[u];
                    }
                    // The walker's trees come deepest first.  All eight chains walk for as many steps as the walker's (kEvalPh1 + 1)-th tree has levels, then the
                    // kEvalPh1 deepest for as many as the (kEvalPh2 + 1)-th has, ... : a chain that has reached its leaf in every lane stops costing instructions
                    // (in ONE loop to the deepest tree's depth the shallow chains idled on their leaves, at the cost of their instructions).
                    int step = 0;
#define RL_EVAL_PHASE(NCH, UNTIL)                                                                                                          \
                    for (; step < (UNTIL); step++) {                                                                                       \
                        float x[NCH];                                                                                                      \
                        _Pragma("unroll") for (int u = 0; u < NCH; u++) x[u] = *(const float *)(sXb + ((unsigned)(v[u] >> 32) & 0xffffu)); \
                        _Pragma("unroll") for (int u = 0; u < NCH; u++) {       /* Split.eval: value <= threshold goes left (Split.java:118); a leaf stays where it is */ \
                            const unsigned off = (unsigned)(v[u] >> 48) + ((x[u] <= __uint_as_float((unsigned)v[u])) ? 0u : 8u);           \
                            v[u] = *(const unsigned long long *)(tb[u] + off);                                                             \
                        }                                                                                                                  \
                    }
                    const unsigned char *pd = pp + kEvalTreeTile + kEvalParts + part * kEvalPhases;
                    const int end0 = __builtin_amdgcn_readfirstlane((int)pd[0]);           // (scalar loop bounds, read once)
                    [[maybe_unused]] const int end1 = __builtin_amdgcn_readfirstlane((int)pd[kEvalPhases >= 2 ? 1 : 0]);
                    [[maybe_unused]] const int end2 = __builtin_amdgcn_readfirstlane((int)pd[kEvalPhases >= 3 ? 2 : 0]);
                    RL_EVAL_PHASE(kEvalPer, end0)
#if RL_EVAL_PHASES >= 2
                    RL_EVAL_PHASE(kEvalPh1, end1)
#endif
#if RL_EVAL_PHASES >= 3
                    RL_EVAL_PHASE(kEvalPh2, end2)
#endif
                    RL_EVAL_PHASE(kEvalPhLast, depth)
#undef RL_EVAL_PHASE
                    if (doc < nd) {
#pragma unroll
                        for (int u = 0; u < kEvalPer; u++) if (li[u] < tt) so[li[u] * kEvalDocs] = __uint_as_float((unsigned)v[u]);
                    }
                }
            } else if (k > 0 && doc < nd) {                                    // accumulate the previous tile while this one is walked
                const float *po = sO + (size_t)(cb ^ 1) * kEvalTreeTile * kEvalDocs + doc, *pw = sW + (cb ^ 1) * kEvalTreeTile;
                eval_accumulate<STAGED>(s, po, pw, tt_prev, st.tbase + t0 - kEvalTreeTile, st, si, n, d0 + doc);
            }
            tt_prev = tt;
        }
        __syncthreads();
        if (!walker && doc < nd) {
            if (k > 0) {
                const int cb = (k - 1) & 1;
                const float *po = sO + (size_t)cb * kEvalTreeTile * kEvalDocs + doc, *pw = sW + cb * kEvalTreeTile;
                eval_accumulate<STAGED>(s, po, pw, tt_prev, st.tbase + (k - 1) * kEvalTreeTile, st, si, n, d0 + doc);
            }
            if (!STAGED) out[d0 + doc] = s;
        }
    }
}
}  // namespace rl

namespace rl {

// the stages of rl_model_from_text, after the text is parsed and the device is open

// the trees as EnsTree arrays [trees][maxn] (what k_model_eval and the other per-document kernels walk) and the trees' weights
static int model_upload_ens(rl_model *m)
{
    const size_t nt = m->trees.size(), en = std::max<size_t>(1, nt * m->maxn);
    std::vector<int32_t> fi(en, -1), le(en, -1), ri(en, -1);
    std::vector<float> th(en, 0.f), ou(en, 0.f), w(std::max<size_t>(1, nt), 0.f);
    for (size_t i = 0; i < nt; i++) {
        const HostTree &t = m->trees[i];
        w[i] = t.weight;
        for (int j = 0; j < t.n_nodes; j++) {
            const size_t o = i * m->maxn + j;
            fi[o] = t.feature[j]; le[o] = t.left[j]; ri[o] = t.right[j]; th[o] = t.threshold[j]; ou[o] = t.output[j];
        }
    }
    memset(&m->ens, 0, sizeof(m->ens));
    RL_HIP(m->pool.upload(&m->ens.feat_idx, fi.data(), en)); RL_HIP(m->pool.upload(&m->ens.left, le.data(), en));
    RL_HIP(m->pool.upload(&m->ens.right, ri.data(), en)); RL_HIP(m->pool.upload(&m->ens.thr, th.data(), en));
    RL_HIP(m->pool.upload(&m->ens.out, ou.data(), en)); RL_HIP(m->pool.upload(&m->d_w, w.data(), w.size()));
    return RL_OK;
}

// what eval_pack made of the model, for k_model_eval_tiled; a model it refuses keeps d_pack null and takes k_model_eval
static int model_upload_pack(rl_model *m, const EvalPack &pk)
{
    m->maxcol = pk.maxcol;
    if (!pk.ok) return RL_OK;
    RL_HIP(m->pool.upload(&m->d_perm, pk.perm.data(), pk.perm.size()));
    RL_HIP(m->pool.upload(&m->d_gdepth, pk.meta.data(), pk.meta.size()));
    RL_HIP(m->pool.upload(&m->d_pack, pk.nodes.data(), pk.nodes.size()));
    RL_HIP(hipFuncSetAttribute((const void *)k_model_eval_tiled<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvalLdsBudget));
    RL_HIP(hipFuncSetAttribute((const void *)k_model_eval_tiled<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvalLdsBudget));
    return RL_OK;
}

}  // namespace rl

extern "C" {

int rl_model_from_text(const char *text, int32_t device, rl_model **out)
{
    if (!text || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<rl_model> m(new rl_model());
    std::string err;
    if (!model_from_text(text, m->trees, err)) return fail(RL_ERR_INVALID, "Error in Emsemble(xmlRepresentation): " + err);
    int rc = open_device(device, false);      // after the text is parsed; a model has never tested the architecture
    if (rc) return rc;
    m->device = device;
    m->knobs.read();
    std::map<int32_t, int> fids;                // the model's features, ascending, each once, and its largest tree
    for (auto &t : m->trees) { m->maxn = std::max(m->maxn, t.n_nodes); for (int f : t.feature) if (f != -1) fids[f] = 0; }
    for (auto &kv : fids) m->features.push_back(kv.first);
    if ((rc = model_upload_ens(m.get()))) return rc;
    if ((rc = model_upload_pack(m.get(), eval_pack(m->trees, m->maxn, m->knobs.deal, m->knobs.phased)))) return rc;
    *out = m.release();
    return RL_OK;
}

void rl_model_destroy(rl_model *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

int rl_model_num_trees(const rl_model *m, int32_t *n)
{
    if (!m) return fail(RL_ERR_INVALID, "null model");
    if (n) *n = (int32_t)m->trees.size();
    return RL_OK;
}

int rl_model_features(const rl_model *m, int32_t *ids, int32_t cap, int32_t *n)
{
    if (!m) return fail(RL_ERR_INVALID, "null model");
    if (n) *n = (int32_t)m->features.size();
    if (ids) for (int i = 0; i < cap && i < (int)m->features.size(); i++) ids[i] = m->features[i];
    return RL_OK;
}

// the staged rows' width and whether the tiled kernel takes this model at this row stride
static bool model_eval_tiled_ok(const rl_model *m, int32_t row_stride, int &cols, size_t &lds)
{
    cols = (int)std::min<int64_t>(INT32_MAX, std::max<int64_t>(row_stride, (int64_t)m->maxcol + 1));     // (a feature id may be INT32_MAX)
    lds = eval_tiled_lds(cols, m->maxn);
    return m->d_pack && lds <= kEvalLdsBudget && !m->knobs.generic;
}

static int model_eval_launch(rl_model *m, const float *dX, int64_t n_docs, int32_t row_stride, float *dO, hipStream_t s)
{
    int cols; size_t lds;
    if (model_eval_tiled_ok(m, row_stride, cols, lds)) {
        const int64_t tiles = (n_docs + kEvalDocs - 1) / kEvalDocs;
        hipLaunchKernelGGL(k_model_eval_tiled<false>, dim3((unsigned)std::min<int64_t>(tiles, 256 * 256)), dim3(kEvalThreads), lds, s,
                           (const unsigned long long *)m->d_pack, (const float *)m->d_w, m->maxn, (int)m->trees.size(), dX, n_docs, row_stride, cols, dO,
                           (const unsigned char *)m->d_perm, (const unsigned char *)m->d_gdepth, EvalStage{});
        m->last_path = RL_MODEL_PATH_TILED;
    } else {
        hipLaunchKernelGGL(k_model_eval, dim3((unsigned)std::min<int64_t>(8192, (n_docs + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, m->ens,
                           (const float *)m->d_w, m->maxn, (int)m->trees.size(), dX, n_docs, row_stride, dO);
        m->last_path = RL_MODEL_PATH_GENERIC;
    }
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int rl_model_predict(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, float *out)
{
    if (!m) return fail(RL_ERR_INVALID, "null model");
    if (!X || !out || n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad argument");
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    DevPool pool;
    float *dX = nullptr, *dO = nullptr;
    RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
    RL_HIP(pool.alloc(&dO, (size_t)n_docs));
    const int rc = model_eval_launch(m, dX, n_docs, row_stride, dO, 0);
    if (rc == RL_OK) { RL_HIP(hipDeviceSynchronize()); RL_HIP(hipMemcpy(out, dO, (size_t)n_docs * sizeof(float), hipMemcpyDeviceToHost)); }
    return rc;
}

int rl_model_predict_device(rl_model *m, const float *dX, int64_t n_docs, int32_t row_stride, float *dOut, void *stream)
{
    if (!m) return fail(RL_ERR_INVALID, "null model");
    if (!dX || !dOut || n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad argument");
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    return model_eval_launch(m, dX, n_docs, row_stride, dOut, (hipStream_t)stream);
}

int rl_model_debug_path(const rl_model *m, int32_t *path)
{
    if (!m || !path) return fail(RL_ERR_INVALID, "null argument");
    *path = m->last_path;
    return RL_OK;
}

}  // extern "C"
