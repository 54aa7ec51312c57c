// rl_permimp.inc -- permutation feature importance of a tree model in one pass over a file: every (column, repeat) cell's scores and
// per-list metric values without a permuted copy of the rows.  DESIGN.md 24.
// Included at the end of rl_trainer.hip, after rl_stage.inc (it uses StageRank, StageEvents, k_stage_eval and stage_chunk: a chunk of cells is
// at least one cell and at most gridDim.y batches' worth).
//
//   k_model_permuted_scores<B>   one lane per document, blockIdx.y over batches of B cells.  Cell g < n_columns * n_repeats is column
//                                columns[g / n_repeats] under repeat g % n_repeats; one more cell, the last, is the base (it has no column).  A
//                                batch is B consecutive cells, so it covers a few adjacent entries of columns[] under all their repeats.  A
//                                lane gathers its B donor values X[donor[r][i]][col] once, then per tree:
//                                  * uses[batch][tree] == 0 (built on the host from the trees' column sets; wave-uniform, a scalar load):
//                                    no node of the tree tests a column of the batch -- one walk, its output joins all B chains;
//                                  * otherwise the base walk is made once.  At a node on it that tests a cell's column the donated value is
//                                    compared with the threshold too: while both go the same way the cell's path IS the base path (and the
//                                    next node that tests the column is asked again); where they part the cell's walk goes on from the other
//                                    child with the donated value standing in at every later node that tests the column.  Cells that never
//                                    part take the base output.
//                                Each chain is Ensemble.eval's statement s = (float)((double)s + (double)out * (double)w[t]).  It walks the
//                                EnsTree arrays, so it serves every model, packed or not.  The scores land as sc[cell in chunk][doc],
//                                coalesced, and k_stage_eval ranks them, cells standing where stages stand.
//   No cross-block atomic, no spin wait.  Built with -ffp-contract=off like the rest.  No CPU fallback.
namespace rl {

constexpr int kPermBatch = RL_PERMUTED_BATCH;

struct PermArgs {
    EnsTree e; const float *w; int MAXN, nt;
    const float *X; int64_t n; int stride;
    const int32_t *columns; int32_t n_repeats, n_cells;       // n_cells = n_columns * n_repeats; cell n_cells is the base
    const int32_t *donor;                                     // [n_repeats][n]
    int32_t c0, nc;                                           // the chunk: cells [c0, c0 + nc)
    const uint8_t *uses;                                      // [batches of the chunk][nt]
    float *sc;                                                // [nc][n]
};

template <int B>
__global__ __launch_bounds__(kThreads) void k_model_permuted_scores(const PermArgs a)
{
    const int b0 = (int)blockIdx.y * B;                        // the batch's first cell in the chunk
    const uint8_t *uses = a.uses + (size_t)blockIdx.y * a.nt;
    int col[B], rep[B];
#pragma unroll
    for (int u = 0; u < B; u++) {                              // wave-uniform
        const int g = a.c0 + b0 + u;
        const bool cell = b0 + u < a.nc && g < a.n_cells;      // (the base and the slots past the chunk's end have no column: -1 is a leaf's mark, never compared)
        col[u] = cell ? a.columns[g / a.n_repeats] : -1;
        rep[u] = cell ? g % a.n_repeats : 0;
        if (col[u] >= a.stride) col[u] = -1;                   // both sides read 0 there: the cell equals the base
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = a.X + (size_t)i * a.stride;
        float dv[B], s[B];
#pragma unroll
        for (int u = 0; u < B; u++) {
            s[u] = 0.f;
            dv[u] = 0.f;
            if (col[u] >= 0) dv[u] = a.X[(size_t)a.donor[(size_t)rep[u] * a.n + i] * a.stride + col[u]];
        }
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
#pragma unroll
                for (int u = 0; u < B; u++)
                    if (fc == col[u] && part[u] < 0 && (dv[u] <= th) != go_left) part[u] = go_left ? ri : le;
                nd = go_left ? le : ri;
            }
            const float base_out = a.e.out[o + nd];
#pragma unroll
            for (int u = 0; u < B; u++) {
                float out = base_out;
                if (part[u] >= 0) {
                    int pn = part[u], pf;
                    while ((pf = a.e.feat_idx[o + pn]) != -1) {
                        const float v = (pf == col[u]) ? dv[u] : (pf < a.stride) ? row[pf] : 0.f;
                        pn = (v <= a.e.thr[o + pn]) ? a.e.left[o + pn] : a.e.right[o + pn];
                    }
                    out = a.e.out[o + pn];
                }
                s[u] = (float)((double)s[u] + (double)out * wt);               // Ensemble.java:113
            }
        }
#pragma unroll
        for (int u = 0; u < B; u++)
            if (b0 + u < a.nc) a.sc[(size_t)(b0 + u) * a.n + i] = s[u];
    }
}

static thread_local double g_pi_walk_ms = 0.0, g_pi_rank_ms = 0.0;      // the last permuted call of this thread, device events

// the checks both entry points share; who names the call
static int perm_check(const char *who, const rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns,
                      int32_t n_columns, const int32_t *donor, int32_t n_repeats, const void *out)
{
    const std::string w = std::string(who) + ": ";
    if (!X) return fail(RL_ERR_INVALID, w + "null X");
    if (!columns) return fail(RL_ERR_INVALID, w + "null columns");
    if (!donor) return fail(RL_ERR_INVALID, w + "null donor");
    if (!out) return fail(RL_ERR_INVALID, w + "null output");
    if (n_docs < 0) return fail(RL_ERR_INVALID, w + "n_docs must be >= 0");
    if (n_docs > (int64_t)INT32_MAX) return fail(RL_ERR_UNSUPPORTED, w + "more than 2^31 documents per call");
    if (row_stride < 1) return fail(RL_ERR_INVALID, w + "row_stride must be >= 1");
    if (n_columns < 1) return fail(RL_ERR_INVALID, w + "n_columns must be >= 1");
    if (n_repeats < 1) return fail(RL_ERR_INVALID, w + "n_repeats must be >= 1");
    if ((int64_t)n_columns * n_repeats >= (int64_t)INT32_MAX) return fail(RL_ERR_UNSUPPORTED, w + "more than 2^31 cells per call");
    for (int32_t c = 0; c < n_columns; c++)
        if (columns[c] < 0) return fail(RL_ERR_INVALID, w + "columns[" + std::to_string(c) + "] = " + std::to_string(columns[c]) + " is negative");
    for (int32_t r = 0; r < n_repeats; r++)
        for (int64_t i = 0; i < n_docs; i++) {
            const int32_t d = donor[(size_t)r * n_docs + i];
            if (d < 0 || (int64_t)d >= n_docs)
                return fail(RL_ERR_INVALID, w + "donor[" + std::to_string(r) + "][" + std::to_string(i) + "] = " + std::to_string(d) + " is outside [0, " +
                                                std::to_string(n_docs) + ")");
        }
    if (!m) return fail(RL_ERR_INVALID, w + "null model");             // (after the arguments a machine without a device can check)
    if (m->trees.empty()) return fail(RL_ERR_INVALID, w + "the model has no trees");
    return RL_OK;
}

// The walk of a call.  The cells (the base last) are cut into chunks of `chunk`, a chunk into batches of kPermBatch; uses[batch][tree] says
// whether a node of the tree tests a column of the batch.  It is built once, when the call starts, from the trees' column sets.
struct PermWalk {
    PermArgs a;
    int chunk = 1;
    int32_t total = 0;                      // n_cells + 1
    std::vector<size_t> batch0;             // per chunk: its first row of uses
    const uint8_t *d_uses0 = nullptr;
    int prepare(DevPool &pool, rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                const int32_t *donor, int32_t n_repeats, int chunk_)
    {
        memset(&a, 0, sizeof(a));
        chunk = chunk_;
        const int32_t T = (int32_t)m->trees.size();
        a.e = m->ens; a.w = m->d_w; a.MAXN = m->maxn; a.nt = T; a.n = n_docs; a.stride = row_stride;
        a.n_repeats = n_repeats; a.n_cells = n_columns * n_repeats;
        total = a.n_cells + 1;
        std::map<int32_t, std::vector<int32_t>> trees_of;      // column -> the trees that test it, ascending, each once
        for (int32_t t = 0; t < T; t++)
            for (int f : m->trees[t].feature)
                if (f != -1) { auto &v = trees_of[f]; if (v.empty() || v.back() != t) v.push_back(t); }
        std::vector<uint8_t> uses;
        for (int32_t c0 = 0; c0 < total; c0 += chunk) {
            const int nc = std::min<int32_t>(chunk, total - c0), nb = (nc + kPermBatch - 1) / kPermBatch;
            batch0.push_back(uses.size() / (size_t)T);
            uses.resize(uses.size() + (size_t)nb * T, 0);
            for (int j = 0; j < nc; j++) {
                const int32_t g = c0 + j;
                if (g >= a.n_cells || columns[g / n_repeats] >= row_stride) continue;
                auto it = trees_of.find(columns[g / n_repeats]);
                if (it == trees_of.end()) continue;
                uint8_t *rowp = uses.data() + (batch0.back() + (size_t)(j / kPermBatch)) * T;
                for (int32_t t : it->second) rowp[t] = 1;
            }
        }
        float *dX = nullptr; int32_t *d_cols = nullptr, *d_donor = nullptr; uint8_t *d_uses = nullptr;
        RL_HIP(pool.upload(&dX, X, (size_t)n_docs * row_stride));
        RL_HIP(pool.upload(&d_cols, columns, (size_t)n_columns));
        RL_HIP(pool.upload(&d_donor, donor, (size_t)n_repeats * n_docs));
        RL_HIP(pool.upload(&d_uses, uses.data(), uses.size()));
        RL_HIP(pool.alloc(&a.sc, (size_t)chunk * n_docs));
        a.X = dX; a.columns = d_cols; a.donor = d_donor; d_uses0 = d_uses;
        return RL_OK;
    }
    // chunk number ci: cells [ci * chunk, ..) into a.sc; returns the number of cells
    int launch(int ci)
    {
        a.c0 = ci * chunk;
        a.nc = std::min<int32_t>(chunk, total - a.c0);
        a.uses = d_uses0 + batch0[ci] * (size_t)a.nt;
        const dim3 grid((unsigned)std::min<int64_t>(8192, (a.n + kThreads - 1) / kThreads), (unsigned)((a.nc + kPermBatch - 1) / kPermBatch));
        hipLaunchKernelGGL((k_model_permuted_scores<kPermBatch>), grid, dim3(kThreads), 0, 0, a);
        return a.nc;
    }
};

}  // namespace rl

extern "C" {

int rl_model_predict_permuted(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                              const int32_t *donor, int32_t n_repeats, float *out_base, float *out)
{
    int rc = perm_check("rl_model_predict_permuted", m, X, n_docs, row_stride, columns, n_columns, donor, n_repeats, out);
    if (rc) return rc;
    g_pi_walk_ms = g_pi_rank_ms = 0.0;
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    DevPool pool;
    PermWalk walk;
    const int32_t total = n_columns * n_repeats + 1;
    rc = walk.prepare(pool, m, X, n_docs, row_stride, columns, n_columns, donor, n_repeats, stage_chunk(0, n_docs * (int64_t)sizeof(float), total));
    if (rc) return rc;
    StageEvents ev;
    RL_HIP(ev.create());
    for (int ci = 0; ci * walk.chunk < total; ci++) {
        RL_HIP(hipEventRecord(ev.e[0], 0));
        const int nc = walk.launch(ci);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        const int c0 = ci * walk.chunk, real = std::min(nc, total - 1 - c0);      // the base is the last cell of the last chunk
        if (real > 0) RL_HIP(hipMemcpy(out + (size_t)c0 * n_docs, walk.a.sc, (size_t)real * n_docs * sizeof(float), hipMemcpyDeviceToHost));
        if (real < nc && out_base) RL_HIP(hipMemcpy(out_base, walk.a.sc + (size_t)real * n_docs, (size_t)n_docs * sizeof(float), hipMemcpyDeviceToHost));
        RL_HIP(hipDeviceSynchronize());
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_pi_walk_ms += (double)ms;
    }
    m->last_path = RL_MODEL_PATH_PERMUTED;
    return RL_OK;
}

int rl_model_eval_permuted(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const float *labels, const int32_t *qoff,
                           int32_t n_lists, const int32_t *qkey, const double *ideal_dcg, const int32_t *rel_doc_count, int32_t metric, int32_t k,
                           double err_max, const int32_t *columns, int32_t n_columns, const int32_t *donor, int32_t n_repeats,
                           int64_t scratch_bytes, double *out_base, uint8_t *out_base_nan, double *out_metric, uint8_t *out_nan, double *out_ideal)
{
    static const char *who = "rl_model_eval_permuted";
    int rc = perm_check(who, m, X, n_docs, row_stride, columns, n_columns, donor, n_repeats, out_metric);
    if (rc) return rc;
    if (!out_nan) return fail(RL_ERR_INVALID, std::string(who) + ": null out_nan");
    if (!out_base) return fail(RL_ERR_INVALID, std::string(who) + ": null out_base");
    if (!out_base_nan) return fail(RL_ERR_INVALID, std::string(who) + ": null out_base_nan");
    if (scratch_bytes < 0) return fail(RL_ERR_INVALID, std::string(who) + ": scratch_bytes must be >= 0");
    std::vector<double> ideal, disc;
    std::string err;
    rc = eval_prepare_lists(who, metric, k, err_max, nullptr, labels, n_docs, qoff, n_lists, qkey, ideal_dcg, rel_doc_count, out_metric, ideal,
                            disc, err);
    if (rc) return fail(rc, err);
    g_pi_walk_ms = g_pi_rank_ms = 0.0;
    RL_HIP(hipSetDevice(m->device));
    StageRank rank;
    rank.classify(qoff, n_lists);
    const int32_t total = n_columns * n_repeats + 1;
    DevPool pool;
    PermWalk walk;
    rc = walk.prepare(pool, m, X, n_docs, row_stride, columns, n_columns, donor, n_repeats, stage_chunk(scratch_bytes, rank.bytes_per_row(n_docs), total));
    if (rc) return rc;
    rc = rank.upload(pool, walk.a.sc, walk.chunk, labels, n_docs, qoff, n_lists, ideal, disc, rel_doc_count, metric, k, err_max);
    if (rc) return rc;
    StageEvents ev;
    RL_HIP(ev.create());
    for (int ci = 0; ci * walk.chunk < total; ci++) {
        RL_HIP(hipEventRecord(ev.e[0], 0));
        const int nc = walk.launch(ci);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        rc = rank.launch(nc);
        if (rc) return rc;
        RL_HIP(hipEventRecord(ev.e[2], 0));
        const int c0 = ci * walk.chunk, real = std::min(nc, total - 1 - c0);      // the base is the last cell of the last chunk
        if (real > 0) {
            RL_HIP(hipMemcpy(out_metric + (size_t)c0 * n_lists, rank.a.out, (size_t)real * n_lists * sizeof(double), hipMemcpyDeviceToHost));
            RL_HIP(hipMemcpy(out_nan + (size_t)c0 * n_lists, rank.a.nan, (size_t)real * n_lists, hipMemcpyDeviceToHost));
        }
        if (real < nc) {
            RL_HIP(hipMemcpy(out_base, rank.a.out + (size_t)real * n_lists, (size_t)n_lists * sizeof(double), hipMemcpyDeviceToHost));
            RL_HIP(hipMemcpy(out_base_nan, rank.a.nan + (size_t)real * n_lists, (size_t)n_lists, hipMemcpyDeviceToHost));
        }
        RL_HIP(hipDeviceSynchronize());
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_pi_walk_ms += (double)ms;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
        g_pi_rank_ms += (double)ms;
    }
    m->last_path = RL_MODEL_PATH_PERMUTED;
    if (out_ideal) std::copy(ideal.begin(), ideal.end(), out_ideal);
    return RL_OK;
}

int rl_debug_permuted_times(double *walk_ms, double *rank_ms)
{
    if (!walk_ms || !rank_ms) return fail(RL_ERR_INVALID, "rl_debug_permuted_times: null argument");
    *walk_ms = g_pi_walk_ms;
    *rank_ms = g_pi_rank_ms;
    return RL_OK;
}

}  // extern "C"
