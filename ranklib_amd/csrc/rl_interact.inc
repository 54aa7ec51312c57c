// rl_interact.inc -- SHAP interaction values of a tree model in one pass over a file.  DESIGN.md 30.
// Included at the end of rl_trainer.hip, after rl_shap.inc (it uses its path tables, ShapArgs, shap_upload and k_model_shap itself, and
// rl_contrib.inc's SlotPass and SlotPlan; the rows go through RowStream chunk by chunk).
//
//   k_model_interact  one lane per row, a block of 64, 128 or 256 rows; the grid is row tile x CONDITIONED slot.  The block of slot i
//                     walks the leaves that have an element in slot i and at least two elements (interact_lists: every other leaf adds
//                     exactly zero), computes a leaf's o mask once, and per element c of the leaf in slot i runs k_model_shap's extend
//                     and unwind on the leaf's elements WITHOUT c: the unwind of element e, times (o_c - z_c) / 2, goes to the cell
//                     [i][slot_e].  LDS holds the accumulators [attributed slot of the pass][D + 1] f64 -- the slots 0 .. C, the bias has
//                     none -- and the lane's column of w[wr][D], wr = the model's longest element list, one row less than k_model_shap's.
//                     A lane touches only its own column: no atomic, no barrier inside the walk.  The conditioned slot, the leaf list,
//                     the elements, z, the slots, the conditions and the table factors are wave-uniform and come through uniform
//                     (scalar) loads; nothing of the path tables is staged.  The unwind keeps k_model_shap's select form.  When the
//                     attributed slots do not fit, several column passes; a cell's chain lies in one pass.  The block stores its piece
//                     of row i of every document's matrix, adjacent lanes on adjacent cells.
//   k_interact_finish one lane per (row, slot): the diagonal cell is the slot's SHAP value -- k_model_shap's, launched on the same chunk
//                     into scratch -- less the other cells of its row, j = 0 .. C ascending; the bias row and column are +0.0 but for
//                     the bias cell, which takes the SHAP bias slot.
//   No cross-block communication, no spin wait.  Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_interact_host.h"

namespace rl {

struct InteractArgs {
    const ShapLeaf *leaves; const ShapElem *elems; const ShapCond *conds;
    const int32_t *list0; const InteractLeaf *list;                    // per conditioned slot 0 .. C its leaves
    const float *w; const double *tb;                                  // the trees' weights; A, B, U, R [kShapT][kShapT] one behind the other
    SlotPass p;                                                        // the attributed slots of the pass [s0, s0 + ns) within 0 .. C; out [n][slots][slots]
};

__global__ __launch_bounds__(kShapDocsMax) void k_model_interact(const InteractArgs a)
{
    extern __shared__ __align__(16) unsigned char itr_raw[];
    const int D = (int)blockDim.x, AS = D + 1, tid = threadIdx.x;
    double *sA = (double *)itr_raw;                                     // [ns][D + 1]
    double *sW = sA + (size_t)a.p.ns * AS + tid;                         // [wr][D], this lane's column
    const double *tA = a.tb, *tB = tA + kShapT * kShapT, *tU = tB + kShapT * kShapT, *tR = tU + kShapT * kShapT;
    const int s0 = a.p.s0, ns = a.p.ns;
    const int ci = (int)blockIdx.y;                                    // the conditioned slot, 0 .. C
    const int64_t d0 = (int64_t)blockIdx.x * D;                        // one row tile per block: the grid is ceil(n / D), n < 2^31
    const int nd = (int)min((int64_t)D, a.p.n - d0);
    for (int s = 0; s < ns; s++) sA[s * AS + tid] = 0.0;
    const float *row = a.p.X + (size_t)(d0 + (tid < nd ? tid : 0)) * a.p.stride;       // (a lane beyond the rows walks the first one's and stores nothing)
    for (int k = a.list0[ci]; k < a.list0[ci + 1]; k++) {
        const InteractLeaf en = a.list[k];
        const ShapLeaf leaf = a.leaves[en.leaf];
        const ShapElem *el = a.elems + leaf.el0;
        const int d = leaf.d, dr = d - 1;                              // d >= 2; the reduced list has dr elements
        const double W = (double)a.w[en.tree];
        bool mine = false;
        for (int e = 0; e < d; e++) mine |= el[e].slot != ci && (unsigned)(el[e].slot - s0) < (unsigned)ns;
        if (!mine) continue;                                           // (wave-uniform)
        unsigned om = 0u;                                              // bit e: the row's own decision is the path's at every split of element e
        for (int e = 0; e < d; e++) {                                  // once per leaf, not once per conditioned element
            const int f = el[e].feat;
            const float v = (f < a.p.stride) ? row[f] : 0.f;             // -missingZero  DenseDataPoint.java:22-25
            const ShapCond *c = a.conds + el[e].c0;
            bool ok = true;
            for (int q = 0; q < el[e].nc; q++) ok &= ((v <= c[q].thr) == (c[q].left != 0));     // Split.java:118: a NaN goes right
            om |= (ok ? 1u : 0u) << e;
        }
        const double *Ud = tU + dr * kShapT, *Bd = tB + dr * kShapT, *Rd = tR + dr * kShapT;
        for (int c = 0; c < d; c++) {
            if (el[c].slot != ci) continue;                            // (several elements of a leaf share a slot in rest only)
            const double zc = el[c].z, oc = ((om >> c) & 1u) ? 1.0 : 0.0;
            const double hc = (oc - zc) * 0.5;
            sW[0] = 1.0;
            int l = 0;
            for (int j = 0; j < d; j++) {                              // extend over the elements without c, the tables at l = 1 .. d - 1
                if (j == c) continue;
                l++;
                const double z = el[j].z, o = ((om >> j) & 1u) ? 1.0 : 0.0;
                const double *Al = tA + l * kShapT, *Bl = tB + l * kShapT;
                double hi = 0.0;                                       // w[i + 1] as the step before left it (w[l] = 0.0)
                for (int i = l - 1; i >= 0; i--) {
                    const double wi = sW[i * D];
                    sW[(i + 1) * D] = hi + o * (wi * Al[i]);
                    hi = (z * wi) * Bl[i];
                }
                sW[0] = hi;
            }
            const double wtop = sW[dr * D];
            for (int e = 0; e < d; e++) {                              // unwind, the tables at d - 1
                if (e == c) continue;
                const int s = el[e].slot - s0;
                if (el[e].slot == ci || (unsigned)s >= (unsigned)ns) continue;
                const double z = el[e].z;
                const bool on = (om >> e) & 1u;
                const double o = on ? 1.0 : 0.0;
                double tot1 = 0.0, tot0 = 0.0, nxt = wtop;
                for (int i = dr - 1; i >= 0; i--) {
                    const double wi = sW[i * D];
                    const double tmp = nxt * Ud[i];
                    tot1 = tot1 + tmp;
                    nxt = wi - (tmp * z) * Bd[i];
                    tot0 = tot0 + wi * Rd[i];
                }
                if (!on) tot0 = tot0 / z;                              // (z == 0 here: the lane is skipped below)
                const double tot = on ? tot1 : tot0;
                double x = (tot * (o - z)) * leaf.out;
                x = x * hc;
                x = x * W;
                if (o != z && oc != zc) sA[s * AS + tid] = sA[s * AS + tid] + x;      // (the conditioned element is never divided by)
            }
        }
    }
    __syncthreads();
    const size_t S = (size_t)a.p.slots;
    for (int e = tid; e < nd * ns; e += D) {                           // adjacent lanes, adjacent cells of row ci of one document's matrix
        const int dd = e / ns, s = e - dd * ns;
        a.p.out[((size_t)(d0 + dd) * S + ci) * S + s0 + s] = sA[s * AS + dd];
    }
}

// one lane per (row, slot i of C + 2): i <= C makes its diagonal cell by the stated chain and zeroes the cell of the bias column;
// i == C + 1 writes the bias row
__global__ __launch_bounds__(kThreads) void k_interact_finish(const double *phi, double *out, int64_t n, int slots)
{
    const int64_t cells = n * slots;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < cells; g += (int64_t)gridDim.x * kThreads) {
        const int64_t doc = g / slots;
        const int i = (int)(g - doc * slots), C = slots - 2;
        double *r = out + ((size_t)doc * slots + i) * slots;
        if (i == C + 1) {
            for (int j = 0; j <= C; j++) r[j] = 0.0;
            r[C + 1] = phi[(size_t)doc * slots + C + 1];
            continue;
        }
        double v = phi[(size_t)doc * slots + i];
        for (int j = 0; j <= C; j++)
            if (j != i) v = v - r[j];
        r[i] = v;
        r[C + 1] = 0.0;
    }
}

static thread_local double g_it_walk_ms = 0.0, g_it_shap_ms = 0.0;     // the last call of this thread, device events
static thread_local int32_t g_it_passes = 0;

}  // namespace rl

extern "C" {

int rl_model_predict_interactions(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                                  int64_t scratch_bytes, double *out)
{
    static const std::string w = "rl_model_predict_interactions: ";
    std::string err;
    int rc = contrib_check_rows(w, m ? (int64_t)m->trees.size() : -1, X, n_docs, row_stride, err);
    if (!rc) rc = contrib_check_columns(w, columns, n_columns, scratch_bytes, out, err);
    if (rc) return fail(rc, err);
    if (m->cover.empty()) return fail(RL_ERR_STATE, w + "no rl_model_cover call has been made on this model");
    int32_t longest = 0;
    if (shap_check_paths(w, m->trees, &longest, err)) return fail(RL_ERR_UNSUPPORTED, err);
    SlotPlan sp = slot_plan(m, columns, n_columns);                    // k_model_shap's plan: all C + 2 slots
    if (interact_check_slots(w, sp.C, err)) return fail(RL_ERR_UNSUPPORTED, err);
    if (!shap_plan(longest + 1, sp.slots, sp.docs, sp.per_pass)) return fail(RL_ERR_UNSUPPORTED, w + "the LDS has no room for one slot");
    const int wr = interact_w_rows(longest);
    int docs = 0;
    int64_t per_pass = 0;                                              // k_model_interact's: the attributed slots 0 .. C
    if (!interact_plan(wr, sp.C + 1, docs, per_pass)) return fail(RL_ERR_UNSUPPORTED, w + "the LDS has no room for one slot");
    g_it_walk_ms = g_it_shap_ms = 0.0;
    g_it_passes = (int32_t)((sp.C + 1 + per_pass - 1) / per_pass);
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    RowStream rows;
    ShapArgs sa;
    ShapPaths paths;
    if ((rc = shap_upload(m, sp, rows.pool, paths, sa))) return rc;
    const InteractLists il = interact_lists(paths, (int32_t)sp.C);
    InteractArgs a;
    memset(&a, 0, sizeof(a));
    int32_t *d_list0 = nullptr; InteractLeaf *d_list = nullptr;
    RL_HIP(rows.pool.upload(&d_list0, il.list0.data(), il.list0.size()));
    RL_HIP(rows.pool.upload(&d_list, il.list.data(), il.list.size()));
    RL_HIP(hipFuncSetAttribute((const void *)k_model_interact, hipFuncAttributeMaxDynamicSharedMemorySize, kShapLds));
    a.leaves = sa.leaves; a.elems = sa.elems; a.conds = sa.conds; a.list0 = d_list0; a.list = d_list; a.w = m->d_w; a.tb = sa.tb;
    rows.chunk = interact_chunk_rows(n_docs, row_stride, sp.C, scratch_bytes);
    RL_HIP(rows.pool.alloc(&rows.dX, (size_t)rows.chunk * row_stride));
    const size_t S = (size_t)sp.slots;
    double *d_phi = nullptr, *d_out = nullptr;
    RL_HIP(rows.pool.alloc(&d_phi, (size_t)rows.chunk * S));
    RL_HIP(rows.pool.alloc(&d_out, (size_t)rows.chunk * S * S));
    sa.p.X = a.p.X = rows.dX; sa.p.stride = a.p.stride = row_stride; sa.p.slots = a.p.slots = (int32_t)sp.slots;
    sa.p.bias = a.p.bias = (int32_t)(sp.C + 1);
    sa.p.out = d_phi; a.p.out = d_out;
    StageEvents ev;                                                    // before k_model_shap, behind it, behind the walk and its finish
    RL_HIP(ev.create());
    bool pending = false;                                              // the events of the chunk before are recorded and not yet read
    auto read_events = [&]() -> int {
        float t = 0.f;
        RL_HIP(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
        g_it_shap_ms += (double)t;
        RL_HIP(hipEventElapsedTime(&t, ev.e[1], ev.e[2]));
        g_it_walk_ms += (double)t;
        pending = false;
        return RL_OK;
    };
    rc = rows.run(X, n_docs, row_stride, [&](int64_t nr) -> int {
        if (pending) { const int r = read_events(); if (r) return r; }       // (the copy-back of that chunk has waited for them)
        sa.p.n = a.p.n = nr;
        RL_HIP(hipEventRecord(ev.e[0], 0));
        for (int64_t s0 = 0; s0 < sp.slots; s0 += sp.per_pass) {
            sa.p.s0 = (int32_t)s0; sa.p.ns = (int32_t)std::min(sp.per_pass, sp.slots - s0);
            hipLaunchKernelGGL(k_model_shap, dim3((unsigned)((nr + sp.docs - 1) / sp.docs)), dim3(sp.docs),
                               ((size_t)sa.p.ns * (sp.docs + 1) + (size_t)(longest + 1) * sp.docs) * sizeof(double), 0, sa);
            RL_HIP(hipGetLastError());
        }
        RL_HIP(hipEventRecord(ev.e[1], 0));
        for (int64_t s0 = 0; s0 < sp.C + 1; s0 += per_pass) {
            a.p.s0 = (int32_t)s0; a.p.ns = (int32_t)std::min(per_pass, sp.C + 1 - s0);
            hipLaunchKernelGGL(k_model_interact, dim3((unsigned)((nr + docs - 1) / docs), (unsigned)(sp.C + 1)), dim3(docs),
                               ((size_t)a.p.ns * (docs + 1) + (size_t)wr * docs) * sizeof(double), 0, a);
            RL_HIP(hipGetLastError());
        }
        const int64_t cells = nr * sp.slots;
        hipLaunchKernelGGL(k_interact_finish, dim3((unsigned)std::min<int64_t>(65536, (cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0,
                           (const double *)d_phi, d_out, nr, (int)sp.slots);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[2], 0));
        pending = true;
        return RL_OK;
    }, d_out, out, (int64_t)(S * S));
    if (rc) return rc;
    if (pending && (rc = read_events())) return rc;
    m->last_path = RL_MODEL_PATH_INTERACT;
    return RL_OK;
}

int rl_debug_interact_times(double *walk_ms, double *shap_ms)
{
    if (!walk_ms || !shap_ms) return fail(RL_ERR_INVALID, "rl_debug_interact_times: null argument");
    *walk_ms = g_it_walk_ms;
    *shap_ms = g_it_shap_ms;
    return RL_OK;
}

int rl_debug_interact_passes(int32_t *passes)
{
    if (!passes) return fail(RL_ERR_INVALID, "rl_debug_interact_passes: null argument");
    *passes = g_it_passes;
    return RL_OK;
}

}  // extern "C"
