// rl_shap.inc -- exact path-dependent TreeSHAP contributions of a tree model in one pass over a file.  DESIGN.md 27.
// Included at the end of rl_trainer.hip, after rl_contrib.inc (it uses rl_model's covers and node values, RowStream, and rl_contrib.inc's
// SlotPass, SlotPlan and slot_stream: the slots of a call and its column passes go the way k_model_contribs' do).
//
//   k_model_shap      one lane per row, a block of 64, 128 or 256 rows; every row meets every leaf of every tree.  LDS holds the
//                     accumulators [slot of the pass][D + 1] f64 as k_model_contribs has them, and the per-lane array w[wd][D] f64 of the
//                     recurrence (wd = the model's longest element list + 1), so its dynamic index costs no scratch and the lanes of a
//                     wavefront hit consecutive 8-byte words.  A lane reads and writes only its own column of either: no atomics, no
//                     barrier inside the walk.  Tree, leaf, element, z, slot, the split conditions and the A / B / U / R factors are
//                     wave-uniform and come from global memory through uniform (scalar) reads: nothing of them is staged.  Per lane
//                     there are the row values (one gather per element, the lanes a row stride apart), the bit mask of the o_e, w[] and
//                     the accumulators.  Extend keeps the word it has just scaled in a register, so a step is one LDS read and one LDS
//                     write; unwind runs both arms in one loop over one read of w[i] and selects by o_e (the lanes of a wavefront differ
//                     in nothing else), the one division per element behind a branch that is skipped when no lane has o_e == 0.  A
//                     column pass walks every leaf that has an element of its slots again and keeps those elements' terms: a slot's
//                     chain lies in one pass.  The block's result is stored transposed: adjacent lanes write adjacent slots of a document.
//   No cross-block communication, no spin wait.  Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_shap_host.h"

namespace rl {

struct ShapArgs {
    const int32_t *leaf0; const ShapLeaf *leaves; const ShapElem *elems; const ShapCond *conds;
    const double *root;                                                // [nt] val[t][0]
    const float *w; const double *tb;                                  // the trees' weights; A, B, U, R [kShapT][kShapT] one behind the other
    int nt;
    SlotPass p;
};

__global__ __launch_bounds__(kShapDocsMax) void k_model_shap(const ShapArgs a)
{
    extern __shared__ __align__(16) unsigned char shp_raw[];
    const int D = (int)blockDim.x, AS = D + 1, tid = threadIdx.x;
    double *sA = (double *)shp_raw;                                     // [ns][D + 1]
    double *sW = sA + (size_t)a.p.ns * AS + tid;                         // [wd][D], this lane's column
    const double *tA = a.tb, *tB = tA + kShapT * kShapT, *tU = tB + kShapT * kShapT, *tR = tU + kShapT * kShapT;
    const int s0 = a.p.s0, ns = a.p.ns;
    const int bias = a.p.bias - s0;                                    // in [0, ns) in the pass that holds it
    const int64_t d0 = (int64_t)blockIdx.x * D;                        // one row tile per block: the grid is ceil(n / D), n < 2^31
    const int nd = (int)min((int64_t)D, a.p.n - d0);
    for (int s = 0; s < ns; s++) sA[s * AS + tid] = 0.0;
    const float *row = a.p.X + (size_t)(d0 + (tid < nd ? tid : 0)) * a.p.stride;       // (a lane beyond the rows walks the first one's and stores nothing)
    for (int t = 0; t < a.nt; t++) {
        const double W = (double)a.w[t];
        if ((unsigned)bias < (unsigned)ns) sA[bias * AS + tid] = sA[bias * AS + tid] + W * a.root[t];
        for (int lf = a.leaf0[t]; lf < a.leaf0[t + 1]; lf++) {
            const ShapLeaf leaf = a.leaves[lf];
            const ShapElem *el = a.elems + leaf.el0;
            const int d = leaf.d;
            bool mine = false;
            for (int e = 0; e < d; e++) mine |= (unsigned)(el[e].slot - s0) < (unsigned)ns;
            if (!mine) continue;                                       // (wave-uniform, and a single-leaf tree adds to bias only)
            unsigned om = 0u;                                          // bit e: the row's own decision is the path's at every split of element e
            for (int e = 0; e < d; e++) {
                const int f = el[e].feat;
                const float v = (f < a.p.stride) ? row[f] : 0.f;         // -missingZero  DenseDataPoint.java:22-25
                const ShapCond *c = a.conds + el[e].c0;
                bool ok = true;
                for (int k = 0; k < el[e].nc; k++) ok &= ((v <= c[k].thr) == (c[k].left != 0));     // Split.java:118: a NaN goes right
                om |= (ok ? 1u : 0u) << e;
            }
            sW[0] = 1.0;
            for (int l = 1; l <= d; l++) {                             // extend
                const double z = el[l - 1].z, o = ((om >> (l - 1)) & 1u) ? 1.0 : 0.0;
                const double *Al = tA + l * kShapT, *Bl = tB + l * kShapT;
                double hi = 0.0;                                       // w[i + 1] as the step before left it (w[l] = 0.0)
                for (int i = l - 1; i >= 0; i--) {
                    const double wi = sW[i * D];
                    sW[(i + 1) * D] = hi + o * (wi * Al[i]);
                    hi = (z * wi) * Bl[i];
                }
                sW[0] = hi;
            }
            const double *Ud = tU + d * kShapT, *Bd = tB + d * kShapT, *Rd = tR + d * kShapT;
            const double wd = sW[d * D];
            for (int e = 0; e < d; e++) {                              // unwind
                const int s = el[e].slot - s0;
                if ((unsigned)s >= (unsigned)ns) continue;
                const double z = el[e].z;
                const bool on = (om >> e) & 1u;
                const double o = on ? 1.0 : 0.0;
                double tot1 = 0.0, tot0 = 0.0, nxt = wd;
                for (int i = d - 1; i >= 0; i--) {
                    const double wi = sW[i * D];
                    const double tmp = nxt * Ud[i];
                    tot1 = tot1 + tmp;
                    nxt = wi - (tmp * z) * Bd[i];
                    tot0 = tot0 + wi * Rd[i];
                }
                if (!on) tot0 = tot0 / z;                              // (z == 0 here: the lane is skipped below)
                const double tot = on ? tot1 : tot0;
                if (o != z) sA[s * AS + tid] = sA[s * AS + tid] + ((tot * (o - z)) * leaf.out) * W;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < nd * ns; e += D) {                           // transposed: adjacent lanes, adjacent slots of one document
        const int dd = e / ns, s = e - dd * ns;
        a.p.out[(size_t)(d0 + dd) * a.p.slots + s0 + s] = sA[s * AS + dd];
    }
}

// The tables of a call on the device, in `pool`: the path tables of every tree under the slots of sp and the model's covers (left in
// `paths` for the caller), the root values and the factor tables; `a` is ready but for its SlotPass.  Shared with rl_interact.inc.
static int shap_upload(const rl_model *m, const SlotPlan &sp, DevPool &pool, ShapPaths &paths, ShapArgs &a)
{
    const size_t T = m->trees.size();
    std::vector<double> root(T);
    std::vector<int32_t> slot((size_t)m->maxn);
    for (size_t t = 0; t < T; t++) {
        const HostTree &h = m->trees[t];
        contrib_node_slots(h, sp.sorted, (int32_t)sp.C, slot.data());
        shap_tree_paths(h, m->cover.data() + t * m->maxn, slot.data(), paths);
        root[t] = m->value[t * m->maxn];
    }
    const std::vector<double> tb = shap_tables();
    memset(&a, 0, sizeof(a));
    int32_t *d_leaf0 = nullptr; ShapLeaf *d_leaves = nullptr; ShapElem *d_elems = nullptr; ShapCond *d_conds = nullptr;
    double *d_root = nullptr, *d_tb = nullptr;
    RL_HIP(pool.upload(&d_leaf0, paths.leaf0.data(), paths.leaf0.size()));
    RL_HIP(pool.upload(&d_leaves, paths.leaves.data(), paths.leaves.size()));
    RL_HIP(pool.upload(&d_elems, paths.elems.data(), paths.elems.size()));
    RL_HIP(pool.upload(&d_conds, paths.conds.data(), paths.conds.size()));
    RL_HIP(pool.upload(&d_root, root.data(), T));
    RL_HIP(pool.upload(&d_tb, tb.data(), tb.size()));
    RL_HIP(hipFuncSetAttribute((const void *)k_model_shap, hipFuncAttributeMaxDynamicSharedMemorySize, kShapLds));
    a.leaf0 = d_leaf0; a.leaves = d_leaves; a.elems = d_elems; a.conds = d_conds; a.root = d_root; a.w = m->d_w; a.tb = d_tb; a.nt = (int)T;
    return RL_OK;
}

static thread_local double g_sh_walk_ms = 0.0;                         // the last call of this thread, device events
static thread_local int32_t g_sh_passes = 0;

}  // namespace rl

extern "C" {

int rl_model_shap_limits(const rl_model *m, int32_t *max_path, int32_t *limit)
{
    if (!m || !max_path || !limit) return fail(RL_ERR_INVALID, "rl_model_shap_limits: null argument");
    std::string err;
    shap_check_paths("", m->trees, max_path, err);
    *limit = kShapP;
    return RL_OK;
}

int rl_model_predict_shap(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                          int64_t scratch_bytes, double *out)
{
    static const std::string w = "rl_model_predict_shap: ";
    std::string err;
    int rc = contrib_check_rows(w, m ? (int64_t)m->trees.size() : -1, X, n_docs, row_stride, err);
    if (!rc) rc = contrib_check_columns(w, columns, n_columns, scratch_bytes, out, err);
    if (rc) return fail(rc, err);
    if (m->cover.empty()) return fail(RL_ERR_STATE, w + "no rl_model_cover call has been made on this model");
    int32_t longest = 0;
    if (shap_check_paths(w, m->trees, &longest, err)) return fail(RL_ERR_UNSUPPORTED, err);
    SlotPlan sp = slot_plan(m, columns, n_columns);
    const int wd = longest + 1;
    if (!shap_plan(wd, sp.slots, sp.docs, sp.per_pass)) return fail(RL_ERR_UNSUPPORTED, w + "the LDS has no room for one slot");
    g_sh_walk_ms = 0.0;
    g_sh_passes = sp.passes();
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    RowStream rows;
    ShapArgs a;
    ShapPaths paths;
    if ((rc = shap_upload(m, sp, rows.pool, paths, a))) return rc;
    rc = slot_stream(k_model_shap, a, sp, X, n_docs, row_stride, scratch_bytes, out, rows,
                     [&](int ns) { return ((size_t)ns * (sp.docs + 1) + (size_t)wd * sp.docs) * sizeof(double); });
    g_sh_walk_ms = rows.ms;
    if (rc) return rc;
    m->last_path = RL_MODEL_PATH_SHAP;
    return RL_OK;
}

int rl_debug_shap_times(double *walk_ms)
{
    if (!walk_ms) return fail(RL_ERR_INVALID, "rl_debug_shap_times: null argument");
    *walk_ms = g_sh_walk_ms;
    return RL_OK;
}

int rl_debug_shap_passes(int32_t *passes)
{
    if (!passes) return fail(RL_ERR_INVALID, "rl_debug_shap_passes: null argument");
    *passes = g_sh_passes;
    return RL_OK;
}

}  // extern "C"
