// rl_shap.inc -- exact path-dependent TreeSHAP contributions of a tree model in one pass over a file.  DESIGN.md 27.
// Included at the end of rl_trainer.hip, after rl_contrib.inc (it uses rl_model's covers and node values, DevPool, StageEvents and
// kStageScratchDefault).
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
    const float *X; int64_t n; int stride;
    int32_t s0, ns, slots, bias;                                       // the pass: slots [s0, s0 + ns) of `slots` = C + 2; bias = C + 1
    double *out;                                                       // [n][slots]
};

__global__ __launch_bounds__(kShapDocsMax) void k_model_shap(const ShapArgs a)
{
    extern __shared__ __align__(16) unsigned char shp_raw[];
    const int D = (int)blockDim.x, AS = D + 1, tid = threadIdx.x;
    double *sA = (double *)shp_raw;                                     // [ns][D + 1]
    double *sW = sA + (size_t)a.ns * AS + tid;                         // [wd][D], this lane's column
    const double *tA = a.tb, *tB = tA + kShapT * kShapT, *tU = tB + kShapT * kShapT, *tR = tU + kShapT * kShapT;
    const int bias = a.bias - a.s0;                                    // in [0, ns) in the pass that holds it
    const int64_t d0 = (int64_t)blockIdx.x * D;                        // one row tile per block: the grid is ceil(n / D), n < 2^31
    const int nd = (int)min((int64_t)D, a.n - d0);
    for (int s = 0; s < a.ns; s++) sA[s * AS + tid] = 0.0;
    const float *row = a.X + (size_t)(d0 + (tid < nd ? tid : 0)) * a.stride;       // (a lane beyond the rows walks the first one's and stores nothing)
    for (int t = 0; t < a.nt; t++) {
        const double W = (double)a.w[t];
        if ((unsigned)bias < (unsigned)a.ns) sA[bias * AS + tid] = sA[bias * AS + tid] + W * a.root[t];
        for (int lf = a.leaf0[t]; lf < a.leaf0[t + 1]; lf++) {
            const ShapLeaf leaf = a.leaves[lf];
            const ShapElem *el = a.elems + leaf.el0;
            const int d = leaf.d;
            bool mine = false;
            for (int e = 0; e < d; e++) mine |= (unsigned)(el[e].slot - a.s0) < (unsigned)a.ns;
            if (!mine) continue;                                       // (wave-uniform, and a single-leaf tree adds to bias only)
            unsigned om = 0u;                                          // bit e: the row's own decision is the path's at every split of element e
            for (int e = 0; e < d; e++) {
                const int f = el[e].feat;
                const float v = (f < a.stride) ? row[f] : 0.f;         // -missingZero  DenseDataPoint.java:22-25
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
                const int s = el[e].slot - a.s0;
                if ((unsigned)s >= (unsigned)a.ns) continue;
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
    for (int e = tid; e < nd * a.ns; e += D) {                         // transposed: adjacent lanes, adjacent slots of one document
        const int dd = e / a.ns, s = e - dd * a.ns;
        a.out[(size_t)(d0 + dd) * a.slots + a.s0 + s] = sA[s * AS + dd];
    }
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
    const std::vector<int32_t> cols = columns ? std::vector<int32_t>(columns, columns + n_columns) : m->features;
    const int64_t C = (int64_t)cols.size(), slots = C + 2;
    const int wd = longest + 1;
    int docs; int64_t per_pass;
    if (!shap_plan(wd, slots, docs, per_pass)) return fail(RL_ERR_UNSUPPORTED, w + "the LDS has no room for one slot");
    g_sh_walk_ms = 0.0;
    g_sh_passes = (int32_t)((slots + per_pass - 1) / per_pass);
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    const size_t T = m->trees.size();
    std::vector<std::pair<int32_t, int32_t>> sorted((size_t)C);
    for (int64_t c = 0; c < C; c++) sorted[(size_t)c] = {cols[(size_t)c], (int32_t)c};
    std::sort(sorted.begin(), sorted.end());
    ShapPaths paths;
    std::vector<double> root(T);
    std::vector<int32_t> slot((size_t)m->maxn);
    for (size_t t = 0; t < T; t++) {
        const HostTree &h = m->trees[t];
        contrib_node_slots(h, sorted, (int32_t)C, slot.data());
        shap_tree_paths(h, m->cover.data() + t * m->maxn, slot.data(), paths);
        root[t] = m->value[t * m->maxn];
    }
    const std::vector<double> tb = shap_tables();
    // the rows of a chunk and their 8 (C + 2) bytes of output stay within scratch_bytes; a chunk holds at least one row
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : kStageScratchDefault;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_docs, budget / ((int64_t)row_stride * 4 + 8 * slots)));
    DevPool pool;
    ShapArgs a;
    memset(&a, 0, sizeof(a));
    int32_t *d_leaf0 = nullptr; ShapLeaf *d_leaves = nullptr; ShapElem *d_elems = nullptr; ShapCond *d_conds = nullptr;
    double *d_root = nullptr, *d_tb = nullptr; float *dX = nullptr;
    RL_HIP(pool.alloc(&d_leaf0, paths.leaf0.size()));
    RL_HIP(pool.alloc(&d_leaves, paths.leaves.size()));
    RL_HIP(pool.alloc(&d_elems, std::max<size_t>(1, paths.elems.size())));
    RL_HIP(pool.alloc(&d_conds, std::max<size_t>(1, paths.conds.size())));
    RL_HIP(pool.alloc(&d_root, T));
    RL_HIP(pool.alloc(&d_tb, tb.size()));
    RL_HIP(pool.alloc(&dX, (size_t)chunk * row_stride));
    RL_HIP(pool.alloc(&a.out, (size_t)chunk * slots));
    RL_HIP(hipMemcpy(d_leaf0, paths.leaf0.data(), paths.leaf0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_leaves, paths.leaves.data(), paths.leaves.size() * sizeof(ShapLeaf), hipMemcpyHostToDevice));
    if (!paths.elems.empty()) RL_HIP(hipMemcpy(d_elems, paths.elems.data(), paths.elems.size() * sizeof(ShapElem), hipMemcpyHostToDevice));
    if (!paths.conds.empty()) RL_HIP(hipMemcpy(d_conds, paths.conds.data(), paths.conds.size() * sizeof(ShapCond), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_root, root.data(), T * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_tb, tb.data(), tb.size() * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipFuncSetAttribute((const void *)k_model_shap, hipFuncAttributeMaxDynamicSharedMemorySize, kShapLds));
    a.leaf0 = d_leaf0; a.leaves = d_leaves; a.elems = d_elems; a.conds = d_conds; a.root = d_root; a.w = m->d_w; a.tb = d_tb;
    a.nt = (int)T; a.X = dX; a.stride = row_stride; a.slots = (int32_t)slots; a.bias = (int32_t)(C + 1);
    StageEvents ev;
    RL_HIP(ev.create());
    for (int64_t r0 = 0; r0 < n_docs; r0 += chunk) {
        const int64_t nr = std::min(chunk, n_docs - r0);
        a.n = nr;
        RL_HIP(hipMemcpy(dX, X + (size_t)r0 * row_stride, (size_t)nr * row_stride * sizeof(float), hipMemcpyHostToDevice));
        RL_HIP(hipEventRecord(ev.e[0], 0));
        for (int64_t s0 = 0; s0 < slots; s0 += per_pass) {
            a.s0 = (int32_t)s0; a.ns = (int32_t)std::min(per_pass, slots - s0);
            const size_t lds = ((size_t)a.ns * (docs + 1) + (size_t)wd * docs) * sizeof(double);
            hipLaunchKernelGGL(k_model_shap, dim3((unsigned)((nr + docs - 1) / docs)), dim3(docs), lds, 0, a);
            RL_HIP(hipGetLastError());
        }
        RL_HIP(hipEventRecord(ev.e[1], 0));
        RL_HIP(hipMemcpy(out + (size_t)r0 * slots, a.out, (size_t)nr * slots * sizeof(double), hipMemcpyDeviceToHost));
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_sh_walk_ms += (double)ms;
    }
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
