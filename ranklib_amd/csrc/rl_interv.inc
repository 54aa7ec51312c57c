// rl_interv.inc -- interventional TreeSHAP of a tree model against background rows in one pass over a file.  DESIGN.md 34.
// Included at the end of rl_trainer.hip, after rl_interact.inc (it uses rl_shap_host.h's path tables, RowStream, and rl_contrib.inc's
// SlotPass, SlotPlan and slot_plan: the slots of a call and its column passes go the way k_model_contribs' do).  Needs no cover.
//
//   k_interv_masks    one lane per background row, the grid's second dimension over the trees of a chunk.  Per leaf of the tree the lane
//                     builds the bit mask zm -- bit e: the background row's own decision is the path's at every split of element e --
//                     and stores it to zm[leaf][z], adjacent lanes on adjacent words; the leaf whose mask is full is the one the row
//                     ends in and goes to zleaf[tree][z].
//   k_interv_bias     one lane per tree of the chunk: the f64 chain over z ascending of (double)out at zleaf[tree][z].  The host adds the
//                     chunk's trees to the bias in tree order.
//   k_model_interv    one lane per document, a block of 64, 128 or 256 documents; every document meets every leaf of every tree of the
//                     chunk and, per leaf, every background row.  A lane builds xm once per leaf from one gather per element and keeps
//                     it in a register.  The z loop reads zm[leaf][z .. z + 3] with ONE 16-byte uniform (scalar) load: the address is
//                     the same for every lane, so the masks cost no vector memory instruction, no LDS and no barrier, and one scalar
//                     cache line serves 16 background rows of all the block's wavefronts (a staged LDS strip would need a barrier per
//                     strip inside the walk and an LDS read per lane and z).  The meet test is an or, a xor and two compares; only
//                     lanes that meet the leaf with a mask unlike z's go on: two population counts, the two table values T[a][b] and
//                     -T[b][a] from the copy of T in LDS (the indices differ from lane to lane), and one LDS read-add-write per
//                     DIFFERING element in the lane's column of s[wd][D] f64 -- the loop runs over the set bits of xm ^ zm; every s_e
//                     is a chain of its own, so the order among the elements changes no bit.  After the last z the touched s_e go,
//                     in element order, into the accumulators [slot of the pass][D + 1] f64 and are set back to +0.0.  A lane touches
//                     only its own column of either: no atomics, no barrier inside the walk.  Between tree chunks the accumulators
//                     travel through `out`: a later chunk starts from what the one before stored, the last divides by B and writes the
//                     bias.  The block's result is stored transposed: adjacent lanes write adjacent slots of a document.
//   No cross-block communication, no spin wait.  Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_interv_host.h"

namespace rl {

struct IntervMaskArgs {
    const int32_t *leaf0; const ShapLeaf *leaves; const ShapElem *elems; const ShapCond *conds;
    const float *BG; int B, BS, stride;                                // the background [B][stride]; BS = interv_mask_stride(B)
    int t0, ntc, lbase;                                                // the chunk's trees [t0, t0 + ntc); lbase = leaf0[t0]
    uint32_t *zm; int32_t *zleaf;                                      // [leaves of the chunk][BS]; [ntc][B]
};

__device__ __forceinline__ unsigned interv_full(int d) { return d >= 32 ? ~0u : (1u << d) - 1u; }

// bit e: the row's own decision is the path's at every split of element e (k_model_shap's o_e)
__device__ __forceinline__ unsigned interv_mask(const ShapElem *el, int d, const ShapCond *conds, const float *row, int stride)
{
    unsigned om = 0u;
    for (int e = 0; e < d; e++) {
        const int f = el[e].feat;
        const float v = (f < stride) ? row[f] : 0.f;                   // -missingZero  DenseDataPoint.java:22-25
        const ShapCond *c = conds + el[e].c0;
        bool ok = true;
        for (int k = 0; k < el[e].nc; k++) ok &= ((v <= c[k].thr) == (c[k].left != 0));     // Split.java:118: a NaN goes right
        om |= (ok ? 1u : 0u) << e;
    }
    return om;
}

__global__ __launch_bounds__(kThreads) void k_interv_masks(const IntervMaskArgs a)
{
    const int z = (int)blockIdx.x * kThreads + (int)threadIdx.x;       // B <= 16 384
    if (z >= a.BS) return;
    const float *row = a.BG + (size_t)z * a.stride;
    for (int ty = (int)blockIdx.y; ty < a.ntc; ty += (int)gridDim.y) {
        const int t = a.t0 + ty;
        int at = a.leaf0[t];
        if (z >= a.B) {                                                // the padding of a buffer row: the walk's 16-byte load reads it (and
            for (int lf = a.leaf0[t]; lf < a.leaf0[t + 1]; lf++) a.zm[(size_t)(lf - a.lbase) * a.BS + z] = 0u;      // skips it), so it is defined
            continue;
        }
        for (int lf = a.leaf0[t]; lf < a.leaf0[t + 1]; lf++) {
            const ShapLeaf leaf = a.leaves[lf];
            const unsigned m = interv_mask(a.elems + leaf.el0, leaf.d, a.conds, row, a.stride);
            a.zm[(size_t)(lf - a.lbase) * a.BS + z] = m;
            if (m == interv_full(leaf.d)) at = lf;                     // (exactly one leaf of a tree)
        }
        a.zleaf[(size_t)ty * a.B + z] = at;
    }
}

__global__ __launch_bounds__(kThreads) void k_interv_bias(const ShapLeaf *leaves, const int32_t *zleaf, int B, int ntc, double *mt)
{
    const int t = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (t >= ntc) return;
    double m = 0.0;
    for (int z = 0; z < B; z++) m = m + leaves[zleaf[(size_t)t * B + z]].out;
    mt[t] = m;
}

struct IntervArgs {
    const int32_t *leaf0; const ShapLeaf *leaves; const ShapElem *elems; const ShapCond *conds;
    const float *w; const double *tb;                                  // the trees' weights; T [kShapT][kShapT]
    const uint32_t *zm; int B, BS;                                     // the chunk's masks [leaves of the chunk][BS]
    int t0, t1, lbase, wd;                                             // the chunk's trees [t0, t1); lbase = leaf0[t0]; wd = the longest element list
    int first, last;                                                   // the call's first / last tree chunk
    double bias;                                                       // what the last chunk writes to the bias slot
    SlotPass p;
};

__global__ __launch_bounds__(kShapDocsMax) void k_model_interv(const IntervArgs a)
{
    extern __shared__ __align__(16) unsigned char iv_raw[];
    const int D = (int)blockDim.x, AS = D + 1, tid = threadIdx.x;
    double *sT = (double *)iv_raw;                                     // [kShapT][kShapT]
    double *sA = sT + kShapT * kShapT;                                 // [ns][D + 1]
    double *sS = sA + (size_t)a.p.ns * AS + tid;                       // [wd][D], this lane's column
    const int s0 = a.p.s0, ns = a.p.ns;
    const int64_t d0 = (int64_t)blockIdx.x * D;                        // one row tile per block: the grid is ceil(n / D), n < 2^31
    const int nd = (int)min((int64_t)D, a.p.n - d0);
    for (int i = tid; i < kShapT * kShapT; i += D) sT[i] = a.tb[i];
    for (int e = 0; e < a.wd; e++) sS[e * D] = 0.0;
    for (int s = 0; s < ns; s++) sA[s * AS + tid] = 0.0;
    __syncthreads();
    if (!a.first)                                                      // the chains go on from what the tree chunk before stored
        for (int e = tid; e < nd * ns; e += D) {
            const int dd = e / ns, s = e - dd * ns;
            sA[s * AS + dd] = a.p.out[(size_t)(d0 + dd) * a.p.slots + s0 + s];
        }
    __syncthreads();
    if (tid < nd) {                                                    // a lane beyond the rows walks nothing; a wavefront of such lanes skips the walk
        const float *row = a.p.X + (size_t)(d0 + tid) * a.p.stride;
        for (int t = a.t0; t < a.t1; t++) {
            const double W = (double)a.w[t];
            for (int lf = a.leaf0[t]; lf < a.leaf0[t + 1]; lf++) {
                const ShapLeaf leaf = a.leaves[lf];
                const ShapElem *el = a.elems + leaf.el0;
                const int d = leaf.d;
                bool mine = false;
                for (int e = 0; e < d; e++) mine |= (unsigned)(el[e].slot - s0) < (unsigned)ns;
                if (!mine) continue;                                       // (wave-uniform, and a single-leaf tree adds to bias only)
                const unsigned xm = interv_mask(el, d, a.conds, row, a.p.stride), full = interv_full(d);
                const uint32_t *zr = a.zm + (size_t)(lf - a.lbase) * a.BS;
                unsigned touched = 0u;
                for (int z4 = 0; z4 < a.B; z4 += 4) {
                    const uint4 q = *(const uint4 *)(zr + z4);              // uniform: one scalar load of four masks
                    const unsigned zz[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (z4 + k >= a.B) break;                          // (the padding of the row)
                        const unsigned zmv = zz[k], df = xm ^ zmv;
                        if ((xm | zmv) != full || df == 0u) continue;      // z does not meet the leaf, or a + b == 0
                        const int pa = __popc(xm & ~zmv), pb = __popc(zmv & ~xm);
                        const double tp = sT[pa * kShapT + pb], tn = -sT[pb * kShapT + pa];      // s - T[b][a] is s + (-T[b][a]), the same bits
                        touched |= df;
                        for (unsigned mm = df; mm; mm &= mm - 1u) {
                            const int e = __ffs((int)mm) - 1;
                            sS[e * D] = sS[e * D] + (((xm >> e) & 1u) ? tp : tn);
                        }
                    }
                }
                for (int e = 0; e < d; e++) {
                    if (!((touched >> e) & 1u)) continue;
                    const double se = sS[e * D];
                    sS[e * D] = 0.0;
                    const int s = el[e].slot - s0;
                    if ((unsigned)s < (unsigned)ns) sA[s * AS + tid] = sA[s * AS + tid] + (se * leaf.out) * W;
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < nd * ns; e += D) {                           // transposed: adjacent lanes, adjacent slots of one document
        const int dd = e / ns, s = e - dd * ns;
        double v = sA[s * AS + dd];
        if (a.last) v = (s0 + s == a.p.bias) ? a.bias : v / (double)a.B;
        a.p.out[(size_t)(d0 + dd) * a.p.slots + s0 + s] = v;
    }
}

static thread_local double g_iv_mask_ms = 0.0, g_iv_walk_ms = 0.0;     // the last call of this thread, device events
static thread_local int32_t g_iv_passes = 0;

}  // namespace rl

extern "C" {

int rl_model_predict_shap_background(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const float *BG, int32_t n_background,
                                     int32_t bg_stride, const int32_t *columns, int32_t n_columns, int64_t scratch_bytes, double *out)
{
    static const std::string w = "rl_model_predict_shap_background: ";
    std::string err;
    int rc = contrib_check_rows(w, m ? (int64_t)m->trees.size() : -1, X, n_docs, row_stride, err);
    if (!rc) rc = interv_check_background(w, BG, n_background, bg_stride, err);
    if (!rc) rc = contrib_check_columns(w, columns, n_columns, scratch_bytes, out, err);
    if (rc) return fail(rc, err);
    int32_t longest = 0;
    if (shap_check_paths(w, m->trees, &longest, err)) return fail(RL_ERR_UNSUPPORTED, err);
    SlotPlan sp = slot_plan(m, columns, n_columns);
    if (!interv_plan(longest, sp.slots, sp.docs, sp.per_pass)) return fail(RL_ERR_UNSUPPORTED, w + "the LDS has no room for one slot");
    g_iv_mask_ms = g_iv_walk_ms = 0.0;
    g_iv_passes = sp.passes();
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(m->device));
    const size_t T = m->trees.size();
    const int B = n_background, BS = interv_mask_stride(B);
    ShapPaths paths;
    std::vector<int32_t> slot((size_t)m->maxn);
    for (size_t t = 0; t < T; t++) {
        contrib_node_slots(m->trees[t], sp.sorted, (int32_t)sp.C, slot.data());
        shap_tree_paths(m->trees[t], nullptr, slot.data(), paths);
    }
    const std::vector<int32_t> cut = interv_tree_chunks(paths.leaf0, B, scratch_bytes);
    int64_t most_leaves = 1, most_trees = 1;
    for (size_t c = 0; c + 1 < cut.size(); c++) {
        most_leaves = std::max<int64_t>(most_leaves, paths.leaf0[(size_t)cut[c + 1]] - paths.leaf0[(size_t)cut[c]]);
        most_trees = std::max<int64_t>(most_trees, cut[c + 1] - cut[c]);
    }
    const std::vector<double> tb = interv_table();
    RowStream rows;
    int32_t *d_leaf0 = nullptr, *d_zleaf = nullptr; ShapLeaf *d_leaves = nullptr; ShapElem *d_elems = nullptr; ShapCond *d_conds = nullptr;
    double *d_tb = nullptr, *d_mt = nullptr; float *d_bg = nullptr; uint32_t *d_zm = nullptr;
    RL_HIP(rows.pool.upload(&d_leaf0, paths.leaf0.data(), paths.leaf0.size()));
    RL_HIP(rows.pool.upload(&d_leaves, paths.leaves.data(), paths.leaves.size()));
    RL_HIP(rows.pool.upload(&d_elems, paths.elems.data(), paths.elems.size()));
    RL_HIP(rows.pool.upload(&d_conds, paths.conds.data(), paths.conds.size()));
    RL_HIP(rows.pool.upload(&d_tb, tb.data(), tb.size()));
    RL_HIP(rows.pool.upload(&d_bg, BG, (size_t)B * bg_stride));
    RL_HIP(rows.pool.alloc(&d_zm, (size_t)most_leaves * BS));
    RL_HIP(rows.pool.alloc(&d_zleaf, (size_t)most_trees * B));
    RL_HIP(rows.pool.alloc(&d_mt, (size_t)most_trees));
    RL_HIP(hipFuncSetAttribute((const void *)k_model_interv, hipFuncAttributeMaxDynamicSharedMemorySize, kShapLds));
    IntervMaskArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.leaf0 = d_leaf0; ma.leaves = d_leaves; ma.elems = d_elems; ma.conds = d_conds; ma.BG = d_bg; ma.B = B; ma.BS = BS; ma.stride = bg_stride;
    ma.zm = d_zm; ma.zleaf = d_zleaf;
    IntervArgs a;
    memset(&a, 0, sizeof(a));
    a.leaf0 = d_leaf0; a.leaves = d_leaves; a.elems = d_elems; a.conds = d_conds; a.w = m->d_w; a.tb = d_tb; a.zm = d_zm; a.B = B; a.BS = BS;
    a.wd = longest;
    if ((rc = rows.open(n_docs, row_stride, scratch_bytes, (int64_t)row_stride * 4 + 8 * sp.slots))) return rc;
    RL_HIP(rows.pool.alloc(&a.p.out, (size_t)rows.chunk * sp.slots));
    a.p.X = rows.dX; a.p.stride = row_stride; a.p.slots = (int32_t)sp.slots; a.p.bias = (int32_t)(sp.C + 1);
    StageEvents ev;
    RL_HIP(ev.create());
    std::vector<double> mt((size_t)most_trees);
    double bias = 0.0;
    for (size_t c = 0; c + 1 < cut.size(); c++) {
        const int t0 = cut[c], t1 = cut[c + 1], ntc = t1 - t0;
        ma.t0 = t0; ma.ntc = ntc; ma.lbase = paths.leaf0[(size_t)t0];
        RL_HIP(hipEventRecord(ev.e[0], 0));
        hipLaunchKernelGGL(k_interv_masks, dim3((unsigned)((B + kThreads - 1) / kThreads), (unsigned)std::min(ntc, 65535)), dim3(kThreads), 0, 0, ma);
        RL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_interv_bias, dim3((unsigned)((ntc + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, (const ShapLeaf *)d_leaves,
                           (const int32_t *)d_zleaf, B, ntc, d_mt);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(ev.e[1], 0));
        RL_HIP(hipMemcpy(mt.data(), d_mt, (size_t)ntc * sizeof(double), hipMemcpyDeviceToHost));
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_iv_mask_ms += (double)ms;
        for (int t = 0; t < ntc; t++) bias = bias + mt[(size_t)t] * (double)m->trees[(size_t)(t0 + t)].weight;
        a.t0 = t0; a.t1 = t1; a.lbase = ma.lbase; a.first = c == 0; a.last = c + 2 == cut.size();
        a.bias = a.last ? bias / (double)B : 0.0;
        int64_t r0 = 0;
        rc = rows.run(X, n_docs, row_stride, [&](int64_t nr) -> int {
            if (!a.first) RL_HIP(hipMemcpy(a.p.out, out + (size_t)r0 * sp.slots, (size_t)nr * sp.slots * sizeof(double), hipMemcpyHostToDevice));
            r0 += nr;
            a.p.n = nr;
            for (int64_t s0 = 0; s0 < sp.slots; s0 += sp.per_pass) {
                a.p.s0 = (int32_t)s0; a.p.ns = (int32_t)std::min(sp.per_pass, sp.slots - s0);
                hipLaunchKernelGGL(k_model_interv, dim3((unsigned)((nr + sp.docs - 1) / sp.docs)), dim3(sp.docs),
                                   interv_lds_bytes(longest, sp.docs, a.p.ns), 0, a);
                RL_HIP(hipGetLastError());
            }
            return RL_OK;
        }, a.p.out, out, sp.slots);
        if (rc) return rc;
    }
    g_iv_walk_ms = rows.ms;
    m->last_path = RL_MODEL_PATH_INTERV;
    return RL_OK;
}

int rl_debug_interv_times(double *mask_ms, double *walk_ms)
{
    if (!mask_ms || !walk_ms) return fail(RL_ERR_INVALID, "rl_debug_interv_times: null argument");
    *mask_ms = g_iv_mask_ms;
    *walk_ms = g_iv_walk_ms;
    return RL_OK;
}

int rl_debug_interv_passes(int32_t *passes)
{
    if (!passes) return fail(RL_ERR_INVALID, "rl_debug_interv_passes: null argument");
    *passes = g_iv_passes;
    return RL_OK;
}

}  // extern "C"
