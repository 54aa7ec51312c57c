// rl_k_ensemble.inc -- K10: the grown tree joins the ensemble, and the ensemble is evaluated on raw rows (Ensemble.java:110-116,
// Split.java:115-125, LambdaMART.java:230-234).  EnsTree, k_export_tree, k_valid_update, k_ensemble_eval (k_model_eval* live in rl_model_eval.inc).
// Included by rl_kernels_round.inc; needs nothing of that file and none of the other pieces.

namespace rl {

// ------------------------------------------------------------------------------------------------
// tree bookkeeping: copy the grown tree into the ensemble (creation order), evaluate it on raw rows
// ------------------------------------------------------------------------------------------------
struct EnsTree {   // device layout of one kept tree, node i at [tree*MAXN + i]
    int32_t *feat_idx;   // column index, -1 = leaf
    float *thr;
    int32_t *left, *right;
    float *out;
    int32_t *n_nodes;    // [n_trees]
    int32_t *count;      // training samples per node (diagnostic)
    double *deviance;
};

__global__ __launch_bounds__(kThreads) void k_export_tree(const Ctx c, const EnsTree e, int tree)
{   // only committed nodes (fid >= 0) are part of the tree; fid = creation order of the committed splits
    const TreeState *st = c.st;
    const int nn = st->n_nodes;
    for (int i = threadIdx.x; i < nn; i += kThreads) {
        const NodeRec &X = c.nodes[i];
        if (X.fid < 0) continue;
        const size_t o = (size_t)tree * c.MAXN + X.fid;
        const bool leaf = X.left < 0;
        e.feat_idx[o] = leaf ? -1 : (c.vcol ? c.vcol[X.best_f] : X.best_f);          // the column of the row matrix (a virtual feature's real column)
        e.thr[o] = leaf ? 0.f : c.thr[(size_t)X.best_f * c.TS + X.best_t];
        e.left[o] = leaf ? -1 : c.nodes[X.left].fid; e.right[o] = leaf ? -1 : c.nodes[X.right].fid;
        e.out[o] = leaf ? X.output : 0.f;
        e.count[o] = X.gcount;
        e.deviance[o] = X.deviance;
    }
    if (threadIdx.x == 0) e.n_nodes[tree] = 2 * st->n_splits + 1;
}

// Split.eval (Split.java:115-125) of tree `tree` on row-major rows; adds lr*out to the running double
// scores of the validation set (LambdaMART.java:230-234).
__global__ __launch_bounds__(kThreads) void k_valid_update(const EnsTree e, int MAXN, int tree, const float *X, int n, int F,
                                                            float lr, double *vscores)
{
    const size_t o = (size_t)tree * MAXN;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const float *row = X + (size_t)i * F;
        int nd = 0;
        while (e.feat_idx[o + nd] != -1) nd = (row[e.feat_idx[o + nd]] <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
        vscores[i] += (double)lr * (double)e.out[o + nd];
    }
}

// Ensemble.eval (Ensemble.java:110-116): float s; s += tree.eval(dp) * weight   for trees 0..nt-1.
// rows: row-major [n][stride]; column of feature index f is colmap ? colmap[f] : f.
__global__ __launch_bounds__(kThreads) void k_ensemble_eval(const EnsTree e, int MAXN, int nt, const float *X, int64_t n,
                                                             int stride, float w, float *out, double *out_d)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float *row = X + (size_t)i * stride;
        float s = 0.f;
        for (int t = 0; t < nt; t++) {
            const size_t o = (size_t)t * MAXN;
            int nd = 0;
            while (e.feat_idx[o + nd] != -1) {
                const int fc = e.feat_idx[o + nd];
                const float v = (fc < stride) ? row[fc] : 0.f;
                nd = (v <= e.thr[o + nd]) ? e.left[o + nd] : e.right[o + nd];
            }
            s = (float)((double)s + (double)e.out[o + nd] * (double)w);
        }
        if (out) out[i] = s;
        if (out_d) out_d[i] = (double)s;
    }
}

}  // namespace rl
