// rl_resume.inc -- a trainer adopts the trees of a saved model as its own first rounds (rl_adopt_model_text).  DESIGN.md 25.
// Included by rl_trainer.hip behind rl_init (it uses rl_trainer, launch_rank, enqueue_metric_mean, sync_rounds and model_from_text).
//
// A round leaves behind: the tree in t->ens, modelScores (the f64 chain  s += (double)lr * (double)output  in tree order from 0.0,
// LambdaMART.java:203-210), the validation scores (the same chain, :230-234), the ranked order of the training lists, the round's two
// float means and the early-stop state (:237-248).  All of it is a function of the trees and the data, so a trainer that REPLAYS the
// trees -- walk, add, rank, score, test, tree by tree -- stands where the trainer that grew them stood.
//
//   k_replay_scores<TILED>  one launch per data set and chunk of trees [t0, t1).  A block is ONE wavefront and owns tiles of kReplayDocs
//                           documents, a lane per document.  TILED: the tile's rows are staged once into LDS, transposed --
//                           sX[column][document], so a lane reads sX[c * 64 + lane]: the bank is the lane whatever column its path asks
//                           for (k_model_eval_tiled's layout) -- and every tree of the chunk is walked against LDS; the direct arm reads
//                           row[c] from global memory, a 4 F-byte lane stride, for every node of every tree.  A lane walks kReplayPer
//                           trees in lockstep (their node loads are issued together, no load sits inside a per-lane condition), then
//                           adds their outputs IN TREE ORDER to the f64 chain it keeps in a register.  The chain starts from
//                           d_scores[i], so chunks chain; after every tree it is stored to stage[tree - t0][i] (adjacent lanes, adjacent
//                           documents), after the chunk's last tree to d_scores[i].  A chain never leaves its lane: neither the chunk
//                           size nor the arm can change a bit.
//   No cross-block atomic, no spin wait, no inline assembly.  Built with -ffp-contract=off like the rest: the product is the double
//   product, the sum a separate add.
namespace rl {

constexpr int kReplayDocs = 64;                                  // documents per tile = lanes of a block
constexpr int kReplayPer = 4;                                    // trees a lane walks in lockstep
constexpr size_t kReplayLdsMax = (size_t)160 * 1024;             // F <= 640 columns fit a tile
constexpr int64_t kReplayScratchDefault = (int64_t)256 << 20;    // scratch_bytes == 0

template <bool TILED>
__global__ __launch_bounds__(kReplayDocs) void k_replay_scores(const EnsTree e, int MAXN, int t0, int t1, const float *X, int64_t n, int F,
                                                                float lr, double *scores, double *stage)
{
    extern __shared__ float rp_sX[];                             // TILED: [F][kReplayDocs]
    const int lane = threadIdx.x;
    const int64_t tiles = (n + kReplayDocs - 1) / kReplayDocs;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t d0 = tile * kReplayDocs;
        const int nd = (int)min((int64_t)kReplayDocs, n - d0);
        if (TILED) {
            __syncthreads();                                     // the previous tile has been walked
            const float *src = X + (size_t)d0 * F;               // the tile is one contiguous range of X
            for (int i = lane; i < nd * F; i += kReplayDocs) { const int dd = i / F, c = i - dd * F; rp_sX[c * kReplayDocs + dd] = src[i]; }
            __syncthreads();
        }
        const bool live = lane < nd;
        const int dl = live ? lane : 0;                          // (idle lanes of the last tile walk document d0 again and store nothing)
        const float *row = X + (size_t)(d0 + dl) * F;
        double s = scores[d0 + dl];
        for (int tb = t0; tb < t1; tb += kReplayPer) {
            size_t o[kReplayPer]; int node[kReplayPer];
#pragma unroll
            for (int u = 0; u < kReplayPer; u++) { o[u] = (size_t)min(tb + u, t1 - 1) * MAXN; node[u] = 0; }      // (past the chunk: its last tree again, unstored)
            for (;;) {
                int f[kReplayPer], le[kReplayPer], ri[kReplayPer]; float th[kReplayPer], v[kReplayPer];
#pragma unroll
                for (int u = 0; u < kReplayPer; u++) {
                    f[u] = e.feat_idx[o[u] + node[u]]; th[u] = e.thr[o[u] + node[u]]; le[u] = e.left[o[u] + node[u]]; ri[u] = e.right[o[u] + node[u]];
                }
#pragma unroll
                for (int u = 0; u < kReplayPer; u++) v[u] = TILED ? rp_sX[max(f[u], 0) * kReplayDocs + dl] : row[max(f[u], 0)];
                bool any = false;
#pragma unroll
                for (int u = 0; u < kReplayPer; u++)
                    if (f[u] >= 0) { node[u] = (v[u] <= th[u]) ? le[u] : ri[u]; any = true; }      // Split.eval: value <= threshold goes left (Split.java:118)
                if (!any) break;
            }
#pragma unroll
            for (int u = 0; u < kReplayPer; u++)
                if (tb + u < t1) {
                    s += (double)lr * (double)e.out[o[u] + node[u]];                                // LambdaMART.java:208 / :232
                    if (live) stage[(size_t)(tb + u - t0) * n + d0 + lane] = s;
                }
        }
        if (live) scores[d0 + lane] = s;
    }
}

static bool replay_tiled_ok(const rl_trainer *t) { return (size_t)t->F * kReplayDocs * sizeof(float) <= kReplayLdsMax && !t->knobs.replay_direct; }

static void launch_replay(rl_trainer *t, DataSet &d, int t0, int t1, double *stage)
{
    const int64_t tiles = (d.N + kReplayDocs - 1) / kReplayDocs;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, (int64_t)1 << 20));
    if (replay_tiled_ok(t)) {
        t->arms[RL_ARM_REPLAY_TILED]++;
        hipLaunchKernelGGL(k_replay_scores<true>, grid, dim3(kReplayDocs), (size_t)t->F * kReplayDocs * sizeof(float), t->stream, t->ens, t->ctx.MAXN, t0, t1,
                           (const float *)d.d_X, (int64_t)d.N, t->F, t->ctx.lr, d.d_scores, stage);
    } else {      // more columns than a tile holds (F > 640), or RLHIP_REPLAY_DIRECT
        t->arms[RL_ARM_REPLAY_DIRECT]++;
        hipLaunchKernelGGL(k_replay_scores<false>, grid, dim3(kReplayDocs), 0, t->stream, t->ens, t->ctx.MAXN, t0, t1, (const float *)d.d_X, (int64_t)d.N, t->F,
                           t->ctx.lr, d.d_scores, stage);
    }
}

// the trees as the trainer keeps them: t->ens, node i of tree r at [r * MAXN + i], feature ids as columns.  The text's pre-order is a
// creation order like any other to the walks; count / deviance are diagnostics the text does not hold: -1 / NaN
static int upload_adopted(rl_trainer *t, const std::vector<HostTree> &trees, const std::map<int32_t, int32_t> &col_of)
{
    const int MAXN = t->ctx.MAXN;
    const size_t T0 = trees.size(), en = T0 * MAXN;
    std::vector<int32_t> fi(en, -1), le(en, -1), ri(en, -1), cn(en, -1), nn(T0);
    std::vector<float> th(en, 0.f), ou(en, 0.f);
    std::vector<double> dv(en, std::numeric_limits<double>::quiet_NaN());
    for (size_t r = 0; r < T0; r++) {
        const HostTree &h = trees[r];
        nn[r] = h.n_nodes;
        for (int j = 0; j < h.n_nodes; j++) {
            const size_t o = r * MAXN + j;
            const bool leaf = h.feature[j] == -1;
            fi[o] = leaf ? -1 : col_of.at(h.feature[j]);
            th[o] = leaf ? 0.f : h.threshold[j]; le[o] = leaf ? -1 : h.left[j]; ri[o] = leaf ? -1 : h.right[j]; ou[o] = leaf ? h.output[j] : 0.f;
        }
    }
    RL_HIP(hipMemcpy(t->ens.feat_idx, fi.data(), en * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(t->ens.left, le.data(), en * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(t->ens.right, ri.data(), en * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(t->ens.count, cn.data(), en * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(t->ens.thr, th.data(), en * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(t->ens.out, ou.data(), en * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(t->ens.deviance, dv.data(), en * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(t->ens.n_nodes, nn.data(), T0 * sizeof(int32_t), hipMemcpyHostToDevice));
    return RL_OK;
}

// what rl_adopt_model_text and rl_refit_model_text (rl_refit.inc) ask of a handle and a text before anything is uploaded; `w` opens every message
static int check_adoptable(rl_trainer *t, const std::string &w, const char *text, bool refit, std::vector<HostTree> &trees, std::map<int32_t, int32_t> &col_of)
{
    if (!text) return fail(RL_ERR_INVALID, w + "null text");
    if (!t->inited) return fail(RL_ERR_STATE, w + "rl_init has not been called");
    if (t->finished) return fail(RL_ERR_STATE, w + "rl_finish has been called");
    if (t->round != 0) return fail(RL_ERR_STATE, w + "a model is " + (refit ? "refitted" : "adopted") + " before the first round (this trainer has " + std::to_string(t->round) + ")");
    if (t->dist) return fail(RL_ERR_UNSUPPORTED, w + "a sharded trainer cannot " + (refit ? "refit a model (the routing is not built for shards)" : "adopt a model (the replay is not built for shards)"));
    std::string err;
    if (!model_from_text(text, trees, err)) return fail(RL_ERR_INVALID, w + "Error in Emsemble(xmlRepresentation): " + err);
    {   // one <ensemble>: the parser stops behind the first
        const std::string s(text);
        const size_t first = s.find("<ensemble>");
        if (first != std::string::npos && s.find("<ensemble>", first + 1) != std::string::npos)
            return fail(RL_ERR_INVALID, w + "the text holds more than one <ensemble> (a Random Forests model: every bag is a trainer of its own)");
    }
    const int T0 = (int)trees.size(), MAXN = t->ctx.MAXN;
    if (trees.empty()) return fail(RL_ERR_INVALID, w + "the model has no trees");
    if (trees.size() > (size_t)t->p.n_trees)
        return fail(RL_ERR_INVALID, w + "the model has " + std::to_string(trees.size()) + " trees, the trainer's n_trees is " + std::to_string(t->p.n_trees) +
                                    " (-tree is the total number of trees)");
    for (int f = 0; f < t->F; f++) col_of.emplace(t->feature_ids[f], f);       // (a repeated id: its first column)
    for (int r = 0; r < T0; r++) {
        const HostTree &h = trees[r];
        if (h.n_nodes > MAXN)
            return fail(RL_ERR_INVALID, w + "tree " + std::to_string(r) + " has " + std::to_string(h.n_nodes) + " nodes, the trainer's tree capacity is " +
                                        std::to_string(MAXN) + " (-leaf too small for this model)");
        for (int j = 0; j < h.n_nodes; j++) {
            const bool split = h.left[j] >= 0;
            if (split && !col_of.count(h.feature[j]))
                return fail(RL_ERR_INVALID, w + "tree " + std::to_string(r) + " splits on feature " + std::to_string(h.feature[j]) + ", which is not among the trainer's feature_ids");
            if (!split && h.feature[j] != -1) return fail(RL_ERR_INVALID, w + "tree " + std::to_string(r) + " has a split without children (internal error)");
        }
        uint32_t wb, lb;
        memcpy(&wb, &h.weight, 4); memcpy(&lb, &t->p.learning_rate, 4);
        if (wb != lb)
            return fail(RL_ERR_INVALID, w + "tree " + std::to_string(r) + " has weight " + java_float_to_string(h.weight) + ", the trainer's learning_rate is " +
                                        java_float_to_string(t->p.learning_rate) + " (per-tree weights are not built: resume under the shrinkage the model was trained with)");
    }
    return RL_OK;
}

// behind the last of T0 adopted or refitted rounds: everything keyed by the index of a tree moves on by T0 -- the round counter, the trees kept, the
// device's count of trees started (the seeded feature draw of a split attempt is keyed by it: root_hash) and the host's mirror of it -- then the
// rounds' metrics come to the host, best_round / best_score are rebuilt and *stop is the test of :248 at round T0 - 1
static int settle_adopted(rl_trainer *t, int T0, int32_t *stop)
{
    Ctx &c = t->ctx;
    int32_t seq = 0;
    RL_HIP(hipStreamSynchronize(t->stream));
    RL_HIP(hipMemcpy(&seq, &c.st->tree_seq, sizeof(seq), hipMemcpyDeviceToHost));
    seq += T0;
    RL_HIP(hipMemcpy(&c.st->tree_seq, &seq, sizeof(seq), hipMemcpyHostToDevice));
    t->tree_seq += (uint32_t)T0;
    t->round = T0; t->n_kept = T0;
    int rc = sync_rounds(t);       // the rounds' metrics -> h_metrics, synced_rounds = T0
    if (rc) return rc;
    if (t->has_valid)              // rl_boost_round's strict > over the rounds in order (LambdaMART.java:237-243)
        for (int r = 0; r < T0; r++) {
            const double score = t->h_metrics[2 * (size_t)r + 1];
            if (score > t->best_score) { t->best_score = score; t->best_round = r; }
        }
    if (stop) *stop = ((T0 - 1) - t->best_round > t->p.early_stop_rounds) ? 1 : 0;      // :248 at round T0 - 1
    return RL_OK;
}

}  // namespace rl

extern "C" int rl_adopt_model_text(rl_trainer *t, const char *text, int64_t scratch_bytes, int32_t *stop)
{
    const std::string w = "rl_adopt_model_text: ";
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (scratch_bytes < 0) return fail(RL_ERR_INVALID, w + "scratch_bytes must be >= 0");
    std::vector<HostTree> trees;
    std::map<int32_t, int32_t> col_of;
    int rc = check_adoptable(t, w, text, false, trees, col_of);
    if (rc) return rc;
    const int T0 = (int)trees.size();
    RL_HIP(hipSetDevice(t->p.device));
    RL_HIP(hipStreamSynchronize(t->stream));
    rc = upload_adopted(t, trees, col_of);
    if (rc) return rc;
    // stage scratch: 8 bytes per document and tree, both data sets; at least one tree per chunk
    const int64_t per_tree = 8 * ((int64_t)t->tr.N + (t->has_valid ? (int64_t)t->va.N : 0));
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(T0, (scratch_bytes ? scratch_bytes : kReplayScratchDefault) / per_tree));
    DevPool scratch;
    double *st_tr = nullptr, *st_va = nullptr;
    RL_HIP(scratch.alloc(&st_tr, (size_t)chunk * t->tr.N));
    if (t->has_valid) RL_HIP(scratch.alloc(&st_va, (size_t)chunk * t->va.N));
    RL_HIP(hipFuncSetAttribute((const void *)k_replay_scores<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kReplayLdsMax));
    Ctx &c = t->ctx;
    for (int t0 = 0; t0 < T0; t0 += chunk) {
        const int t1 = std::min(T0, t0 + chunk);
        launch_replay(t, t->tr, t0, t1, st_tr);
        if (t->has_valid) launch_replay(t, t->va, t0, t1, st_va);
        RL_HIP(hipGetLastError());
        for (int r = t0; r < t1; r++) {      // what enqueue_scores_and_metrics does behind a round's score update, on that round's scores
            rc = launch_rank(t, t->tr, st_tr + (size_t)(r - t0) * t->tr.N, t->tr.d_ndcg, r == T0 - 1);      // the last tree: the ranking of round T0's lambdas
            if (rc) return rc;
            enqueue_metric_mean(t, t->tr.d_ndcg, t->tr.Q, c.round_metric + 2 * (size_t)r);
            if (t->has_valid) {
                rc = launch_rank(t, t->va, st_va + (size_t)(r - t0) * t->va.N, t->va.d_ndcg, false);
                if (rc) return rc;
                enqueue_metric_mean(t, t->va.d_ndcg, t->va.Q, c.round_metric + 2 * (size_t)r + 1);
            }
        }
        RL_HIP(hipGetLastError());
    }
    return settle_adopted(t, T0, stop);
}
