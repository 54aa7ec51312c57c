// rl_trainer.hip -- host orchestration + C ABI of librlhip.so (see include/rlhip.h): the translation unit's includes, `struct rl_trainer`, the
// timing helpers, the small helpers between the stages, and the extern "C" entries.  Every multi-stage host sequence has a file of its own,
// included where it is needed: rl_chain_host.inc (float chains), rl_launch.inc (the k_rank_* / k_hist launchers), rl_tie_host.inc
// (resolve_ties), rl_round.inc (enqueue_round), rl_init.inc (rl_init).
//
// One handle = one GPU = one HIP stream.  After rl_init everything a boosting round needs is resident in
// HBM; a round is a fixed sequence of kernel launches with NO host synchronisation inside it: the tree is
// grown by device-side state (TreeState / NodeRec), the host only enqueues "one more split step" L-1 times.
//
// There is no CPU fallback anywhere in this file: without a gfx950 device rl_create fails with
// RL_ERR_NO_DEVICE.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>

#include "rl_internal.h"
#include "rl_lists_host.h"
#include "rl_knobs.h"
#include "rl_device.h"
#include "rl_wave.h"
#include "rl_kernels_init.inc"
#include "rl_chain.inc"
#include "rl_kernels_round.inc"
#include "rl_fast_leaf.inc"
#include "rl_step2.inc"
#include "rl_java_order.inc"
#include "rl_csc.inc"
#include "rl_tie.inc"
#include "rl_membench.inc"
#include "rl_dist.inc"
#include "rl_model.h"

namespace rl {

static thread_local std::string g_err;
static double g_err_max = 16.0;      // ERRScorer.MAX: a process-wide static in the reference as well (metric/ERRScorer.java:25)
void set_error(const std::string &msg) { g_err = msg; }
int fail(int code, const std::string &msg) { g_err = msg; return code; }

struct DataSet : ListSetHost {     // the host side (labels, qoff, qkey, the -qrel tables of rl_set_external_judgments): rl_lists_host.h
    float *d_X = nullptr;          // row-major rows [N][F]
    int64_t rows_next = -1;        // chunked upload (rl_set_rows): next row expected; -1 = the rows came with rl_set_train / rl_set_validation
    float *d_labels = nullptr; int32_t *d_qoff = nullptr; double *d_ideal0 = nullptr, *d_ideal1 = nullptr;
    double *d_scores = nullptr, *d_ndcg = nullptr;
    double *d_ss = nullptr; float *d_sl = nullptr; int32_t *d_srel = nullptr, *d_sidx = nullptr, *d_docq = nullptr;   // ranked order (training set only)
    int32_t *d_aux_i = nullptr; double *d_aux_a = nullptr, *d_aux_b = nullptr;   // swapChange tables of MAP / ERR in ranked order
    int32_t *d_ext_rd = nullptr;   // ext_rd on the device (null: none given)
    int32_t *d_qsmall = nullptr, *d_qbig = nullptr, *d_qtiny = nullptr; int32_t n_small = 0, n_big = 0, n_tiny = 0, max_big = 0, n_small_long = 0; bool all_small = false;
    int32_t *d_qhuge = nullptr, *d_relscratch = nullptr; int32_t n_huge = 0;      // lists beyond kLambdaBlockCap documents (k_rank_huge)
    // queries by length class for the fused lambda kernel: <= 64, <= 128, <= 192 documents, longer (tiled by 256); a block is as
    // wide as its class, so short lists do not leave most of a block idle
    int32_t *d_qcls[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; int32_t n_qcls[5] = {0, 0, 0, 0, 0};     // [4]: <= 16 documents (k_lambda_tiny)
};

struct TimingSlot { double ms = 0; int64_t launches = 0; double bytes = 0; };

}  // namespace rl

using namespace rl;

struct rl_trainer {
    rl_params p;
    Knobs knobs;                       // every RLHIP_* knob, read once by rl_create (rl_knobs.h)
    int32_t F = 0;
    std::vector<int32_t> feature_ids;
    std::vector<int32_t> vcol;         // histogram (virtual) feature -> column of the row matrix; empty = identity (rl_init: tables beyond 4095 entries)
    DataSet tr, va;
    bool has_train = false, has_valid = false, inited = false, finished = false;
    hipStream_t stream = nullptr;
    // the per-round training metric (a float chain over the queries) is off the critical path of the next round: it runs
    // on a side stream between two events (single-GPU runs without a validation set)
    hipStream_t side = nullptr; hipEvent_t ev_ranked = nullptr, ev_metric = nullptr; bool side_pending = false;
    // the lambda kernels of the list-length classes are independent: three of them run on streams of their own beside the main one, so that the tail
    // of one class (its last blocks) overlaps the next class instead of idling the chip (knobs.lam_side of them are used)
    hipStream_t lam_s[3] = {nullptr, nullptr, nullptr}; hipEvent_t ev_lam_fork = nullptr, ev_lam_join[3] = {nullptr, nullptr, nullptr};
    DevPool pool;
    Ctx ctx;
    EnsTree ens;
    int32_t L_eff = 0;          // leaf budget in force: n_leaves, or floor(N / min_leaf_support) for -leaf -1
    int32_t *d_tie_flag = nullptr;                    // sharded tie-break: the ranks' common out-of-memory decision (resolve_ties)
    int64_t sp_entries = 0; int32_t sp_cols = 0;      // sparse-column path of the root pass (rl_csc.inc)
    int32_t cr_groups = 0; double cr_entries = 0, cr_overflow = 0;          // compact rows (groups that use them; of the child passes (k_compact_rows): entries outside the mode bins, rows that need the dense fallback
    double err_max = 16.0;      // ERRScorer.MAX when the trainer was created (rl_set_err_max)
    int32_t round = 0;          // rounds enqueued so far
    int64_t refit_stats[3] = {0, 0, 0};    // rl_debug_refit_stats: k_refit_route launches through the LDS tile / from global memory, leaves that kept their old output
    int64_t arms[RL_ARM_COUNT_] = {};      // RL_ARR_LAUNCH_ARMS: launches per kernel variant, counted where the host picks one (the tests assert the variant a knob selects)
    // growth progress reported by the device (Ctx::progress): the host keeps at most knobs.step_ahead growth steps in flight and
    // stops enqueuing steps of a finished tree; 0 = enqueue all L-1 steps blindly
    // (1: c2 409.5 -> 411.7 rounds/s against 3, profiles/r05g_ab_step_ahead_c2.txt -- fewer empty steps behind a finished tree)
    // sharded runs, knobs.dist_ahead: growth steps enqueued beyond the last one whose bookkeeping the host has seen -- 0: every enqueued step has work (an empty
    // step still costs its all-reduce on every rank)
    unsigned long long *h_progress = nullptr; uint32_t tree_seq = 0;
    unsigned long long chain_seq = 0; std::vector<void *> pinned;     // chain pass tags; pinned words of the chains (freed in rl_destroy)
    int32_t synced_rounds = 0;
    long long tie_stalls = 0, tie_nodes = 0, tie_chain_nodes = 0, tie_chain_docs = 0;      // lazy tie-break (rl_tie.inc): resolutions run, nodes resolved, chain nodes / documents summed
    long long tie_batches = 0;      // of the resolutions, the batched ones at the end of a tree (deferred ties)
    bool fin_split = false;      // wide data: k_hist_finish_wide + k_select instead of the fused finish (rl_init)
    long long tie_phase_us[6] = {0, 0, 0, 0, 0, 0};   // knobs.tie_prof: host microseconds per phase of resolve_ties (printed by rl_destroy)
    long long chain_calls[2] = {0, 0}, chain_repairs[2] = {0, 0}, chain_timeouts = 0, chain_wait_us = 0;      // knobs.chain_prof: float-chain evaluations [hinted, blind], repair passes enqueued, progress-word time-outs, host microseconds spent waiting for a stitch
    long long tie_regrown = 0;      // trees grown a second time because a deferred tie over several features hid two different cuts (k_tie_verify)
    long long tie_us = 0, tie_spec_segs = 0, tie_spec_miss = 0, tie_spec_serial = 0, tie_spec_repairs = 0;      // host time in resolve_ties; segments evaluated, window misses, serial segments, repair passes
    std::vector<int32_t> h_nthr; std::vector<char> tie_blob;
    void *tie_pin = nullptr; size_t tie_pin_cap = 0;                                          // pinned staging of its small device-to-host reads
    void *tie_buf = nullptr; size_t tie_cap = 0, tie_hint = 0;                                              // scratch arena of resolve_ties (only ever grows)
    int32_t n_kept = 0;         // trees kept after rollback (== round until rl_finish)
    int32_t best_round = 2147483647 - 2;     // LambdaMART.bestModelOnValidation  LambdaMART.java:50
    double best_score = 0.0;                 // Ranker.bestScoreOnValidationData  Ranker.java:43
    std::vector<float> h_metrics;            // [round][2]
    std::vector<HostTree> trees;             // host copies (pre-order), fetched lazily
    float *d_final_f = nullptr; double *d_final_d = nullptr, *d_mean = nullptr;
    ChainBufs leaf_chain, metric_chain;      // exact parallel float chains (rl_chain.inc)
    int32_t *d_seg_buf = nullptr;
    double2 *d_fast_part = nullptr, *d_fast_sums = nullptr; int64_t fast_slots = 0;      // RL_FLAG_FAST_LEAF (rl_fast_leaf.inc): tile partials [fast_slots], R of every leaf [MAXN + 1]
    double2 *d_T = nullptr;                  // pair terms of the lambda computation [N][k]
    double *d_wmax = nullptr;                // per-block max |lambda| of the lambda launches
    float *d_vmetric = nullptr;
    // timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending[RL_KERNEL_COUNT_];
    std::vector<double> ev_bytes[RL_KERNEL_COUNT_];
    std::vector<hipEvent_t> ev_free;
    TimingSlot timing[RL_KERNEL_COUNT_];
    // distributed (rl_dist.inc)
    int32_t rank = 0, n_ranks = 1;
    std::unique_ptr<DistBackend> dist;
    std::vector<int32_t> all_N, all_Q;        // local sizes of every rank
    int64_t Nglobal = 0; int32_t Qglobal = 0, Qmax = 0;
    ChainBufs gchain;                          // float chains over the all-gathered leaf values
    double *d_gx = nullptr, *d_send = nullptr; int32_t *d_gls = nullptr; int32_t lsstride = 0; float *d_gres = nullptr;     // leaf-owner exchange: receive / send buffers
    int32_t *d_own = nullptr; long long *d_xtab = nullptr;     // owner of every leaf; pack / assemble offsets (rl_dist.inc LeafExchange)
    std::vector<int32_t> h_gls, h_own; std::vector<long long> h_xtab;
    // round 6, distributed float chains (rl_dist.inc "piece mode"; knobs.dist_owner_chains: the leaf-owner exchange instead)
    bool piece_chains = false; double *d_pc_loc = nullptr, *d_pc_all = nullptr, *d_pc_base = nullptr; uint32_t *d_ptab = nullptr, *d_gtab = nullptr, *d_res_loc = nullptr, *d_res_all = nullptr;
    CrossState xstate{nullptr, nullptr, nullptr}; long long piece_rounds = 0, piece_misses = 0;
    long long *h_xmail = nullptr, *d_xmail = nullptr, xmail_tag = 0;     // pinned mailbox of k_plan_exchange (transfer sizes of the leaf-owner exchange): no stream synchronisation in a round
    double *d_qsend = nullptr, *d_qgath = nullptr, *d_qcat = nullptr; int32_t *d_allQ = nullptr;
    // the same for the validation set (sharded by query like the training set)
    int32_t vQglobal = 0, vQmax = 0; double *d_vqsend = nullptr, *d_vqgath = nullptr, *d_vqcat = nullptr; int32_t *d_vallQ = nullptr;
};

namespace rl {

static int check_trainer(const rl_trainer *t) { return t ? RL_OK : fail(RL_ERR_INVALID, "null trainer handle"); }

static int validate_dataset(const float *X, int64_t n, int32_t F, const float *labels, const int32_t *qoff, int32_t Q)
{
    if (!labels || !qoff) return fail(RL_ERR_INVALID, "null data pointer");       // X == NULL: the rows follow through rl_set_rows
    if (n <= 0 || Q <= 0 || F <= 0) return fail(RL_ERR_INVALID, "There are no training samples / features");
    if (n >= (int64_t)2147483647 - 4096) return fail(RL_ERR_UNSUPPORTED, "more than 2^31 documents per GPU");
    std::string err;
    const int rc = check_lists("", labels, n, qoff, Q, err);
    return rc ? fail(rc, err) : RL_OK;
}

static int load_dataset(rl_trainer *t, DataSet &d, const float *X, int64_t n, const float *labels, const int32_t *qoff,
                        int32_t Q, const int32_t *qkey)
{
    d.store(labels, n, qoff, Q, qkey);
    RL_HIP(t->pool.alloc(&d.d_X, (size_t)n * t->F));
    if (X) { RL_HIP(hipMemcpy(d.d_X, X, (size_t)n * t->F * sizeof(float), hipMemcpyHostToDevice)); d.rows_next = -1; }
    else d.rows_next = 0;
    return RL_OK;
}

static int upload_query_side(rl_trainer *t, DataSet &d, const std::vector<double> &ideal0, const std::vector<double> &ideal1)
{
    RL_HIP(t->pool.alloc(&d.d_labels, (size_t)d.N));
    RL_HIP(hipMemcpy(d.d_labels, d.labels.data(), d.N * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(t->pool.alloc(&d.d_qoff, (size_t)d.Q + 1));
    RL_HIP(hipMemcpy(d.d_qoff, d.qoff.data(), ((size_t)d.Q + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(t->pool.alloc(&d.d_ideal0, (size_t)d.Q));
    RL_HIP(t->pool.alloc(&d.d_ideal1, (size_t)d.Q));
    RL_HIP(hipMemcpy(d.d_ideal0, ideal0.data(), d.Q * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d.d_ideal1, ideal1.data(), d.Q * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(t->pool.alloc(&d.d_scores, (size_t)d.N));
    RL_HIP(hipMemset(d.d_scores, 0, d.N * sizeof(double)));                // modelScores = 0  LambdaMART.java:86
    RL_HIP(t->pool.alloc(&d.d_ndcg, (size_t)d.Q));
    const size_t tiny_min = (size_t)t->knobs.tiny_min;           // lists of <= 16 documents get kernels of their own when there are enough of them
    std::vector<int32_t> small, big, tiny, huge;
    for (int32_t q = 0; q < d.Q; q++) {
        const int n = d.qoff[q + 1] - d.qoff[q];
        (n <= kRankTinyDocs ? tiny : n <= kLambdaWaveCap ? small : n <= kLambdaBlockCap ? big : huge).push_back(q);
    }
    d.n_huge = (int32_t)huge.size();
    if (!huge.empty()) {
        RL_HIP(t->pool.alloc(&d.d_qhuge, huge.size()));
        RL_HIP(hipMemcpy(d.d_qhuge, huge.data(), huge.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        RL_HIP(t->pool.alloc(&d.d_relscratch, (size_t)d.N));
    }
    if (tiny.size() < tiny_min) { small.insert(small.end(), tiny.begin(), tiny.end()); tiny.clear(); }
    d.n_tiny = (int32_t)tiny.size();
    RL_HIP(t->pool.alloc(&d.d_qtiny, tiny.size()));
    if (!tiny.empty()) RL_HIP(hipMemcpy(d.d_qtiny, tiny.data(), tiny.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    // longest first: a block's work grows with n (n^2 for the rank), so late long lists would leave a tail
    auto by_len = [&](int32_t a, int32_t b) { return (d.qoff[a + 1] - d.qoff[a]) > (d.qoff[b + 1] - d.qoff[b]); };
    std::stable_sort(small.begin(), small.end(), by_len);
    std::stable_sort(big.begin(), big.end(), by_len);
    d.n_small = (int32_t)small.size(); d.n_big = (int32_t)big.size();
    d.n_small_long = 0;
    for (int32_t q : small) d.n_small_long += (d.qoff[q + 1] - d.qoff[q] > kRankShort) ? 1 : 0;
    d.max_big = big.empty() ? 0 : (((d.qoff[big[0] + 1] - d.qoff[big[0]]) + 63) & ~63);      // (longest first) what k_rank_block's LDS is sized for
    d.all_small = false;      // the lists are permutations now: always index through them
    RL_HIP(t->pool.alloc(&d.d_qsmall, small.size()));
    RL_HIP(t->pool.alloc(&d.d_qbig, big.size()));
    if (!small.empty()) RL_HIP(hipMemcpy(d.d_qsmall, small.data(), small.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!big.empty()) RL_HIP(hipMemcpy(d.d_qbig, big.data(), big.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    std::vector<int32_t> qcls[5];
    for (int32_t q = 0; q < d.Q; q++) {
        const int n = d.qoff[q + 1] - d.qoff[q];
        qcls[n <= kLambdaTinyDocs ? 4 : n <= 64 ? 0 : n <= 128 ? 1 : n <= 192 ? 2 : 3].push_back(q);
    }
    if (qcls[4].size() < tiny_min) {   // a handful of tiny lists is not worth a launch of its own: they join the 64-wide class
        qcls[0].insert(qcls[0].end(), qcls[4].begin(), qcls[4].end());
        qcls[4].clear();
    }
    for (int cI = 0; cI < 5; cI++) {
        std::stable_sort(qcls[cI].begin(), qcls[cI].end(), by_len);
        d.n_qcls[cI] = (int32_t)qcls[cI].size();
        RL_HIP(t->pool.alloc(&d.d_qcls[cI], qcls[cI].size()));
        if (!qcls[cI].empty()) RL_HIP(hipMemcpy(d.d_qcls[cI], qcls[cI].data(), qcls[cI].size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return RL_OK;
}

static int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// ---- timing helpers ----------------------------------------------------------------------------
static hipEvent_t take_event(rl_trainer *t)
{
    if (!t->ev_free.empty()) { hipEvent_t e = t->ev_free.back(); t->ev_free.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
struct ScopedTiming {
    rl_trainer *t; int which; hipEvent_t a = nullptr, b = nullptr; bool on;
    ScopedTiming(rl_trainer *t_, int which_, double bytes)
        : t(t_), which(which_), on((t_->p.flags & (which_ == RL_KERNEL_HIST_NODE ? RL_FLAG_TIMING_NODES : RL_FLAG_TIMING)) != 0)
    {
        if (!on) return;
        a = take_event(t); b = take_event(t);
        (void)hipEventRecord(a, t->stream);
        t->ev_bytes[which].push_back(bytes);
    }
    ~ScopedTiming() { if (on) { (void)hipEventRecord(b, t->stream); t->ev_pending[which].push_back({a, b}); } }
};
static void collect_timing(rl_trainer *t)
{
    for (int w = 0; w < RL_KERNEL_COUNT_; w++) {
        for (size_t i = 0; i < t->ev_pending[w].size(); i++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, t->ev_pending[w][i].first, t->ev_pending[w][i].second) == hipSuccess) {
                t->timing[w].ms += ms; t->timing[w].launches++; t->timing[w].bytes += t->ev_bytes[w][i];
            }
            t->ev_free.push_back(t->ev_pending[w][i].first); t->ev_free.push_back(t->ev_pending[w][i].second);
        }
        t->ev_pending[w].clear(); t->ev_bytes[w].clear();
    }
}

}  // namespace rl

#include "rl_chain_host.inc"   // the host side of the exact float chains: enqueue_chain, the two sharded leaf-sum exchanges, enqueue_metric_mean
#include "rl_launch.inc"       // launch_rank and launch_hist<ROOT>: which k_rank_* / k_hist instantiation a data set and a Ctx get

namespace rl {

// multi-GPU: per-query values of all ranks in global query order (ranks hold ascending contiguous query ranges)
static int gather_queries(rl_trainer *t, const double *local, const double **out, bool valid = false)
{
    hipStream_t s = t->stream;
    const int Q = valid ? t->va.Q : t->tr.Q, Qmax = valid ? t->vQmax : t->Qmax;
    double *snd = valid ? t->d_vqsend : t->d_qsend, *gat = valid ? t->d_vqgath : t->d_qgath, *cat = valid ? t->d_vqcat : t->d_qcat;
    hipLaunchKernelGGL(k_copy_f64, dim3(std::max(1, std::min(1024, (Q + kThreads - 1) / kThreads))), dim3(kThreads), 0, s, local, snd, Q);
    int rc = t->dist->allgather(snd, gat, (size_t)Qmax * sizeof(double), s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_concat_ranks, dim3(64), dim3(kThreads), 0, s, (const double *)gat, (const int32_t *)(valid ? t->d_vallQ : t->d_allQ), t->n_ranks, Qmax, cat);
    *out = cat;
    return RL_OK;
}

}  // namespace rl

#include "rl_tie_host.inc"   // the lazy tie-break's host side: the stages of a resolution and resolve_ties itself (their kernels: rl_tie.inc)
#include "rl_round.inc"      // the stages of a boosting round and enqueue_round itself (resolve_ties is theirs to call)

namespace rl {

static int sync_rounds(rl_trainer *t)
{
    RL_HIP(hipStreamSynchronize(t->stream));
    RL_HIP(hipStreamSynchronize(t->side));
    collect_timing(t);
    TreeState st;
    RL_HIP(hipMemcpy(&st, t->ctx.st, sizeof(st), hipMemcpyDeviceToHost));
    if (st.error) return fail(RL_ERR_HIP, "device tree growth ran out of node slots (internal error)");
    if (t->round > t->synced_rounds) {
        t->h_metrics.resize((size_t)t->round * 2);
        RL_HIP(hipMemcpy(t->h_metrics.data() + 2 * (size_t)t->synced_rounds, t->ctx.round_metric + 2 * (size_t)t->synced_rounds,
                         (size_t)(t->round - t->synced_rounds) * 2 * sizeof(float), hipMemcpyDeviceToHost));
        t->synced_rounds = t->round;
    }
    return RL_OK;
}

static int fetch_tree(const rl_trainer *tc, int i, HostTree &out)
{
    rl_trainer *t = const_cast<rl_trainer *>(tc);
    if ((int)t->trees.size() <= i) t->trees.resize((size_t)i + 1);
    if (t->trees[i].n_nodes > 0) { out = t->trees[i]; return RL_OK; }
    const int MAXN = t->ctx.MAXN;
    int32_t nn = 0;
    RL_HIP(hipMemcpy(&nn, t->ens.n_nodes + i, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (nn <= 0 || nn > MAXN) return fail(RL_ERR_STATE, "tree " + std::to_string(i) + " has not been built");
    std::vector<int32_t> fi(nn), le(nn), ri(nn), cn(nn);
    std::vector<float> th(nn), ou(nn);
    std::vector<double> dv(nn);
    const size_t o = (size_t)i * MAXN;
    RL_HIP(hipMemcpy(fi.data(), t->ens.feat_idx + o, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(le.data(), t->ens.left + o, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(ri.data(), t->ens.right + o, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(cn.data(), t->ens.count + o, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(th.data(), t->ens.thr + o, nn * sizeof(float), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(ou.data(), t->ens.out + o, nn * sizeof(float), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(dv.data(), t->ens.deviance + o, nn * sizeof(double), hipMemcpyDeviceToHost));
    HostTree h;
    h.weight = t->p.learning_rate;
    // creation order -> pre-order (root, left subtree, right subtree)
    std::vector<int> stack{0};
    std::vector<int> order, newid(nn, -1);
    while (!stack.empty()) {
        const int x = stack.back(); stack.pop_back();
        newid[x] = (int)order.size(); order.push_back(x);
        if (fi[x] != -1) { stack.push_back(ri[x]); stack.push_back(le[x]); }
    }
    h.n_nodes = (int)order.size();
    for (int x : order) {
        const bool leaf = fi[x] == -1;
        h.feature.push_back(leaf ? -1 : t->feature_ids[fi[x]]);
        h.threshold.push_back(th[x]);
        h.left.push_back(leaf ? -1 : newid[le[x]]);
        h.right.push_back(leaf ? -1 : newid[ri[x]]);
        h.output.push_back(ou[x]);
        h.deviance.push_back(dv[x]);
        h.count.push_back(cn[x]);
    }
    t->trees[i] = h;
    out = h;
    return RL_OK;
}

__global__ void k_debug_root_sum(const Ctx c, double *out, long long *out_fixed)
{
    const int f = blockIdx.x;
    for (int t = threadIdx.x; t < c.nthr[f]; t += blockDim.x) {
        const size_t o = (size_t)f * c.TS + t;
        if (out) out[o] = fixed_to_double(make_i128(c.cum_hi[o], c.cum_lo[o]), c.st->E);
        if (out_fixed) { out_fixed[2 * o] = c.cum_hi[o]; out_fixed[2 * o + 1] = (long long)c.cum_lo[o]; }
    }
}

}  // namespace rl

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int rl_abi_version(void) { return RLHIP_ABI_VERSION; }
const char *rl_last_error(void) { return g_err.c_str(); }

int rl_device_count(int32_t *n)
{
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { if (n) *n = 0; return fail(RL_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    if (n) *n = c;
    return RL_OK;
}

void rl_params_default(rl_params *p)
{   // learning/tree/LambdaMART.java:37-42
    if (!p) return;
    p->n_trees = 1000; p->n_leaves = 10; p->n_threshold = 256; p->min_leaf_support = 1; p->early_stop_rounds = 100;
    p->learning_rate = 0.1F; p->metric = RL_METRIC_NDCG; p->metric_k = 10; p->device = 0; p->flags = 0;
    p->ranker = RL_RANKER_LAMBDAMART;
    p->feature_sampling_rate = 1.0f; p->seed = 0;
}

int rl_set_external_judgments(rl_trainer *t, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (t->inited) return fail(RL_ERR_STATE, "rl_set_external_judgments must be called before rl_init");
    if (validation ? !t->has_valid : !t->has_train) return fail(RL_ERR_STATE, "set the data first");
    std::string err;
    const int rc = (validation ? t->va : t->tr).set_external(ideal_dcg, rel_doc_count, err);
    return rc ? fail(rc, err) : RL_OK;
}

int rl_set_err_max(double max_gain)
{
    if (!(max_gain > 0.0) || !std::isfinite(max_gain)) return fail(RL_ERR_INVALID, "ERRScorer.MAX must be positive and finite");
    g_err_max = max_gain;
    return RL_OK;
}

int rl_create(const rl_params *p, rl_trainer **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    if (p->metric < RL_METRIC_NDCG || p->metric > RL_METRIC_RR)
        return fail(RL_ERR_UNSUPPORTED, "train metric must be NDCG, DCG, MAP, ERR, P or RR (BEST is not built for training)");
    if (p->metric == RL_METRIC_MAP ? p->metric_k < 0 : p->metric_k < 1) return fail(RL_ERR_UNSUPPORTED, "metric k out of range");
    if (p->ranker != RL_RANKER_LAMBDAMART && p->ranker != RL_RANKER_MART)
        return fail(RL_ERR_UNSUPPORTED, "ranker must be RL_RANKER_LAMBDAMART (6) or RL_RANKER_MART (0)");
    if (!(p->feature_sampling_rate >= 0.0f && p->feature_sampling_rate <= 1.0f)) return fail(RL_ERR_INVALID, "feature_sampling_rate must be in [0, 1]");
    if (p->n_trees < 1) return fail(RL_ERR_INVALID, "n_trees must be >= 1");
    if (p->n_leaves < 1 && p->n_leaves != -1) return fail(RL_ERR_INVALID, "n_leaves must be >= 1, or -1 for trees limited by min_leaf_support only");
    if (p->min_leaf_support < 1) return fail(RL_ERR_INVALID, "min_leaf_support must be >= 1");
    if (p->n_threshold != -1 && (p->n_threshold < 1 || p->n_threshold > (1 << 24)))
        return fail(RL_ERR_UNSUPPORTED, "n_threshold must be -1 or in [1, 2^24]");
    if (p->flags & ~(RL_FLAG_FAST_LEAF | RL_FLAG_TIMING | RL_FLAG_TIMING_NODES | RL_FLAG_SERIAL_CHAIN | RL_FLAG_JAVA_ORDER | RL_FLAG_FIRST_TIE)) return fail(RL_ERR_INVALID, "unknown bit in rl_params.flags");
    if ((p->flags & RL_FLAG_FAST_LEAF) && (p->flags & RL_FLAG_JAVA_ORDER))
        return fail(RL_ERR_INVALID, "RL_FLAG_FAST_LEAF with RL_FLAG_JAVA_ORDER: the strict mode is a parity instrument, its leaves are the Java's float running sums");
    if ((p->flags & RL_FLAG_FAST_LEAF) && (p->flags & RL_FLAG_SERIAL_CHAIN))
        return fail(RL_ERR_INVALID, "RL_FLAG_FAST_LEAF with RL_FLAG_SERIAL_CHAIN: the serial kernel evaluates the float running sums that the fast mode replaces");
    const int gate = open_device(p->device, true);
    if (gate) return gate;
    std::unique_ptr<rl_trainer> t(new rl_trainer());
    t->p = *p;
    t->knobs.read();
    t->err_max = g_err_max;
    memset(&t->ctx, 0, sizeof(t->ctx));
    memset(&t->ens, 0, sizeof(t->ens));
    RL_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    RL_HIP(hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking));
    RL_HIP(hipEventCreateWithFlags(&t->ev_ranked, hipEventDisableTiming)); RL_HIP(hipEventCreateWithFlags(&t->ev_metric, hipEventDisableTiming));
    RL_HIP(hipEventCreateWithFlags(&t->ev_lam_fork, hipEventDisableTiming));
    for (int i = 0; i < 3; i++) { RL_HIP(hipStreamCreateWithFlags(&t->lam_s[i], hipStreamNonBlocking)); RL_HIP(hipEventCreateWithFlags(&t->ev_lam_join[i], hipEventDisableTiming)); }
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 16, kHistLdsStride>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 16, kHistLdsStride>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 16, kHistLdsStride, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 16, kHistLdsStride, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 16, kHistLdsStride, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 16, kHistLdsStride, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 16, kHistLdsStride, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 16, kHistLdsStride, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 16, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 16, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 8, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 8, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 4, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 4, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 2, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 2, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<true, 1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist<false, 1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_reduce, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxBins * 20));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_sp<kHistLdsStride>, hipFuncAttributeMaxDynamicSharedMemorySize, kHistFG * kHistLdsStride * 8));
    RL_HIP(hipFuncSetAttribute((const void *)k_select, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_finish_wide, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_finish<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_finish<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_finish<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_finish<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_finish<true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_hist_finish<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_rank_block, hipFuncAttributeMaxDynamicSharedMemorySize, ((kLambdaBlockCap + 63) & ~63) * kRankLdsPerDoc));      // (max_big is rounded up to 64 documents)
    RL_HIP(hipFuncSetAttribute((const void *)k_rank_mixed, hipFuncAttributeMaxDynamicSharedMemorySize, std::max((kLambdaBlockCap + 63) & ~63, (kRankBlockThreads / 64) * kLambdaWaveCap) * kRankLdsPerDoc));
    RL_HIP(hipFuncSetAttribute((const void *)k_lambda_tiny, hipFuncAttributeMaxDynamicSharedMemorySize, kLambdaTinyGroups * lambda_tiny_group_bytes(kLambdaFusedMaxK)));
    RL_HIP(hipFuncSetAttribute((const void *)k_lambda_fused<256, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kLambdaFusedMaxK * (256 + 8) * 16 + 2048));
    RL_HIP(hipFuncSetAttribute((const void *)k_lambda_fused<256, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLambdaFusedMaxK * (256 + 8) * 16 + 2048 + lambda_fused_cp_bytes(kLambdaFusedMaxK, 256)));
    RL_HIP(hipFuncSetAttribute((const void *)k_lambda_fused<256, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, kLambdaFusedMaxK * (256 + 8) * 16 + 8192));
    RL_HIP(hipFuncSetAttribute((const void *)k_lambda_fused<256, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, kLambdaFusedMaxK * (256 + 8) * 16 + 8192));
    RL_HIP(hipFuncSetAttribute((const void *)k_lambda_fused<256, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, kLambdaFusedMaxK * (256 + 8) * 16 + 2048));
    RL_HIP(hipFuncSetAttribute((const void *)k_lambda_fused<256, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, kLambdaFusedMaxK * (256 + 8) * 16 + 2048));
    RL_HIP(hipFuncSetAttribute((const void *)k_chain_stitch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_tie_finish, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    *out = t.release();
    return RL_OK;
}

void rl_destroy(rl_trainer *t)
{
    if (!t) return;
    (void)hipSetDevice(t->p.device);
    if (t->knobs.tie_prof && t->tie_stalls > 0)
        fprintf(stderr, "[rlhip] tie-break: %lld resolutions (%lld batches, %lld trees regrown), host us: first read %lld, chains %lld, candidates+lists %lld, sums %lld, finish %lld, total %lld\n",
                t->tie_stalls, t->tie_batches, t->tie_regrown, t->tie_phase_us[0], t->tie_phase_us[1], t->tie_phase_us[2], t->tie_phase_us[3], t->tie_phase_us[4], t->tie_us);
    if (t->knobs.chain_prof)
        fprintf(stderr, "[rlhip] float chains: %lld watched evaluations with %lld repair passes, %lld blind ones with %lld; progress-word time-outs %lld; host waited %lld us for stitches\n",
                t->chain_calls[0], t->chain_repairs[0], t->chain_calls[1], t->chain_repairs[1], t->chain_timeouts, t->chain_wait_us);
    if (t->stream) { (void)hipStreamSynchronize(t->stream); }
    if (t->side) { (void)hipStreamSynchronize(t->side); (void)hipStreamDestroy(t->side); }
    if (t->ev_lam_fork) (void)hipEventDestroy(t->ev_lam_fork);
    for (int i = 0; i < 3; i++) { if (t->ev_lam_join[i]) (void)hipEventDestroy(t->ev_lam_join[i]); if (t->lam_s[i]) (void)hipStreamDestroy(t->lam_s[i]); }
    if (t->ev_ranked) (void)hipEventDestroy(t->ev_ranked);
    if (t->ev_metric) (void)hipEventDestroy(t->ev_metric);
    for (int w = 0; w < RL_KERNEL_COUNT_; w++)
        for (auto &pr : t->ev_pending[w]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto e : t->ev_free) (void)hipEventDestroy(e);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    if (t->h_progress) (void)hipHostFree(t->h_progress);
    if (t->h_xmail) (void)hipHostFree(t->h_xmail);
    if (t->tie_buf) (void)hipFree(t->tie_buf);
    if (t->tie_pin) (void)hipHostFree(t->tie_pin);
    for (void *q : t->pinned) (void)hipHostFree(q);
    delete t;
}

int rl_set_train(rl_trainer *t, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                 int32_t n_queries, const int32_t *feature_ids, const int32_t *qkey)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (t->has_train) return fail(RL_ERR_STATE, "training set already set");
    int rc = validate_dataset(X, n_docs, n_features, labels, qoff, n_queries);
    if (rc) return rc;
    RL_HIP(hipSetDevice(t->p.device));
    t->F = n_features;
    t->feature_ids.resize(n_features);
    for (int f = 0; f < n_features; f++) {
        t->feature_ids[f] = feature_ids ? feature_ids[f] : f + 1;
        if (t->feature_ids[f] <= 0) return fail(RL_ERR_INVALID, "Cannot use feature numbering less than or equal to zero. Start your features at 1.");
    }
    rc = load_dataset(t, t->tr, X, n_docs, labels, qoff, n_queries, qkey);
    if (rc) return rc;
    t->has_train = true;
    return RL_OK;
}

int rl_set_validation(rl_trainer *t, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                      const int32_t *qkey)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->has_train) return fail(RL_ERR_STATE, "set the training set first");
    if (t->inited) return fail(RL_ERR_STATE, "validation set must be set before rl_init");
    if (t->has_valid) return fail(RL_ERR_STATE, "validation set already set");
    int rc = validate_dataset(X, n_docs, t->F, labels, qoff, n_queries);
    if (rc) return rc;
    RL_HIP(hipSetDevice(t->p.device));
    rc = load_dataset(t, t->va, X, n_docs, labels, qoff, n_queries, qkey);
    if (rc) return rc;
    t->has_valid = true;
    return RL_OK;
}

int rl_set_rows(rl_trainer *t, int32_t validation, int64_t first_doc, int64_t n_docs, const float *X)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (t->inited) return fail(RL_ERR_STATE, "rows must be delivered before rl_init");
    if (validation ? !t->has_valid : !t->has_train) return fail(RL_ERR_STATE, "rl_set_rows before rl_set_train / rl_set_validation");
    DataSet &d = validation ? t->va : t->tr;
    if (d.rows_next < 0) return fail(RL_ERR_STATE, "the rows of this data set were already given to rl_set_train / rl_set_validation");
    if (!X || n_docs <= 0) return fail(RL_ERR_INVALID, "bad argument");
    if (first_doc != d.rows_next || first_doc + n_docs > d.N) return fail(RL_ERR_INVALID, "row blocks must be consecutive and stay inside the data set");
    RL_HIP(hipSetDevice(t->p.device));
    RL_HIP(hipMemcpy(d.d_X + (size_t)first_doc * t->F, X, (size_t)n_docs * t->F * sizeof(float), hipMemcpyHostToDevice));
    d.rows_next += n_docs;
    return RL_OK;
}

}  // extern "C"

#include "rl_init.inc"      // the stages of rl_init (the kernels they launch are instantiated here)

extern "C" {

int rl_init(rl_trainer *t)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->has_train) return fail(RL_ERR_STATE, "no training set");
    if (t->inited) return fail(RL_ERR_STATE, "rl_init called twice");
    if ((t->tr.rows_next >= 0 && t->tr.rows_next != t->tr.N) || (t->has_valid && t->va.rows_next >= 0 && t->va.rows_next != t->va.N))
        return fail(RL_ERR_STATE, "rl_set_rows has not delivered every row yet");
    RL_HIP(hipSetDevice(t->p.device));
    RL_HIP(hipDeviceSynchronize());      // uploads of rl_set_* went through the null stream; t->stream is non-blocking
    InitWork w;
    int rc = init_shape(t, w);
    if (!rc) rc = init_threshold_tables(t, w);
    if (!rc) rc = init_hist_features(t, w);
    if (!rc) rc = init_bins(t, w);
    if (!rc) rc = init_compact_rows(t, w);
    if (!rc) rc = init_sparse_root(t, w);
    if (!rc) rc = init_java_deal(t, w);
    if (!rc) rc = init_query_side(t, w);
    if (!rc) rc = init_round_state(t, w);
    if (!rc) rc = init_dist_state(t, w);
    if (!rc) rc = init_lambda_state(t);
    if (rc) return rc;
    RL_HIP(hipDeviceSynchronize());
    t->inited = true;
    return RL_OK;
}

int rl_boost_round(rl_trainer *t, rl_tree *out, float *train_metric, float *valid_metric, int32_t *stop)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    if (t->finished) return fail(RL_ERR_STATE, "rl_finish has been called");
    if (t->round >= t->p.n_trees) return fail(RL_ERR_STATE, "all n_trees rounds are done");
    RL_HIP(hipSetDevice(t->p.device));
    const int m = t->round;
    int rc = enqueue_round(t);
    if (rc) return rc;
    rc = sync_rounds(t);
    if (rc) return rc;
    if (train_metric) *train_metric = t->h_metrics[2 * (size_t)m];
    if (t->has_valid) {
        const float vm = t->h_metrics[2 * (size_t)m + 1];
        if (valid_metric) *valid_metric = vm;
        const double score = vm;                                     // LambdaMART.java:237-243
        if (score > t->best_score) { t->best_score = score; t->best_round = t->round - 1; }
    }
    if (stop) *stop = (m - t->best_round > t->p.early_stop_rounds) ? 1 : 0;      // :248
    if (out) return rl_get_tree(t, m, out);
    return RL_OK;
}

int rl_boost_rounds_async(rl_trainer *t, int32_t n)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    if (t->has_valid) return fail(RL_ERR_STATE, "asynchronous rounds cannot honour early stopping; use rl_boost_round");
    if (t->round + n > t->p.n_trees) return fail(RL_ERR_STATE, "more rounds than n_trees");
    RL_HIP(hipSetDevice(t->p.device));
    for (int i = 0; i < n; i++) { int rc = enqueue_round(t); if (rc) return rc; }
    return RL_OK;
}

int rl_sync(rl_trainer *t)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    RL_HIP(hipSetDevice(t->p.device));
    return sync_rounds(t);
}

static int final_score(rl_trainer *t, DataSet &d, double *out)
{
    hipStream_t s = t->stream;
    double *d_sc = nullptr;
    RL_HIP(t->pool.alloc(&d_sc, (size_t)d.N));
    hipLaunchKernelGGL(k_ensemble_eval, dim3((unsigned)std::min<int64_t>(8192, (d.N + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, t->ens,
                       t->ctx.MAXN, t->n_kept, (const float *)d.d_X, d.N, t->F, t->p.learning_rate, (float *)nullptr, d_sc);
    int rc = launch_rank(t, d, d_sc, d.d_ndcg, false);
    if (rc) return rc;
    if (t->dist) {
        const double *gq = nullptr;
        const bool valid = (&d == &t->va);
        rc = gather_queries(t, d.d_ndcg, &gq, valid);
        if (rc) return rc;
        hipLaunchKernelGGL(k_double_mean, dim3(1), dim3(64), 0, s, gq, valid ? t->vQglobal : t->Qglobal, t->d_mean);
    } else hipLaunchKernelGGL(k_double_mean, dim3(1), dim3(64), 0, s, (const double *)d.d_ndcg, d.Q, t->d_mean);
    RL_HIP(hipGetLastError());
    RL_HIP(hipStreamSynchronize(s));
    RL_HIP(hipMemcpy(out, t->d_mean, sizeof(double), hipMemcpyDeviceToHost));
    t->pool.release(d_sc);
    return RL_OK;
}

int rl_finish(rl_trainer *t, double *train_score, double *valid_score)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    RL_HIP(hipSetDevice(t->p.device));
    int rc = sync_rounds(t);
    if (rc) return rc;
    if ((int64_t)t->n_kept > (int64_t)t->best_round + 1) t->n_kept = t->best_round + 1;      // LambdaMART.java:254-256
    double ts = 0, vs = 0;
    rc = final_score(t, t->tr, &ts);                                                          // :259
    if (rc) return rc;
    if (train_score) *train_score = ts;
    if (t->has_valid) {
        rc = final_score(t, t->va, &vs);                                                      // :263
        if (rc) return rc;
        t->best_score = vs;
        if (valid_score) *valid_score = vs;
    }
    t->finished = true;
    return RL_OK;
}

int rl_num_trees(const rl_trainer *t, int32_t *n)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (n) *n = t->n_kept;
    return RL_OK;
}

int rl_tree_capacity(const rl_trainer *t, int32_t *cap)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    if (cap) *cap = t->ctx.MAXN;
    return RL_OK;
}

int rl_get_tree(const rl_trainer *t, int32_t i, rl_tree *out)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!out) return fail(RL_ERR_INVALID, "null tree");
    if (i < 0 || i >= t->synced_rounds) return fail(RL_ERR_INVALID, "tree index out of range (did you rl_sync?)");
    RL_HIP(hipSetDevice(t->p.device));
    HostTree h;
    int rc = fetch_tree(t, i, h);
    if (rc) return rc;
    out->n_nodes = h.n_nodes;
    if (out->cap < h.n_nodes) return fail(RL_ERR_INVALID, "rl_tree.cap too small");
    for (int j = 0; j < h.n_nodes; j++) {
        out->feature[j] = h.feature[j]; out->threshold[j] = h.threshold[j]; out->left[j] = h.left[j]; out->right[j] = h.right[j];
        out->output[j] = h.output[j];
        if (out->deviance) out->deviance[j] = h.deviance[j];
        if (out->count) out->count[j] = h.count[j];
    }
    return RL_OK;
}

int rl_get_round_metrics(const rl_trainer *t, int32_t round, float *train_metric, float *valid_metric)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (round < 0 || round >= t->synced_rounds) return fail(RL_ERR_INVALID, "round out of range (did you rl_sync?)");
    if (train_metric) *train_metric = t->h_metrics[2 * (size_t)round];
    if (valid_metric && t->has_valid) *valid_metric = t->h_metrics[2 * (size_t)round + 1];
    return RL_OK;
}

int rl_best_validation(const rl_trainer *t, int32_t *best_round, double *best_score)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (best_round) *best_round = t->best_round;
    if (best_score) *best_score = t->best_score;
    return RL_OK;
}

int rl_predict(rl_trainer *t, const float *X, int64_t n_docs, float *out)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    if (!X || !out || n_docs < 0) return fail(RL_ERR_INVALID, "bad argument");
    if (n_docs == 0) return RL_OK;
    RL_HIP(hipSetDevice(t->p.device));
    int rc = sync_rounds(t);
    if (rc) return rc;
    float *dX = nullptr, *dO = nullptr;
    RL_HIP(hipMalloc((void **)&dX, (size_t)n_docs * t->F * sizeof(float)));
    RL_HIP(hipMalloc((void **)&dO, (size_t)n_docs * sizeof(float)));
    RL_HIP(hipMemcpyAsync(dX, X, (size_t)n_docs * t->F * sizeof(float), hipMemcpyHostToDevice, t->stream));
    hipLaunchKernelGGL(k_ensemble_eval, dim3((unsigned)std::min<int64_t>(8192, (n_docs + kThreads - 1) / kThreads)), dim3(kThreads), 0, t->stream,
                       t->ens, t->ctx.MAXN, t->n_kept, (const float *)dX, n_docs, t->F, t->p.learning_rate, dO, (double *)nullptr);
    RL_HIP(hipGetLastError());
    RL_HIP(hipStreamSynchronize(t->stream));
    RL_HIP(hipMemcpy(out, dO, (size_t)n_docs * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(dX); (void)hipFree(dO);
    return RL_OK;
}

int rl_model_to_text(const rl_trainer *t, char *buf, int64_t cap, int64_t *needed)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    RL_HIP(hipSetDevice(t->p.device));
    if (t->synced_rounds < t->n_kept) return fail(RL_ERR_STATE, "rounds still in flight: call rl_sync first");
    std::vector<HostTree> trees((size_t)t->n_kept);
    for (int i = 0; i < t->n_kept; i++) { int rc = fetch_tree(t, i, trees[i]); if (rc) return rc; }
    ModelHeader h{t->p.n_trees, t->p.n_leaves, t->p.n_threshold, t->p.learning_rate, t->p.early_stop_rounds,
                  t->p.ranker == RL_RANKER_MART ? "MART" : "LambdaMART"};
    const std::string s = model_to_text(h, trees);                // LambdaMART.model()  LambdaMART.java:290-301
    if (needed) *needed = (int64_t)s.size() + 1;
    if (buf && cap >= (int64_t)s.size() + 1) memcpy(buf, s.c_str(), s.size() + 1);
    return RL_OK;
}

// ---- multi-GPU (rl_dist.inc) -------------------------------------------------------------------------
int rl_dist_unique_id(void *id_out)
{
    if (!id_out) return fail(RL_ERR_INVALID, "null id buffer");
    RcclApi &r = rccl();
    if (!r.lib || !r.GetUniqueId) return fail(RL_ERR_COMM, "librccl.so could not be loaded");
    const int rc = r.GetUniqueId(id_out);
    return rc == 0 ? RL_OK : fail(RL_ERR_COMM, std::string("ncclGetUniqueId: ") + r.GetErrorString(rc));
}

static int dist_precheck(rl_trainer *t, int32_t rank, int32_t n_ranks)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (t->inited) return fail(RL_ERR_STATE, "rl_dist_init must be called before rl_init");
    if (n_ranks < 1 || n_ranks > 64 || rank < 0 || rank >= n_ranks) return fail(RL_ERR_INVALID, "bad rank / n_ranks (1..64 ranks)");
    if (t->p.flags & RL_FLAG_FAST_LEAF)
        return fail(RL_ERR_UNSUPPORTED, "RL_FLAG_FAST_LEAF with sharded training: an f64 sum over ranks is not rank-count-invariant (the leaf values would depend on "
                                        "how the queries are sharded); train on one GPU, or without the flag");
    return RL_OK;
}

int rl_dist_init(rl_trainer *t, const void *id, int32_t rank, int32_t n_ranks)
{
    int rc = dist_precheck(t, rank, n_ranks);
    if (rc) return rc;
    if (!id) return fail(RL_ERR_INVALID, "null unique id");
    RL_HIP(hipSetDevice(t->p.device));
    RcclApi &r = rccl();
    if (!r.lib || !r.CommInitRank || !r.AllReduce || !r.AllGather) return fail(RL_ERR_COMM, "librccl.so could not be loaded");
    std::unique_ptr<RcclBackend> b(new RcclBackend());
    UidVal u;
    memcpy(u.b, id, RL_UNIQUE_ID_BYTES);
    const int nrc = r.CommInitRank(&b->comm, n_ranks, u, rank);
    if (nrc != 0) return fail(RL_ERR_COMM, std::string("ncclCommInitRank: ") + r.GetErrorString(nrc));
    b->rank = rank; b->n = n_ranks;
    t->rank = rank; t->n_ranks = n_ranks;
    t->dist = std::move(b);
    return RL_OK;
}

int rl_dist_stats(const rl_trainer *t, int64_t *out)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!out) return fail(RL_ERR_INVALID, "null argument");
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (t->dist) {
        out[0] = t->dist->n_allreduce; out[1] = t->dist->b_allreduce; out[2] = t->dist->n_allgather; out[3] = t->dist->b_allgather;
        out[4] = t->dist->n_alltoall; out[5] = t->dist->b_alltoall; out[6] = t->dist->n_tie; out[7] = t->dist->b_tie;
    }
    return RL_OK;
}

int rl_dist_init_callback(rl_trainer *t, int32_t rank, int32_t n_ranks, rl_host_allreduce_fn allreduce, rl_host_allgather_fn allgather,
                          rl_host_alltoallv_fn alltoallv, void *user)
{
    int rc = dist_precheck(t, rank, n_ranks);
    if (rc) return rc;
    if (!allreduce || !allgather) return fail(RL_ERR_INVALID, "null callback");
    std::unique_ptr<CallbackBackend> b(new CallbackBackend());
    b->ar = allreduce; b->ag = allgather; b->aa = alltoallv; b->user = user; b->rank = rank; b->n = n_ranks;
    t->rank = rank; t->n_ranks = n_ranks;
    t->dist = std::move(b);
    return RL_OK;
}

// ---- introspection -------------------------------------------------------------------------------
int rl_hist_features(const rl_trainer *t, int32_t *n, int32_t *columns, int32_t cap)
{
    if (check_trainer(t) || !n) return fail(RL_ERR_INVALID, "null argument");
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    *n = t->ctx.F;
    if (columns) for (int32_t v = 0; v < t->ctx.F && v < cap; v++) columns[v] = t->vcol.empty() ? v : t->vcol[v];
    return RL_OK;
}

int rl_bin_stride(const rl_trainer *t, int32_t *stride)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    if (stride) *stride = t->ctx.TS;
    return RL_OK;
}

int rl_quant_exponent(const rl_trainer *t, int32_t *e)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    TreeState st;
    RL_HIP(hipMemcpy(&st, t->ctx.st, sizeof(st), hipMemcpyDeviceToHost));
    if (e) *e = st.E;
    return RL_OK;
}

int rl_get_array(rl_trainer *t, int32_t which, void *out, int64_t cap_bytes)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (!t->inited) return fail(RL_ERR_STATE, "rl_init has not been called");
    RL_HIP(hipSetDevice(t->p.device));
    RL_HIP(hipStreamSynchronize(t->stream));
    const Ctx &c = t->ctx;
    const void *src = nullptr; size_t bytes = 0;
    switch (which) {
    case RL_ARR_LAMBDA: case RL_ARR_WEIGHT: {        // interleaved on the device: strided copy of one component
        bytes = (size_t)c.N * 8;
        if ((int64_t)bytes > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
        RL_HIP(hipMemcpy2D(out, 8, (const char *)c.lw + (which == RL_ARR_WEIGHT ? 8 : 0), 16, 8, (size_t)c.N, hipMemcpyDeviceToHost));
        return RL_OK;
    }
    case RL_ARR_SCORE: src = c.scores; bytes = (size_t)c.N * 8; break;
    case RL_ARR_VALID_SCORE: if (!t->has_valid) return fail(RL_ERR_STATE, "no validation set"); src = t->va.d_scores; bytes = (size_t)t->va.N * 8; break;
    case RL_ARR_NBINS: src = c.nthr; bytes = (size_t)c.F * 4; break;
    case RL_ARR_THRESHOLDS: src = c.thr; bytes = (size_t)c.F * c.TS * 4; break;
    case RL_ARR_ROOT_COUNT: src = c.cum_cnt; bytes = (size_t)c.F * c.TS * 4; break;
    case RL_ARR_QUANT: src = c.q; bytes = (size_t)c.N * 8; break;
    case RL_ARR_NDCG_PER_QUERY: src = c.ndcg_q; bytes = (size_t)c.Q * 8; break;
    case RL_ARR_GROW_STATS: src = c.grow_stats; bytes = 16; break;
    case RL_ARR_GROW_DOCS: src = c.grow_docs; bytes = 32; break;
    case RL_ARR_BUBBLES: src = c.grow_docs + 4; bytes = 32; break;
    case RL_ARR_PIECE_STATS: {
        const int64_t v[2] = {t->piece_rounds, t->piece_misses};
        if ((int64_t)sizeof(v) > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
        memcpy(out, v, sizeof(v));
        return RL_OK;
    }
    case RL_ARR_SPARSE_INFO: {
        const int64_t v[8] = {c.sp_on ? c.sp_ngroups : 0, t->sp_entries, c.sp_on ? c.numFG - c.sp_ngroups : c.numFG, t->sp_cols,
                              c.crows ? t->cr_groups : 0, (int64_t)t->cr_entries, (int64_t)t->cr_overflow, c.cr_stride};
        if (cap_bytes < (int64_t)sizeof(v)) return fail(RL_ERR_INVALID, "output buffer too small");
        memcpy(out, v, sizeof(v));
        return RL_OK;
    }
    case RL_ARR_LAUNCH_ARMS: {       // host counters (t->arms) and the settings in force: the knobs as read, what rl_init left in the context
        int64_t v[RL_ARM_COUNT_];
        memcpy(v, t->arms, sizeof(v));
        v[RL_ARM_SET_STEP_AHEAD] = t->knobs.step_ahead; v[RL_ARM_SET_DIST_AHEAD] = t->knobs.dist_ahead;
        v[RL_ARM_SET_P8] = c.p8; v[RL_ARM_SET_DM_ROOT] = c.dm_root; v[RL_ARM_SET_DM_DIV] = c.dm_div; v[RL_ARM_SET_SUB_CHILD] = c.sub_child; v[RL_ARM_SET_HIST_NT] = c.hist_nt;
        v[RL_ARM_SET_ANY_RUNS] = c.any_runs; v[RL_ARM_SET_CROWS] = c.crows ? 1 : 0; v[RL_ARM_SET_TIE_ON] = c.tie_on; v[RL_ARM_SET_NODE_DIV] = c.node_div;
        v[RL_ARM_SET_NODE_MIN] = c.node_min; v[RL_ARM_SET_BALANCE] = c.balance; v[RL_ARM_SET_BALANCE_TARGET] = c.balance_target; v[RL_ARM_SET_BALANCE_MIN] = c.balance_min;
        v[RL_ARM_SET_BALANCE_CAP] = c.balance_cap; v[RL_ARM_SET_NODE_CHUNK] = c.node_chunk; v[RL_ARM_SET_MAX_CHUNKS] = c.maxChunks;
        // (the table grew behind its 64th entry, the two replay arms: a caller built against the 64-entry table gets those 64)
        if (cap_bytes < (int64_t)(RL_ARM_REPLAY_TILED * sizeof(int64_t))) return fail(RL_ERR_INVALID, "output buffer too small");
        memcpy(out, v, std::min<size_t>(sizeof(v), (size_t)cap_bytes));
        return RL_OK;
    }
    case RL_ARR_TIE_STATS: {
        const int64_t v[10] = {t->tie_stalls, t->tie_nodes, t->tie_chain_nodes, t->tie_chain_docs, t->tie_us, t->tie_spec_segs, t->tie_spec_miss, t->tie_spec_serial,
                                t->tie_batches, t->tie_regrown};
        if (cap_bytes < (int64_t)sizeof(v)) return fail(RL_ERR_INVALID, "output buffer too small");
        memcpy(out, v, sizeof(v));
        return RL_OK;
    }
    case RL_ARR_STEP_LOG: {
        bytes = ((size_t)8 + 8 * kStepLogCap) * sizeof(int32_t);
        if ((int64_t)bytes > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
        if (c.steplog) { RL_HIP(hipMemcpy(out, c.steplog, bytes, hipMemcpyDeviceToHost)); RL_HIP(hipMemset(c.steplog, 0, 32)); }      // reading empties the log
        else memset(out, 0, bytes);
        return RL_OK;
    }
    case RL_ARR_PHASE_CLOCKS: src = c.clk; bytes = 64 * 32 * sizeof(long long); break;
    case RL_ARR_BLOCK_TRACE: if (!c.trace) return fail(RL_ERR_STATE, "no block trace (RLHIP_TRACE_TREE unset)"); src = c.trace; bytes = (size_t)64 * 3 * kTraceBlocks * kTraceStamps * sizeof(long long); break;
    case RL_ARR_CHAIN_STATS: {
        if (cap_bytes < 24) return fail(RL_ERR_INVALID, "output buffer too small");
        RL_HIP(hipMemcpy(out, (t->dist ? t->gchain : t->leaf_chain).stats, 12, hipMemcpyDeviceToHost));
        RL_HIP(hipMemcpy((char *)out + 12, t->metric_chain.stats, 12, hipMemcpyDeviceToHost));
        return RL_OK;
    }
    case RL_ARR_CHAIN_MISS: {
        const ChainBufs &b = (t->dist && !t->piece_chains) ? t->gchain : t->leaf_chain;
        bytes = (size_t)2 * b.maxseg * 4;
        if ((int64_t)bytes > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
        RL_HIP(hipMemcpy(out, b.miss, bytes, hipMemcpyDeviceToHost));
        return RL_OK;
    }
    case RL_ARR_BINS: {
        bytes = (size_t)c.F * c.N * 2;
        if ((int64_t)bytes > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
        RL_HIP(hipMemcpy2D(out, (size_t)c.N * 2, c.bins, (size_t)c.Npad * 2, (size_t)c.N * 2, c.F, hipMemcpyDeviceToHost));
        return RL_OK;
    }
    case RL_ARR_ROOT_SUM:
    case RL_ARR_ROOT_SUM_FIXED: {
        const bool fixed = which == RL_ARR_ROOT_SUM_FIXED;
        bytes = (size_t)c.F * c.TS * (fixed ? 16 : 8);
        if ((int64_t)bytes > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
        void *d = nullptr;
        RL_HIP(hipMalloc(&d, bytes));
        RL_HIP(hipMemsetAsync(d, 0, bytes, t->stream));      // same stream as the kernel: t->stream is non-blocking
        hipLaunchKernelGGL(k_debug_root_sum, dim3(c.F), dim3(kThreads), 0, t->stream, c, fixed ? (double *)nullptr : (double *)d,
                           fixed ? (long long *)d : (long long *)nullptr);
        RL_HIP(hipStreamSynchronize(t->stream));
        RL_HIP(hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
        (void)hipFree(d);
        return RL_OK;
    }
    case RL_ARR_ROOT_SUM_JAVA: {
        if (!c.java) return fail(RL_ERR_STATE, "RL_ARR_ROOT_SUM_JAVA needs RL_FLAG_JAVA_ORDER");
        bytes = (size_t)c.F * c.TS * 8;
        if ((int64_t)bytes > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
        RL_HIP(hipStreamSynchronize(t->stream));
        RL_HIP(hipMemcpy(out, c.jcum, bytes, hipMemcpyDeviceToHost));       // node 0 = the root
        return RL_OK;
    }
    default: return fail(RL_ERR_INVALID, "unknown array id");
    }
    if ((int64_t)bytes > cap_bytes) return fail(RL_ERR_INVALID, "output buffer too small");
    RL_HIP(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return RL_OK;
}

#include "rl_debug_abi.inc"

int rl_set_timing_flags(rl_trainer *t, int32_t flags)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    const int32_t mask = RL_FLAG_TIMING | RL_FLAG_TIMING_NODES;
    t->p.flags = (t->p.flags & ~mask) | (flags & mask);
    return RL_OK;
}

int rl_get_timing(rl_trainer *t, int32_t kernel, double *total_ms, int64_t *launches, double *alg_bytes)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    if (kernel < 0 || kernel >= RL_KERNEL_COUNT_) return fail(RL_ERR_INVALID, "unknown kernel id");
    if (total_ms) *total_ms = t->timing[kernel].ms;
    if (launches) *launches = t->timing[kernel].launches;
    if (alg_bytes) *alg_bytes = t->timing[kernel].bytes;
    return RL_OK;
}

int rl_reset_timing(rl_trainer *t)
{
    if (check_trainer(t)) return RL_ERR_INVALID;
    for (auto &s : t->timing) s = TimingSlot();
    return RL_OK;
}


// ---- scoring-only model (Ensemble loaded from RankLib model text) -----------------------------------
}  // extern "C"

#include "rl_model_eval.inc"
#include "rl_stage.inc"      // the model after every requested number of trees: k_model_stage_scores walks, k_stage_eval ranks and scores
#include "rl_permimp.inc"    // permutation importance: k_model_permuted_scores walks every (column, repeat) cell, k_stage_eval ranks and scores
#include "rl_partial.inc"    // partial dependence and ICE curves: k_model_partial_scores walks every (column, grid value) cell, k_partial_reduce sums them in one fixed order
#include "rl_model_rows.inc" // RowStream: a file's rows through a model kernel chunk by chunk, the host loop of the four entry points below
#include "rl_contrib.inc"    // contributions of the features to a document's score: k_model_cover counts a background file, k_model_contribs walks the paths
#include "rl_shap.inc"       // the same as exact TreeSHAP values: k_model_shap runs every row through the recurrence of every leaf
#include "rl_interact.inc"   // SHAP interaction values: k_model_interact runs that recurrence once per conditioned element, k_interact_finish makes the diagonal
#include "rl_resume.inc"     // resume: rl_adopt_model_text replays a saved model's trees as this trainer's first rounds (k_replay_scores)
#include "rl_refit.inc"      // refit: rl_refit_model_text keeps those trees' structure and recomputes their leaf values on this trainer's data (k_refit_route)
