// rl_round.inc -- the stages of one boosting round, in the order enqueue_round (at the end of this file) calls them.  Included by rl_trainer.hip behind
// rl_tie_host.inc, whose resolve_ties the growth stages call.
//
// Every trainer path runs these stages: one GPU, MART, the strict Java order, sharded.  A stage enqueues on the trainer's stream and returns; where
// the modes differ, the branches sit side by side inside the stage.  Sharded runs: every rank enqueues the same collectives in the same order, so
// every host decision that ends or stalls a tree is taken at the same growth step on every rank (growth_gate, enqueue_growth_step).
//
// What lives how long: RoundPlan is computed once per call, in front of the first launch.  A Growth is made afresh for every pass over a tree -- a
// tree that is grown again (deferred tie-break, rl_tie.inc) starts from a new one -- and the same Growth goes through a stall and its resumption.

namespace rl {

// ---- the launch geometry: the same every round, a few integer operations to compute -----------------------------------
struct RoundPlan {
    size_t hist_lds, red_lds, par_lds, fin_lds, slot_words;
    int hist_gx, rootCs, rootChunks, nodes_in_lds, jbg, steps;
};

static int round_plan(const rl_trainer *t, RoundPlan &pl)
{
    const Ctx &c = t->ctx;
    pl.hist_lds = (size_t)c.sub * ((c.sub == 16 && c.TS <= kHistLdsStride) ? kHistLdsStride : c.TS) * 12;    // int64 sums + int32 counts
    pl.hist_gx = c.numFG * (kHistFG / c.sub);
    pl.red_lds = (size_t)c.TS * 20;
    pl.rootCs = std::min(kChunk, std::max(kMinChunk, (((c.N + 63) / 64 + 255) & ~255)));   // == chunk_docs<true>(N)
    pl.rootChunks = (c.N + pl.rootCs - 1) / pl.rootCs;
    // the last block of k_hist_finish runs the growth bookkeeping (select_step); node records live in LDS when they fit
    pl.nodes_in_lds = (select_lds_bytes(c.L, c.NC, true, c.F, c.fs_on != 0) <= 60 * 1024) ? 1 : 0;
    pl.par_lds = (c.TS <= kParCacheTS) ? (size_t)c.TS * 20 + 8 : 0;       // the parent's entries next to the bins (hist_finish_body)
    pl.fin_lds = std::max((size_t)c.TS * (c.java ? 28 : 20) + 8 + pl.par_lds, select_lds_bytes(c.L, c.NC, pl.nodes_in_lds != 0, c.F, c.fs_on != 0));      // bins + the parent's entries (hist_finish_body)
    pl.jbg = (c.TS + 63) / 64;        // RL_FLAG_JAVA_ORDER: 64-bin groups of k_jhist (+ 1 block for the node totals)
    if (pl.fin_lds > 128 * 1024) return fail(RL_ERR_UNSUPPORTED, "too many features / leaves for the growth bookkeeping in LDS (feature sampling needs 64 bytes per feature)");
    // Growth steps: each prepares up to kSpec queue nodes and commits as many splits as the fit loop allows; L-1 steps
    // always suffice (every step commits at least the head of the queue); finished trees make the rest no-ops.
    pl.steps = std::max(c.L - 1, 1);
    pl.slot_words = (size_t)c.F * c.TS * c.limb_words + 4;
    return RL_OK;
}

// ---- lambdas (MART: residuals) and the blocks' max |lambda|; n_max: blocks that reported theirs (folded by k_max_reduce) ----
static int enqueue_lambdas(rl_trainer *t, int &n_max)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const int m = t->round;
    // round scalars
    RL_HIP(hipMemsetAsync(&c.st->maxabs_bits, 0, sizeof(unsigned long long) + sizeof(long long), s));
    n_max = 0;
    if (c.mart) {    // MART: residuals instead of lambdas (weights stay 0)
        ScopedTiming tm(t, RL_KERNEL_LAMBDA, (double)c.N * 20.0);
        n_max = std::min(2048, (c.N + kThreads - 1) / kThreads);
        t->arms[RL_ARM_LAM_MART]++;
        hipLaunchKernelGGL(k_mart_residual, dim3(n_max), dim3(kThreads), 0, s, c.labels, (const double *)c.scores, c.lw, c.N, t->d_wmax);
    } else {   // K1 lambdas: pair terms in parallel, then ordered accumulation (ranked order comes from the previous
        // round's k_rank_* / from rl_init for round 0)
        ScopedTiming tm(t, RL_KERNEL_LAMBDA, (double)c.N * 28.0);
        const double *ideal = (c.metric == RL_METRIC_NDCG) ? (m == 0 ? c.ideal0 : c.ideal1) : nullptr;
        LamArgs g{t->tr.d_ss, t->tr.d_sl, t->tr.d_srel, t->tr.d_sidx, c.qoff, t->tr.d_docq, ideal, c.disc,
                  t->d_T, c.lw, &c.st->maxabs_bits, c.N, c.k, c.k, c.metric, t->p.metric_k,
                  t->tr.d_aux_i, t->tr.d_aux_a, t->tr.d_aux_b, t->d_wmax, t->tr.d_ext_rd};
        if (t->d_T == nullptr) {
            const int mode = (c.metric == RL_METRIC_ERR) ? 1 : (c.metric == RL_METRIC_MAP) ? 2 : (c.metric == RL_METRIC_P) ? 3 : (c.metric == RL_METRIC_RR) ? 4 : 0;
            // (P / RR launches are counted under no RL_ARM_LAM_* arm: the arm table is full, DESIGN.md 21; their stream is counted as every fused launch's)
            static const int mode_arm[5] = {RL_ARM_LAM_FUSED, RL_ARM_LAM_ERR, RL_ARM_LAM_MAP, -1, -1};
            // knobs.lam_compact: NDCG / DCG pair terms from per-wavefront lists of the active pairs (k_lambda_fused<., 0, true>) instead of column by row.
            // Built and measured slower at NDCG@10 (profiles/r05i_ab_lambda_c2.txt: a wavefront's ~390 active pairs are 3.05 steps of 128, i.e. 4 against the 5 of
            // ten rows in pairs, and the lists cost LDS, registers and six ds_bpermute per pair); it is the shorter way from about NDCG@16 on.  Off by default.
            const bool cp = t->knobs.lam_compact && mode == 0;
            auto lds_of = [&](int bt) { return (size_t)c.k * (bt + 8) * 16 + (size_t)c.k * 24 + lambda_fused_extra_bytes(mode, c.k, bt) + (cp ? lambda_fused_cp_bytes(c.k, bt) : 0); };
            n_max = 0;
            const DataSet &d = t->tr;
            // (ls: the stream of this class -- the main one, or one of the three side streams forked below)
            int lam_used = 0;
            RL_HIP(hipEventRecord(t->ev_lam_fork, s));       // (sharded runs too, round 6: the classes only touch this rank's lists; the collectives follow on the main stream behind the join)
            auto lam_stream = [&]() -> hipStream_t {
                const int lam_side = t->knobs.lam_side;      // side streams used (the rest of the classes: the main stream).  One: the widest class beside the
                // three others in a row on the main stream -- c2 423.1 -> 426.5 rounds/s against three side streams, c1 / c3 / c1ns within their noise
                // (profiles/r05q_ab_lambda_side_*): the classes fill the chip either way, and a kernel that ends on a side stream is a cross-stream wait
                if (lam_used >= lam_side) return s;
                hipStream_t ls = t->lam_s[lam_used++];
                (void)hipStreamWaitEvent(ls, t->ev_lam_fork, 0);
                return ls;
            };
#define RL_LAUNCH_FUSED(BT, cls)                                                                                                             \
            if (d.n_qcls[cls] > 0) {                                                                                                         \
                hipStream_t ls = lam_stream();                                                                                               \
                if (cp) t->arms[RL_ARM_LAM_COMPACT]++; else if (mode_arm[mode] >= 0) t->arms[mode_arm[mode]]++;                               \
                t->arms[ls == s ? RL_ARM_LAM_ON_MAIN : RL_ARM_LAM_ON_SIDE]++;                                                                \
                if (cp) hipLaunchKernelGGL((k_lambda_fused<BT, 0, true>), dim3(d.n_qcls[cls]), dim3(BT), lds_of(BT), ls, g, (const int *)d.d_qcls[cls], d.n_qcls[cls]); \
                else if (mode == 0) hipLaunchKernelGGL((k_lambda_fused<BT, 0>), dim3(d.n_qcls[cls]), dim3(BT), lds_of(BT), ls, g, (const int *)d.d_qcls[cls], d.n_qcls[cls]); \
                else if (mode == 1) hipLaunchKernelGGL((k_lambda_fused<BT, 1>), dim3(d.n_qcls[cls]), dim3(BT), lds_of(BT), ls, g, (const int *)d.d_qcls[cls], d.n_qcls[cls]); \
                else if (mode == 2) hipLaunchKernelGGL((k_lambda_fused<BT, 2>), dim3(d.n_qcls[cls]), dim3(BT), lds_of(BT), ls, g, (const int *)d.d_qcls[cls], d.n_qcls[cls]); \
                else if (mode == 3) hipLaunchKernelGGL((k_lambda_fused<BT, 3>), dim3(d.n_qcls[cls]), dim3(BT), lds_of(BT), ls, g, (const int *)d.d_qcls[cls], d.n_qcls[cls]); \
                else hipLaunchKernelGGL((k_lambda_fused<BT, 4>), dim3(d.n_qcls[cls]), dim3(BT), lds_of(BT), ls, g, (const int *)d.d_qcls[cls], d.n_qcls[cls]); \
                n_max += d.n_qcls[cls]; g.blockmax = t->d_wmax + n_max;                                                                      \
            }
            if (d.n_qcls[4] > 0 && mode == 0) {
                const int nb = (d.n_qcls[4] + kLambdaTinyGroups - 1) / kLambdaTinyGroups;
                t->arms[RL_ARM_LAM_TINY]++; t->arms[RL_ARM_LAM_ON_MAIN]++;
                hipLaunchKernelGGL(k_lambda_tiny, dim3(nb), dim3(kLambdaTinyDocs * kLambdaTinyGroups),
                                   (size_t)kLambdaTinyGroups * lambda_tiny_group_bytes(c.k), s, g, (const int *)d.d_qcls[4], d.n_qcls[4]);
                n_max += nb; g.blockmax = t->d_wmax + n_max;
            } else {
                // ERR / MAP / P / RR: the lists of at most 16 documents take the block-per-query kernel too -- on the main stream: the side stream is for the
                // widest class below (ADVICE r05: the first class launched used to take it)
                const int keep = lam_used; lam_used = 1 << 20;
                RL_LAUNCH_FUSED(64, 4)
                lam_used = keep;
            }
            // longest lists first on the side streams (they take longest per block), the shortest class last on the main stream
            RL_LAUNCH_FUSED(256, 3)
            RL_LAUNCH_FUSED(192, 2)
            RL_LAUNCH_FUSED(128, 1)
            RL_LAUNCH_FUSED(64, 0)
#undef RL_LAUNCH_FUSED
            for (int i = 0; i < lam_used; i++) { RL_HIP(hipEventRecord(t->ev_lam_join[i], t->lam_s[i])); RL_HIP(hipStreamWaitEvent(s, t->ev_lam_join[i], 0)); }
        } else {
            const unsigned nb = (unsigned)((c.N + kThreads - 1) / kThreads);
            t->arms[RL_ARM_LAM_UNFUSED]++;
            hipLaunchKernelGGL(k_pair_terms, dim3(nb), dim3(kThreads), 0, s, g);
            hipLaunchKernelGGL(k_lambda_acc, dim3(nb), dim3(kThreads), 0, s, g);
            n_max = (int)nb;
        }
    }
    return RL_OK;
}

// ---- max |lambda| over the blocks (sharded: over the ranks), then the fixed-point lambdas unless the root pass makes them ----
static int enqueue_max_and_quant(rl_trainer *t, int n_max, bool &root_quant_fused)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    hipLaunchKernelGGL(k_max_reduce, dim3((unsigned)std::max(1, std::min(16, (n_max + 4095) / 4096))), dim3(1024), 0, s, (const double *)t->d_wmax, n_max, &c.st->maxabs_bits);
    if (t->dist) { int rcd = t->dist->allreduce(&c.st->maxabs_bits, 1, DT_U64, OP_MAX, s); if (rcd) return rcd; }
    // The plain one-GPU root pass makes the fixed-point lambdas itself (k_hist<.., FQ>): one pass over the documents and one launch less a round.
    // Sharded, strict-order and sparse-column runs (their kernels between here and the root pass read q) and a regrown tree (q exists) keep k_quantize.
    root_quant_fused = t->knobs.fused_quant && !c.java && !c.sp_on && c.sub == 16 && c.TS <= kHistLdsStride && !c.any_runs;       // (sharded runs too, round 6: max |lambda| is all-reduced before this point, nothing between here and the root pass reads q)
    if (!root_quant_fused) {
        t->arms[RL_ARM_QUANTIZE]++;
        hipLaunchKernelGGL(k_quantize, dim3(std::min(2048, (c.N + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, c);
    }
    return RL_OK;
}

// ---- the root: histogram pass, then the finish that picks the root's split and starts the tree (TreeState::tree_seq, mirrored in t->tree_seq) ----
static int enqueue_root(rl_trainer *t, const RoundPlan &pl, bool quant_fused)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    {   // K2 root histogram: dense groups from their 32-byte rows, groups of sparse columns from their entry lists (rl_csc.inc)
        const double root_bytes = c.sp_on ? (double)c.N * ((double)(c.numFG - c.sp_ngroups) * kHistFG * 2.0 + 8.0) + (double)t->sp_entries * 4.0
                                          : (double)c.N * ((double)c.F * 2.0 + 8.0);
        ScopedTiming tm(t, RL_KERNEL_HIST_ROOT, root_bytes);
        launch_hist<true>(c, t->knobs, t->arms, pl.hist_gx, pl.rootChunks, pl.hist_lds, s, quant_fused);
        if (c.sp_on) {
            hipLaunchKernelGGL(k_hist_sp<kHistLdsStride>, dim3(c.sp_ngroups, pl.rootChunks), dim3(kSpThreads), (size_t)kHistFG * kHistLdsStride * 8, s, c, pl.rootCs);
        }
    }
    if (t->dist) {
        hipLaunchKernelGGL(k_hist_reduce, dim3(c.F), dim3(kFinThreads), pl.red_lds, s, c, 1);
        int rcd = t->dist->allreduce(c.dist_buf, (size_t)c.F * c.TS * c.limb_words + 4, DT_I64, OP_SUM, s);
        if (rcd) return rcd;
        hipLaunchKernelGGL((k_hist_finish<true, true>), dim3(c.F), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    } else if (c.java) {
        hipLaunchKernelGGL(k_jgather, dim3((c.N + kPartTile - 1) / kPartTile), dim3(kThreads), 0, s, c, 1);
        if (c.jmap) hipLaunchKernelGGL(k_jhist2, dim3(c.n_live + 1, 1), dim3(kJ2Threads), 0, s, c, 1, c.jmap, c.jinv, c.jone);
        else hipLaunchKernelGGL(k_jhist, dim3(c.n_live, pl.jbg + 2, 1), dim3(64), 0, s, c, 1, pl.jbg);
        hipLaunchKernelGGL((k_hist_finish<true, false, true>), dim3(c.n_live), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    } else if (t->knobs.step2 && c.TS <= kFin2MaxT) {       // rl_step2.inc
        hipLaunchKernelGGL(k_fin2_root, dim3(c.n_live), dim3(kFin2RootThreads), 0, s, c, pl.rootChunks);
        hipLaunchKernelGGL(k_select_root, dim3(1), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    } else hipLaunchKernelGGL((k_hist_finish<true, false>), dim3(c.n_live), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    t->tree_seq++;
    return RL_OK;
}

// ---- growth ----------------------------------------------------------------------------------------------------------
// The host's state of one pass over a tree: made afresh for every pass (a tree grown again included), kept through a stall and its resumption.
// Lazy tie-break (rl_tie.inc): the device may STALL the tree (no slots, progress word bit 31) until resolve_ties has run.  Growth kernels
// enqueued meanwhile are no-ops; afterwards the host carries on from the device's own step count.  `extra`: the stalled select_step call and
// its resumption count as steps of the device without committing a split.
struct Growth {
    int it = 0, extra = 0;         // the growth step to enqueue next; steps allowed beyond RoundPlan::steps
    bool throttle;                 // follow the progress word (given up after a spin timeout: the rest is enqueued blindly)
    bool saw_end = false;          // the host has seen the tree's done flag
    bool defer_seen = false;       // the finished tree holds nodes whose stored threshold awaits the batched tie-break (progress word bit 30)
    explicit Growth(const Ctx &c) : throttle(c.progress != nullptr) {}
};
// what a look at the tree decided.  Go: enqueue growth step `it` (after a step: go on to it + 1); Again: look again at the same `it` (a stall was
// resolved, `it` is the device's own step now); Ended: the tree is finished
enum class Next { Go, Again, Ended };

static bool word_stalled(const rl_trainer *t, unsigned long long w) { return t->ctx.tie_on && (w >> 32) == t->tree_seq && ((w >> 31) & 1ull); }
static bool word_finished(const rl_trainer *t, unsigned long long w) { return (w >> 32) == t->tree_seq && (w & 1); }

// stream idle, tree stalled: resolve, then continue at the device's step
static int after_stall(rl_trainer *t, const RoundPlan &pl, Growth &g, Next &next)
{
    Ctx &c = t->ctx;
    int rcs = resolve_ties(t, pl.fin_lds, pl.nodes_in_lds);
    if (rcs) return rcs;
    g.extra += 2;
    bool ended, deferred;
    if (c.progress) {       // resolve_ties waited for k_tie_finish, whose select_step left (step, done, deferred ties) in the pinned progress word
        const unsigned long long w = __atomic_load_n(t->h_progress, __ATOMIC_ACQUIRE);
        if ((w >> 32) != t->tree_seq) return fail(RL_ERR_STATE, "tie-break: the progress word is not this tree's (internal error)");
        ended = (w & 1ull) != 0;
        deferred = ((w >> 30) & 1ull) != 0;
        g.it = (int)((unsigned)(w & 0x3fffffffull) >> 1);
    } else {
        TreeState sth;
        RL_HIP(hipMemcpy(&sth, c.st, sizeof(sth), hipMemcpyDeviceToHost));
        ended = sth.done != 0;
        deferred = sth.defer_any != 0;
        g.it = sth.step;
    }
    if (ended) g.defer_seen = deferred;
    next = ended ? Next::Ended : Next::Again;
    return RL_OK;
}

// The gate in front of growth step g.it: a stall seen in the progress word is resolved here; with the host more than `ahead` steps in front of the
// bookkeeping it has seen, wait for the progress word and take the tree's end or stall from it (sharded: only as of step g.it - ahead).
static int growth_gate(rl_trainer *t, const RoundPlan &pl, Growth &g, Next &next)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    next = Next::Go;
    if (g.throttle && c.tie_on && !t->dist) {
        const unsigned long long w0 = __atomic_load_n(t->h_progress, __ATOMIC_ACQUIRE);
        if (word_stalled(t, w0)) return after_stall(t, pl, g, next);       // (resolve_ties reads the tree state through the stream: no drain of its own needed here)
    }
    const int ahead = t->dist ? t->knobs.dist_ahead : t->knobs.step_ahead;
    if (!g.throttle || g.it < ahead) return RL_OK;
    // wait (bounded) until growth step it - step_ahead has been selected, then look at the tree's done flag.  Purely a
    // scheduling hint: on a timeout the remaining steps are enqueued blindly, which is always correct.
    const unsigned long long want = ((unsigned long long)t->tree_seq << 32) | ((unsigned long long)(unsigned)(g.it - ahead) << 1);
    unsigned long long w = __atomic_load_n(t->h_progress, __ATOMIC_ACQUIRE);
    if (t->dist) {
        // Deterministic over the ranks (they grow the same tree): wait -- without a timeout -- until growth step
        // it - step_ahead has been selected or the tree is finished, and stop only if the tree was finished by a step
        // <= it - step_ahead.  The word keeps (step at which `done` was set, done) once the tree is finished, so a rank
        // that looks early and one that looks late take the same decision at the same `it`.
        unsigned spins = 0;
        const auto t0w = std::chrono::steady_clock::now();
        while ((w & ~(3ull << 30)) < want && !word_finished(t, w) && !word_stalled(t, w)) {       // (bits 30 / 31 of the low word are flags)
            w = __atomic_load_n(t->h_progress, __ATOMIC_ACQUIRE);
            if ((++spins & 0xfffff) == 0) {
                const hipError_t q = hipStreamQuery(s);
                if (q != hipSuccess && q != hipErrorNotReady) return fail(RL_ERR_HIP, std::string("device error while growing a tree: ") + hipGetErrorString(q));
                // the wait ends when THIS rank's device finishes a growth step, which needs every other rank's share of the step's
                // collective: a rank that died or fell behind for good must surface as an error here, not as a hang
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0w).count() > t->knobs.dist_timeout_s)
                    return fail(RL_ERR_COMM, "timed out after " + std::to_string((int)t->knobs.dist_timeout_s) + " s waiting for growth step " + std::to_string(g.it - ahead) +
                                             " of tree " + std::to_string(t->tree_seq) + " (a rank of the job is missing from a collective?)");
            }
        }
        const int step_w = (int)((unsigned)(w & 0x3fffffffull) >> 1);
        if (word_finished(t, w) && step_w <= g.it - ahead) { g.defer_seen = ((w >> 30) & 1ull) != 0; next = Next::Ended; return RL_OK; }
        // a stalled tree (rl_tie.inc): the word keeps the step at which it stalled, so -- as for the end of the tree -- every rank acts on
        // it at the same `it`, after the same number of (empty) steps and their collectives
        if (word_stalled(t, w) && step_w <= g.it - ahead) return after_stall(t, pl, g, next);
    } else {
        // (bits 30 / 31 of the low word are flags: the step is compared field by field)
        const auto behind = [&](unsigned long long v) {
            if ((v >> 32) != t->tree_seq) return true;                   // still the previous tree's word
            return (unsigned)((v & 0x3fffffffull) >> 1) < (unsigned)(g.it - ahead) && !(v & 1) && !((v >> 31) & 1);
        };
        if (behind(w)) {
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (behind(w = __atomic_load_n(t->h_progress, __ATOMIC_ACQUIRE))) {
                if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) { g.throttle = false; break; }
            }
        }
        if (word_stalled(t, w)) next = Next::Again;       // handled at the top of the gate
        else if (word_finished(t, w)) { g.defer_seen = ((w >> 30) & 1ull) != 0; next = Next::Ended; }
    }
    return RL_OK;
}

// Growth step g.it: partition, child histograms, finish and bookkeeping by mode; a sharded run without a progress word looks at the tree state here.
static int enqueue_growth_step(rl_trainer *t, const RoundPlan &pl, Growth &g, Next &next)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    next = Next::Go;
    if (t->dist && !c.cum_cnt_loc) {      // local child sizes unknown in advance: count pass, then scatter (round 5; RLHIP_DIST_COUNT_PASS=1)
        hipLaunchKernelGGL(k_part_count, dim3(c.nTiles), dim3(kThreads), 0, s, c);
        hipLaunchKernelGGL(k_part_scatter<false>, dim3(c.nTiles), dim3(kThreads), 0, s, c);
    } else hipLaunchKernelGGL(k_part_scatter<true>, dim3(c.nTiles), dim3(kThreads), 0, s, c);
    t->arms[RL_ARM_STEPS_ENQUEUED]++;
    {
        ScopedTiming tm(t, RL_KERNEL_HIST_NODE, 0.0);
        launch_hist<false>(c, t->knobs, t->arms, pl.hist_gx, c.maxChunks, pl.hist_lds, s);
    }
    if (t->dist) {
        hipLaunchKernelGGL(k_hist_reduce, dim3(c.F, kSpec), dim3(kFinThreads), pl.red_lds, s, c, 0);
        // growth step `it` works on at most min(kSpec, 2^it) nodes (1 after the root, then at most twice the commits of the step
        // before): the first steps -- the ones with the largest histograms to wait for -- reduce one or two slots, not kSpec
        const int max_slots = std::min(kSpec, 1 << std::min(g.it, 8));
        int rcd = t->dist->allreduce(c.dist_buf, pl.slot_words * max_slots, DT_I64, OP_SUM, s);
        if (rcd) return rcd;
        // round 6: the finish and the bookkeeping of the plain path's step (rl_step2.inc) on the all-reduced limbs; the round-4 fused kernel for what
        // k_select2 does not cover (feature sampling, more than 160 features, more than 62 leaves)
        const size_t sel2_lds_d = select2_lds_bytes(c.L, c.NC);
        if (t->knobs.step2 && c.TS <= kFin2MaxT && !c.fs_on && c.F <= kSel2MaxF && c.L > 0 && c.L + 2 <= 64 && sel2_lds_d <= 60 * 1024) {
            hipLaunchKernelGGL(k_fin2<true>, dim3(c.F, kSpec), dim3(kFin2Threads), 0, s, c);
            hipLaunchKernelGGL(k_select2<false>, dim3(1), dim3(kSel2Threads), sel2_lds_d, s, c);
        } else hipLaunchKernelGGL((k_hist_finish<false, true>), dim3(c.F, kSpec), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
        // Sharded runs pay a collective per step even when the tree is already finished, so the host looks at the
        // (rank-invariant) `done` flag now and then and stops enqueuing: a stream sync costs far less than the
        // all-reduces of ~20 empty steps.  One GPU keeps the fully asynchronous schedule (an empty step is 3 tiny launches).
        if (!c.progress && g.it + 1 < pl.steps + g.extra && ((g.it >= 7 && (g.it - 7) % 3 == 0) || c.tie_on)) {
            TreeState sth;
            RL_HIP(hipStreamSynchronize(s));
            RL_HIP(hipMemcpy(&sth, c.st, sizeof(sth), hipMemcpyDeviceToHost));
            if (sth.stall_n > 0) return after_stall(t, pl, g, next);       // (without a progress word every step of a tie-breaking sharded run is looked at: rank-invariant by construction)
            if (sth.done) { g.defer_seen = sth.defer_any != 0; next = Next::Ended; }
        }
    } else if (c.java) {
        hipLaunchKernelGGL(k_jgather, dim3(c.nTiles), dim3(kThreads), 0, s, c, 0);
        if (c.jmap) hipLaunchKernelGGL(k_jhist2, dim3(c.n_live + 1, kSpec), dim3(kJ2Threads), 0, s, c, 0, c.jmap, c.jinv, c.jone);
        else hipLaunchKernelGGL(k_jhist, dim3(c.n_live, pl.jbg + 2, kSpec), dim3(64), 0, s, c, 0, pl.jbg);
        hipLaunchKernelGGL((k_hist_finish<false, false, true>), dim3(c.n_live, kSpec), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    } else if (t->knobs.step2 && c.TS <= kFin2MaxT) {
        // rl_step2.inc: one bin per thread, DPP scans, plain stores -- then the bookkeeping as a launch of its own
        hipLaunchKernelGGL(k_fin2<false>, dim3(c.n_live, kSpec), dim3(kFin2Threads), 0, s, c);
        const size_t sel2_lds = select2_lds_bytes(c.L, c.NC);
        if (!c.fs_on && c.F <= kSel2MaxF && c.L > 0 && c.L + 2 <= 64 && sel2_lds <= 60 * 1024)
            hipLaunchKernelGGL(k_select2<false>, dim3(1), dim3(kSel2Threads), sel2_lds, s, c);
        else if (t->knobs.sel2_wide && !c.fs_on && c.F <= 32 * kWideS && c.L > 0 && c.L + 2 <= 64 && sel2_lds <= 60 * 1024)
            hipLaunchKernelGGL(k_select2<true>, dim3(1), dim3(kSel2Threads), sel2_lds, s, c);       // (hundreds of features: the Yahoo-set1 shape)
        else hipLaunchKernelGGL(k_select, dim3(1), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    } else if (t->fin_split || !pl.nodes_in_lds) {       // (wide data; or node records that do not fit the LDS: the fused kernel has no path for them)
        hipLaunchKernelGGL(k_hist_finish_wide, dim3(c.n_live, kSpec), dim3(kFinWideThreads), (size_t)c.TS * 20 + 8 + pl.par_lds, s, c);
        hipLaunchKernelGGL(k_select, dim3(1), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    } else hipLaunchKernelGGL((k_hist_finish<false, false>), dim3(c.n_live, kSpec), dim3(kFinThreads), pl.fin_lds, s, c, pl.nodes_in_lds);
    return RL_OK;
}

// Grows the tree behind its root: gate and step until the tree has ended or every step is enqueued.
static int grow_tree(rl_trainer *t, const RoundPlan &pl, Growth &g)
{
    Ctx &c = t->ctx;
    for (;;) {
        while (g.it < pl.steps + g.extra) {
            Next next;
            int rc = growth_gate(t, pl, g, next);
            if (rc) return rc;
            if (next == Next::Go) { rc = enqueue_growth_step(t, pl, g, next); if (rc) return rc; }
            if (next == Next::Ended) { g.saw_end = true; break; }
            if (next == Next::Go) g.it++;
        }
        if (!c.tie_on || g.saw_end) return RL_OK;
        // every step was enqueued without the host ever seeing the end of the tree (no progress word, a spin timeout, or a tree of fewer steps
        // than the host keeps in flight): a stall may have gone unnoticed -- look, once per pass over the steps
        RL_HIP(hipStreamSynchronize(t->stream));
        TreeState sth;
        RL_HIP(hipMemcpy(&sth, c.st, sizeof(sth), hipMemcpyDeviceToHost));
        if (sth.stall_n == 0) { g.defer_seen = sth.defer_any != 0; return RL_OK; }
        Next next;
        int rcs = after_stall(t, pl, g, next);
        if (rcs) return rcs;
        if (next == Next::Ended) return RL_OK;       // (else: the steps from the device's own step on)
    }
}

// ---- the leaves' outputs -----------------------------------------------------------------------------------------
static int enqueue_leaf_outputs(rl_trainer *t, bool stream_scores)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    hipLaunchKernelGGL(k_leaf_table, dim3(1), dim3(kThreads), 0, s, c, t->leaf_chain, t->d_seg_buf);
    if (t->p.flags & RL_FLAG_SERIAL_CHAIN) {       // (the serial chain stores the outputs itself)
        hipLaunchKernelGGL(k_leaf_chain, dim3(c.L), dim3(64), 0, s, c);
        return RL_OK;
    }
    if (t->p.flags & RL_FLAG_FAST_LEAF) {
        // rl_fast_leaf.inc: the fixed f64 reduction over the leaf table k_leaf_table has just written; level 0 leaves every document's leaf behind
        // exactly as the float chains' gather does, so the score update takes the same kernel as in the default mode (the same bits either way)
        const FastLeafArgs fa{c.lw, c.idx[0], c.idx[1], t->d_seg_buf, c.leaf_start, &c.st->n_leaves, c.MAXN + 1, stream_scores ? c.leaf_of : nullptr,
                              t->d_fast_part, (int32_t)t->fast_slots, t->d_fast_sums, c.nodes, c.leaf_node, c.mart};
        hipLaunchKernelGGL(k_fast_leaf_tiles, dim3((unsigned)t->fast_slots), dim3(kFastTile), 0, s, fa);
        hipLaunchKernelGGL(k_fast_leaf_finish, dim3((unsigned)(c.MAXN + 1)), dim3(kFastTile), 0, s, fa);
        return RL_OK;
    }
    const ChainSource src{nullptr, nullptr, c.lw, c.idx[0], c.idx[1], t->d_seg_buf, stream_scores ? c.leaf_of : nullptr};
    const ChainBufs *sums = &t->leaf_chain;
    if (t->dist && t->piece_chains) {      // round 6: every rank evaluates its own pieces of every leaf, only tables travel (rl_dist.inc)
        int rcp = enqueue_leaf_chains_pieces(t, src);
        if (rcp) return rcp;
    } else if (t->dist) {      // the leaf-owner exchange (rl_dist.inc): lambda / weight of a leaf's documents go to the leaf's owner rank only
        int rco = enqueue_leaf_chains_owner(t, src);
        if (rco) return rco;
        sums = &t->gchain;
    } else enqueue_chain(t, t->leaf_chain, src);       // K7: the two Java float running sums of every leaf, exactly, in parallel (rl_chain.inc)
    hipLaunchKernelGGL(k_leaf_output, dim3((c.L + kThreads - 1) / kThreads), dim3(kThreads), 0, s, c, *sums);
    return RL_OK;
}

// ---- score update, the tree's export, the round's metrics --------------------------------------------------------
// (export_tree = false: a refit round, rl_refit.inc -- its tree is in t->ens already, with thresholds that are not in the trainer's own table)
static int enqueue_scores_and_metrics(rl_trainer *t, bool stream_scores, bool export_tree = true)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const int m = t->round;
    if (stream_scores) hipLaunchKernelGGL(k_score_stream, dim3(std::max(1, std::min(2048, (c.N + kScoreBatch * kThreads - 1) / (kScoreBatch * kThreads)))), dim3(kThreads), 0, s, c);
    else hipLaunchKernelGGL(k_score_update, dim3(std::max(1, std::min(4096, (c.N + kScoreBatch * kThreads - 1) / (kScoreBatch * kThreads)))), dim3(kThreads), 0, s, c);
    if (export_tree) hipLaunchKernelGGL(k_export_tree, dim3(1), dim3(kThreads), 0, s, c, t->ens, m);
    RL_HIP(hipGetLastError());
    // per-round training metric (LambdaMART.java:216)
    // (sharded runs, round 6: the per-query values are gathered on the main stream -- one communicator, one stream -- and the float mean over the
    // gathered lists runs on the side stream beside the next round's lambdas, as the one-GPU mean does)
    const bool use_side = !t->has_valid;
    if (use_side && t->side_pending) RL_HIP(hipStreamWaitEvent(s, t->ev_metric, 0));     // the previous round's metric still reads d_ndcg (sharded: the gathered copy)
    int rc = launch_rank(t, t->tr, c.scores, t->tr.d_ndcg, true);      // also the ranking of round m+1's lambdas
    if (rc != RL_OK) return rc;
    if (use_side) {
        const double *mq = t->tr.d_ndcg; int mQ = t->tr.Q;
        if (t->dist) { rc = gather_queries(t, t->tr.d_ndcg, &mq); if (rc != RL_OK) return rc; mQ = t->Qglobal; }
        RL_HIP(hipEventRecord(t->ev_ranked, s));
        RL_HIP(hipStreamWaitEvent(t->side, t->ev_ranked, 0));
        enqueue_metric_mean(t, mq, mQ, c.round_metric + 2 * (size_t)m, t->side);
        RL_HIP(hipEventRecord(t->ev_metric, t->side));
        t->side_pending = true;
    } else if (t->dist) {
        const double *gq = nullptr;
        rc = gather_queries(t, t->tr.d_ndcg, &gq);
        if (rc != RL_OK) return rc;
        enqueue_metric_mean(t, gq, t->Qglobal, c.round_metric + 2 * (size_t)m);
    } else enqueue_metric_mean(t, t->tr.d_ndcg, t->tr.Q, c.round_metric + 2 * (size_t)m);
    if (t->has_valid) {   // :228-237
        hipLaunchKernelGGL(k_valid_update, dim3(std::min<int64_t>(4096, (t->va.N + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                           t->ens, c.MAXN, m, (const float *)t->va.d_X, (int)t->va.N, t->F, c.lr, t->va.d_scores);
        rc = launch_rank(t, t->va, t->va.d_scores, t->va.d_ndcg, false);
        if (rc != RL_OK) return rc;
        if (t->dist) {      // every rank holds a shard of the validation lists: the float mean runs over all of them in list order
            const double *gq = nullptr;
            rc = gather_queries(t, t->va.d_ndcg, &gq, true);
            if (rc != RL_OK) return rc;
            enqueue_metric_mean(t, gq, t->vQglobal, c.round_metric + 2 * (size_t)m + 1);
        } else enqueue_metric_mean(t, t->va.d_ndcg, t->va.Q, c.round_metric + 2 * (size_t)m + 1);
    }
    RL_HIP(hipGetLastError());
    t->round = m + 1;
    t->n_kept = t->round;
    return RL_OK;
}

// the score update streams over the documents when the leaf sums' gather can leave every document's leaf behind (one GPU, parallel chains, <= 1024 leaves)
static bool round_streams_scores(const rl_trainer *t)
{
    const Ctx &c = t->ctx;
    return t->knobs.score_stream && !(t->p.flags & RL_FLAG_SERIAL_CHAIN) && c.leaf_of != nullptr && c.L > 0 && c.L <= 1024;       // (sharded runs too, round 6: the local gather in leaf order leaves every document's leaf behind)
}

static int enqueue_round(rl_trainer *t)
{
    Ctx &c = t->ctx;
    // (a tree is grown a second time, from its root histogram, when the deferred tie-break finds that a tie over several features it took for one
    // cut is not one -- rl_tie.inc, k_tie_verify; nothing a round keeps has been written by then)
    const int tie_mode = c.tie_on;
    struct TieModeRestore { Ctx &c; int v; ~TieModeRestore() { c.tie_on = v; } } tie_mode_restore{c, tie_mode};
    const bool stream_scores = round_streams_scores(t);
    RoundPlan pl;
    int rc = round_plan(t, pl);
    if (rc) return rc;
    int n_max = 0;
    bool root_quant_fused = false;
    if ((rc = enqueue_lambdas(t, n_max)) != RL_OK) return rc;
    if ((rc = enqueue_max_and_quant(t, n_max, root_quant_fused)) != RL_OK) return rc;
    for (;;) {      // one pass per growth of the tree
        if ((rc = enqueue_root(t, pl, root_quant_fused)) != RL_OK) return rc;
        root_quant_fused = false;        // (a regrown tree reads the q / r the first root pass has stored)
        Growth g(c);
        if ((rc = grow_tree(t, pl, g)) != RL_OK) return rc;
        if ((rc = enqueue_leaf_outputs(t, stream_scores)) != RL_OK) return rc;
        if (!c.tie_on || !g.defer_seen) break;
        // deferred ties (plateaus of right children, several features over one cut): the tree was grown with the partition the tied candidates
        // share; the (feature, threshold) the Java's rounding noise would store is decided now, in one batch (the leaf sums above are already
        // enqueued and run meanwhile; the score update waits, because a tie that turns out to hide two different cuts restarts the tree)
        bool other_cut = false;
        if ((rc = resolve_ties(t, pl.fin_lds, pl.nodes_in_lds, true, &other_cut)) != RL_OK) return rc;
        if (!other_cut || !(c.tie_on & 2)) break;
        c.tie_on = 1; t->tie_regrown++;
    }
    return enqueue_scores_and_metrics(t, stream_scores);
}

}  // namespace rl
