// rl_chain_host.inc -- the host side of the exact parallel float chains: the Java's float running sums over a leaf's samples
// (LambdaMART.java:401-413) and over the per-query metric (LambdaMART.java:469-471), evaluated in parallel yet bit for bit.  Included by
// rl_trainer.hip behind `struct rl_trainer` and the timing helpers; needs the struct, fail() / RL_HIP, and the kernels of rl_chain.inc,
// rl_dist.inc and rl_k_leaf.inc, all ahead of the struct.
//
//   chain_stitch_lds, alloc_chain      the LDS a stitch needs; the buffers of one ChainBufs out of the trainer's pool (no kernel)
//   spin_until                         bounded wait on the pinned progress word (no kernel)
//   enqueue_chain                      one whole evaluation, rl_chain.inc: k_chain_prefix, k_chain_scan_tiles, k_chain_bounds, k_chain_pass1<false>,
//                                      k_chain_guess, k_chain_tables<false>, k_chain_compose, k_chain_stitch; per repair pass k_chain_pass1<true>,
//                                      k_chain_recentre, k_chain_tables<true>, k_chain_compose, k_chain_stitch; k_chain_fallback unless seen clean
//   chain_repair_rounds                the repair passes alone (the same five kernels of rl_chain.inc, then k_chain_fallback), for pieces
//   enqueue_leaf_chains_pieces         rl_chain.inc's kernels as in enqueue_chain, interleaved with rl_dist.inc's k_piece_totals, k_piece_base,
//                                      k_piece_drifts, k_chain_cross, and per round k_chain_arm, chain_repair_rounds, k_chain_resolved, k_chain_cross
//   enqueue_leaf_chains_owner          k_chain_prefix (rl_chain.inc); rl_dist.inc: k_plan_exchange (or the host plan), k_chain_pack, k_plan_global,
//                                      k_chain_assemble; enqueue_chain on the owner's whole leaves; k_chain_pick (rl_dist.inc)
//   enqueue_metric_mean                k_float_mean (rl_k_leaf.inc) for short or serial runs, else k_plan_single (rl_chain.inc), enqueue_chain,
//                                      k_metric_finish (rl_k_leaf.inc)
//
// The two enqueue_leaf_chains_* are the two ways a sharded run sums its leaves.  _pieces keeps every document on its rank: each rank evaluates
// its own piece of every leaf and the pieces' transition tables are gathered and crossed, with repair rounds until every piece's start state
// is exact.  _owner sends a leaf's lambda / weight values to one owner rank, which evaluates the whole leaf as a single-GPU run would, and the
// 2 L float sums come back to every rank.  enqueue_round (rl_round.inc) chooses between them.

namespace rl {

// ---- exact parallel float chains (rl_chain.inc) ------------------------------------------------------
static size_t chain_stitch_lds(const ChainBufs &b)
{
    const size_t ng1 = (size_t)(b.cap_chunks / b.group + 2), ng2 = ng1 / kChainSuper + 2;
    return (ng1 * (kChainW + 1) + ng2 * kChainW) * sizeof(uint32_t);
}

static int alloc_chain(rl_trainer *t, ChainBufs &b, int maxseg, int A, int64_t n, bool hint = false)
{
    memset(&b, 0, sizeof(b));
    b.maxseg = maxseg; b.A = A;
    b.cap_tiles = n / kChainTile + maxseg + 2;
    b.cap_chunks = b.cap_tiles + maxseg + 2;
    b.cap_n = std::max<int64_t>(n, b.cap_chunks);
    // stitch tables in LDS: first-level groups of `group` chunks (the smaller the group, the shorter the chain of dependent loads)
    b.group = kChainBlock;
    while (chain_stitch_lds(b) > 152 * 1024) {
        b.group *= 2;
        if (b.group > 65536) return fail(RL_ERR_UNSUPPORTED, "data set too large for the float-chain stitch kernel");
    }
    RL_HIP(t->pool.alloc(&b.plan, (size_t)1));
    RL_HIP(t->pool.alloc(&b.seg_start, (size_t)maxseg + 2)); RL_HIP(t->pool.alloc(&b.seg_tile0, (size_t)maxseg + 2));
    RL_HIP(t->pool.alloc(&b.xs, (size_t)A * b.cap_n)); RL_HIP(t->pool.alloc(&b.pre, (size_t)A * b.cap_n));
    RL_HIP(t->pool.alloc(&b.tile_tot, (size_t)A * b.cap_tiles)); RL_HIP(t->pool.alloc(&b.tile_base, (size_t)A * b.cap_tiles));
    RL_HIP(t->pool.alloc(&b.bnd, (size_t)A * b.cap_tiles));
    RL_HIP(t->pool.alloc(&b.cbase, (size_t)A * b.cap_chunks)); RL_HIP(t->pool.alloc(&b.drift, (size_t)A * b.cap_chunks));
    RL_HIP(t->pool.alloc(&b.drift2, (size_t)A * b.cap_chunks));
    RL_HIP(t->pool.alloc(&b.gkey, (size_t)A * b.cap_chunks)); RL_HIP(t->pool.alloc(&b.gkey2, (size_t)A * b.cap_chunks));
    RL_HIP(t->pool.alloc(&b.R, (size_t)A * b.cap_chunks * kChainW));
    RL_HIP(t->pool.alloc(&b.comp0, (size_t)A * (b.cap_chunks / kChainBlock + 1) * kChainW));
    RL_HIP(t->pool.alloc(&b.result, (size_t)A * maxseg)); RL_HIP(t->pool.alloc(&b.miss, (size_t)A * maxseg));
    RL_HIP(t->pool.alloc(&b.st_status, (size_t)A * maxseg)); RL_HIP(t->pool.alloc(&b.st_chunk, (size_t)A * maxseg));
    RL_HIP(t->pool.alloc(&b.st_key, (size_t)A * maxseg)); RL_HIP(t->pool.alloc(&b.st_delta, (size_t)A * maxseg));
    RL_HIP(t->pool.alloc(&b.st_win, (size_t)A * maxseg));
    b.lds_words = (int32_t)(chain_stitch_lds(b) / 4);
    RL_HIP(hipMemset(b.st_status, 0, (size_t)A * maxseg * sizeof(int32_t)));
    RL_HIP(hipMemset(b.miss, 0, (size_t)A * maxseg * sizeof(int32_t)));
    RL_HIP(t->pool.alloc(&b.arrive, (size_t)1)); RL_HIP(hipMemset(b.arrive, 0, sizeof(unsigned long long)));
    if (hint) {      // optional, like the trainer's progress word
        if (hipHostMalloc((void **)&b.h_progress, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            *b.h_progress = 0;
            t->pinned.push_back(b.h_progress);
            if (hipHostGetDevicePointer((void **)&b.progress, b.h_progress, 0) != hipSuccess) { b.progress = nullptr; b.h_progress = nullptr; (void)hipGetLastError(); }
        } else { b.h_progress = nullptr; (void)hipGetLastError(); }
    }
    RL_HIP(t->pool.alloc(&b.stats, (size_t)4));
    RL_HIP(hipMemset(b.stats, 0, 4 * sizeof(int32_t)));
    RL_HIP(hipMemset(b.plan, 0, sizeof(ChainPlan)));
    return RL_OK;
}

// the plan must already be on the device (k_leaf_table / k_plan_single); grids are sized by capacity
// bounded wait on a pinned progress word written by the device (a scheduling hint, never a correctness dependency)
template <class Pred>
static bool spin_until(const unsigned long long *word, Pred ok, unsigned long long &w)
{
    w = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    if (ok(w)) return true;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; spins++) {
        w = __atomic_load_n(word, __ATOMIC_ACQUIRE);
        if (ok(w)) return true;
        if ((spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) return false;
    }
}

static void enqueue_chain(rl_trainer *t, const ChainBufs &b_in, const ChainSource &src, hipStream_t s = nullptr)
{
    if (!s) s = t->stream;
    // The device cuts its repair passes into windows (kChainWinMax chunks) only when the host watches them and keeps repairing (the progress word);
    // a host that enqueues its passes blindly (no pinned word, RLHIP_STEP_AHEAD=0) gets passes that rebuild everything that remains -- otherwise a
    // chain longer than kChainRepairs windows ended in the serial fallback (exact, but ~100 ms for a 40 M-document leaf).
    ChainBufs b = b_in;
    if (!(b.h_progress != nullptr && t->knobs.step_ahead > 0)) { b.progress = nullptr; b.h_progress = nullptr; }
    const unsigned tb = (unsigned)((b.cap_tiles + 3) / 4);
    hipLaunchKernelGGL(k_chain_prefix, dim3(tb), dim3(kThreads), 0, s, b, src);
    hipLaunchKernelGGL(k_chain_scan_tiles, dim3(b.A), dim3(kScanThreads), 0, s, b);
    hipLaunchKernelGGL(k_chain_bounds, dim3(tb, b.A), dim3(kThreads), 0, s, b);
    const dim3 p1grid((unsigned)((b.cap_chunks * 16 + kThreads - 1) / kThreads), b.A);
    hipLaunchKernelGGL(k_chain_pass1<false>, p1grid, dim3(kThreads), 0, s, b);
    hipLaunchKernelGGL(k_chain_guess, dim3(b.A), dim3(kScanThreads), 0, s, b);
    const dim3 tgrid((unsigned)((b.cap_chunks + kThreads / 64 - 1) / (kThreads / 64)), b.A);       // one wavefront per chunk
    const size_t lds = chain_stitch_lds(b);
    // every stitch pass carries a tag; with a progress word (ChainBufs::h_progress) the host looks at the result of the pass
    // before the last one it enqueued and leaves the remaining repair passes (near-empty launches) away once nothing is open
    const unsigned long long seq = ++t->chain_seq;
    t->chain_calls[b.h_progress ? 0 : 1]++;
    bool hint = b.h_progress != nullptr && t->knobs.step_ahead > 0, clean = false;
    const dim3 cgrid((unsigned)((b.cap_chunks / kChainBlock + kThreads / 64) / (kThreads / 64)), b.A);       // one wavefront per block of kChainBlock chunks
    hipLaunchKernelGGL(k_chain_tables<false>, tgrid, dim3(kThreads), 0, s, b, 0);
    hipLaunchKernelGGL(k_chain_compose, cgrid, dim3(kThreads), 0, s, b, 0);
    hipLaunchKernelGGL(k_chain_stitch, dim3(b.maxseg, b.A), dim3(kScanThreads), lds, s, b, 0, seq << 16);
    // With the hint the host sees every stitch's outcome before it enqueues the next repair pass, so it repairs for as long as a segment is open
    // (a chain of tens of millions of elements needs a pass per window of 8192 chunks and one per window miss; the serial finish of a chain
    // that long costs 100 ms) and enqueues nothing on a clean round; without it exactly kChainRepairs passes are enqueued blindly.
    for (int rep = 0; rep < (hint ? kChainRepairsMax : kChainRepairs); rep++) {
        if (hint) {      // (a repair pass is four launches: none is enqueued before the stitch it would repair has reported)
            const unsigned long long want = (seq << 16) | (unsigned)rep;            // the stitch before repair pass rep (0 = the first stitch)
            unsigned long long w;
            const auto tw0 = std::chrono::steady_clock::now();
            const bool seen = spin_until(b.h_progress, [&](unsigned long long v) { return (v >> 1) >= want; }, w);
            t->chain_wait_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - tw0).count();
            if (!seen) { hint = false; t->chain_timeouts++; }
            else if ((w >> 17) == seq && !(w & 1)) { clean = true; break; }
        }
        t->chain_repairs[b.h_progress ? 0 : 1]++;
        hipLaunchKernelGGL(k_chain_pass1<true>, p1grid, dim3(kThreads), 0, s, b);
        hipLaunchKernelGGL(k_chain_recentre, dim3(b.maxseg, b.A), dim3(kScanThreads), 0, s, b);
        hipLaunchKernelGGL(k_chain_tables<true>, tgrid, dim3(kThreads), 0, s, b, 1);
        hipLaunchKernelGGL(k_chain_compose, cgrid, dim3(kThreads), 0, s, b, 1);
        hipLaunchKernelGGL(k_chain_stitch, dim3(b.maxseg, b.A), dim3(kScanThreads), lds, s, b, 1, (seq << 16) | (unsigned)(rep + 1));
    }
    if (!clean) hipLaunchKernelGGL(k_chain_fallback, dim3(b.maxseg, b.A), dim3(64), 0, s, b);
}

// float s = 0; for (q) s += ndcg_q; s / Q   -- serial for short lists, exact parallel chain otherwise
// the ordinary repair passes on the segments k_chain_arm has opened (exact start states known), until the host has seen them closed
static void chain_repair_rounds(rl_trainer *t, const ChainBufs &b, hipStream_t s)
{
    const dim3 p1grid((unsigned)((b.cap_chunks * 16 + kThreads - 1) / kThreads), b.A);
    const dim3 tgrid((unsigned)((b.cap_chunks + kThreads / 64 - 1) / (kThreads / 64)), b.A);
    const dim3 cgrid((unsigned)((b.cap_chunks / kChainBlock + kThreads / 64) / (kThreads / 64)), b.A);
    const size_t lds = chain_stitch_lds(b);
    const unsigned long long seq = ++t->chain_seq;
    bool hint = b.h_progress != nullptr && t->knobs.step_ahead > 0, clean = false;
    for (int rep = 0; rep < (hint ? kChainRepairsMax : kChainRepairs); rep++) {
        t->chain_repairs[b.h_progress ? 0 : 1]++;
        hipLaunchKernelGGL(k_chain_pass1<true>, p1grid, dim3(kThreads), 0, s, b);
        hipLaunchKernelGGL(k_chain_recentre, dim3(b.maxseg, b.A), dim3(kScanThreads), 0, s, b);
        hipLaunchKernelGGL(k_chain_tables<true>, tgrid, dim3(kThreads), 0, s, b, 1);
        hipLaunchKernelGGL(k_chain_compose, cgrid, dim3(kThreads), 0, s, b, 1);
        hipLaunchKernelGGL(k_chain_stitch, dim3(b.maxseg, b.A), dim3(kScanThreads), lds, s, b, 1, (seq << 16) | (unsigned)(rep + 1));
        if (hint) {
            const unsigned long long want = (seq << 16) | (unsigned)(rep + 1);
            unsigned long long w;
            const bool seen = spin_until(b.h_progress, [&](unsigned long long v) { return (v >> 1) >= want; }, w);
            if (!seen) { hint = false; t->chain_timeouts++; }
            else if ((w >> 17) == seq && !(w & 1)) { clean = true; break; }
        }
    }
    if (!clean) hipLaunchKernelGGL(k_chain_fallback, dim3(b.maxseg, b.A), dim3(64), 0, s, b);
}

// Sharded runs, round 6: the leaves' float sums from this rank's own pieces (rl_dist.inc, "piece mode"): three small all-gathers, no document leaves its rank.
static int enqueue_leaf_chains_pieces(rl_trainer *t, const ChainSource &src)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    ChainBufs b = t->leaf_chain;
    if (!(b.h_progress != nullptr && t->knobs.step_ahead > 0)) { b.progress = nullptr; b.h_progress = nullptr; }
    const int R = t->n_ranks, me = t->dist->rank, A = b.A, MS = b.maxseg, nseg = std::max(c.L, 2), n = A * MS;
    int rcd = t->dist->allgather(c.leaf_start, t->d_gls, (size_t)t->lsstride * sizeof(int32_t), s);       // the pieces' lengths on every rank
    if (rcd) return rcd;
    const unsigned tb = (unsigned)((b.cap_tiles + 3) / 4), nb = (unsigned)((n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_chain_prefix, dim3(tb), dim3(kThreads), 0, s, b, src);
    hipLaunchKernelGGL(k_chain_scan_tiles, dim3(b.A), dim3(kScanThreads), 0, s, b);
    hipLaunchKernelGGL(k_piece_totals, dim3(nb), dim3(kThreads), 0, s, b, t->d_pc_loc);
    rcd = t->dist->allgather(t->d_pc_loc, t->d_pc_all, (size_t)n * sizeof(double), s);
    if (rcd) return rcd;
    hipLaunchKernelGGL(k_piece_base, dim3(nb), dim3(kThreads), 0, s, (const double *)t->d_pc_all, n, me, t->d_pc_base, 0);
    b.seg_base = t->d_pc_base; b.ptab = t->d_ptab;
    hipLaunchKernelGGL(k_chain_bounds, dim3(tb, b.A), dim3(kThreads), 0, s, b);
    const dim3 p1grid((unsigned)((b.cap_chunks * 16 + kThreads - 1) / kThreads), b.A);
    hipLaunchKernelGGL(k_chain_pass1<false>, p1grid, dim3(kThreads), 0, s, b);
    hipLaunchKernelGGL(k_piece_drifts, dim3(MS, b.A), dim3(64), 0, s, b, t->d_pc_loc);
    rcd = t->dist->allgather(t->d_pc_loc, t->d_pc_all, (size_t)n * sizeof(double), s);
    if (rcd) return rcd;
    hipLaunchKernelGGL(k_piece_base, dim3(nb), dim3(kThreads), 0, s, (const double *)t->d_pc_all, n, me, t->d_pc_base, 1);
    hipLaunchKernelGGL(k_chain_guess, dim3(b.A), dim3(kScanThreads), 0, s, b);
    const dim3 tgrid((unsigned)((b.cap_chunks + kThreads / 64 - 1) / (kThreads / 64)), b.A);
    const dim3 cgrid((unsigned)((b.cap_chunks / kChainBlock + kThreads / 64) / (kThreads / 64)), b.A);
    const size_t lds = chain_stitch_lds(b);
    const unsigned long long seq = ++t->chain_seq;
    t->chain_calls[b.h_progress ? 0 : 1]++;
    hipLaunchKernelGGL(k_chain_tables<false>, tgrid, dim3(kThreads), 0, s, b, 0);
    hipLaunchKernelGGL(k_chain_compose, cgrid, dim3(kThreads), 0, s, b, 0);
    hipLaunchKernelGGL(k_chain_stitch, dim3(b.maxseg, b.A), dim3(kScanThreads), lds, s, b, 0, seq << 16);
    rcd = t->dist->allgather(t->d_ptab, t->d_gtab, (size_t)n * (kChainW + 1) * sizeof(uint32_t), s);
    if (rcd) return rcd;
    hipLaunchKernelGGL(k_chain_cross, dim3(1), dim3(kThreads), 0, s, (const uint32_t *)t->d_gtab, (const int32_t *)t->d_gls, t->lsstride, R, nseg, A, MS, me, t->xstate,
                       (const uint32_t *)t->d_res_all, 0, t->knobs.piece_force, b.result, t->d_xmail, ++t->xmail_tag);
    ChainBufs br = b; br.ptab = nullptr;            // (the repair passes stitch from ONE known state)
    for (int round = 0;; round++) {
        // every rank sees the same gathered tables, hence the same pending pieces: the rounds of this loop -- and their collectives -- are the same everywhere
        const auto t0w = std::chrono::steady_clock::now();
        unsigned spins = 0;
        while (__atomic_load_n(&t->h_xmail[2], __ATOMIC_ACQUIRE) != t->xmail_tag) {
            if ((++spins & 0xffff) == 0) {
                const hipError_t q = hipStreamQuery(s);
                if (q != hipSuccess && q != hipErrorNotReady) return fail(RL_ERR_HIP, std::string("device error in the leaves' float chains: ") + hipGetErrorString(q));
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0w).count() > t->knobs.dist_timeout_s)
                    return fail(RL_ERR_COMM, "timed out waiting for the leaves' float chains (a rank of the job is missing from a collective?)");
            }
        }
        const long long pend = t->h_xmail[0], mine = t->h_xmail[1];
        if (pend == 0) break;
        if (round > R * n + 8) return fail(RL_ERR_STATE, "the leaves' float chains did not close (internal error)");
        t->piece_rounds++; t->piece_misses += pend;
        hipLaunchKernelGGL(k_chain_arm, dim3(1), dim3(kThreads), 0, s, br, t->xstate, me, br.progress ? 1 : 0);
        if (mine > 0) chain_repair_rounds(t, br, s);
        hipLaunchKernelGGL(k_chain_resolved, dim3(1), dim3(kThreads), 0, s, br, t->xstate, me, t->d_res_loc);
        rcd = t->dist->allgather(t->d_res_loc, t->d_res_all, (size_t)n * sizeof(uint32_t), s);
        if (rcd) return rcd;
        hipLaunchKernelGGL(k_chain_cross, dim3(1), dim3(kThreads), 0, s, (const uint32_t *)t->d_gtab, (const int32_t *)t->d_gls, t->lsstride, R, nseg, A, MS, me, t->xstate,
                           (const uint32_t *)t->d_res_all, 1, t->knobs.piece_force, b.result, t->d_xmail, ++t->xmail_tag);
    }
    return RL_OK;
}

// Sharded runs, the leaf-owner exchange (rl_dist.inc): lambda / weight of a leaf's documents go to the leaf's owner rank only, which evaluates the
// chains over the whole leaf (t->gchain); the 2 L float sums come back to every rank.
static int enqueue_leaf_chains_owner(rl_trainer *t, const ChainSource &src)
{
    Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const ChainBufs &lb = t->leaf_chain;
    const int R = t->n_ranks, me = t->dist->rank, nseg = std::max(c.L, 2), MS = t->gchain.maxseg;      // -leaf 1 still has two leaves (the root always splits)
    hipLaunchKernelGGL(k_chain_prefix, dim3((unsigned)((lb.cap_tiles + 3) / 4)), dim3(kThreads), 0, s, lb, src);      // local values in leaf order -> lb.xs
    int rcd = t->dist->allgather(c.leaf_start, t->d_gls, (size_t)t->lsstride * sizeof(int32_t), s);
    if (rcd) return rcd;
    std::vector<int64_t> scount(R), sdispl(R), rcount(R), rdispl(R);
    const bool dev_plan = t->d_xmail != nullptr && !t->knobs.dist_host_plan && nseg <= kPlanMaxSeg && R <= 64;       // (knobs.dist_host_plan: the host plan behind a stream synchronisation, as until round 5)
    t->arms[dev_plan ? RL_ARM_XPLAN_DEVICE : RL_ARM_XPLAN_HOST]++;
    if (dev_plan) {
        // the plan on the device; the host only needs the byte counts of the transfers and reads them from a pinned mailbox below, after it has
        // enqueued the pack kernel (k_plan_exchange)
        hipLaunchKernelGGL(k_plan_exchange, dim3(1), dim3(64), 0, s, (const int32_t *)t->d_gls, R, t->lsstride, nseg, MS, me, t->d_own, t->d_xtab, t->d_xmail, ++t->xmail_tag);
    } else {
        // the send / receive counts of the exchange have to be known to the host: one small copy per round (sharded runs are host-paced anyway)
        std::vector<int32_t> &gls = t->h_gls;
        gls.resize((size_t)R * t->lsstride);
        RL_HIP(hipMemcpyAsync(gls.data(), t->d_gls, gls.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        auto len_of = [&](int r, int l) { return (long long)gls[(size_t)r * t->lsstride + l + 1] - gls[(size_t)r * t->lsstride + l]; };
        std::vector<int32_t> &own = t->h_own; own.assign((size_t)MS, 0);
        {   // owners: largest leaf first onto the least loaded rank (every rank computes the same map from the same table)
            std::vector<long long> glen((size_t)nseg, 0), load((size_t)R, 0);
            std::vector<int32_t> order((size_t)nseg);
            for (int l = 0; l < nseg; l++) { order[l] = l; for (int r = 0; r < R; r++) glen[l] += len_of(r, l); }
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return glen[a] > glen[b]; });
            for (int l : order) {
                if (glen[l] == 0) { own[l] = l % R; continue; }
                int o = 0;
                for (int r = 1; r < R; r++) if (load[r] < load[o]) o = r;
                own[l] = o; load[o] += glen[l];
            }
        }
        std::vector<long long> &tab = t->h_xtab; tab.assign((size_t)MS * (R + 1), 0);       // pack_off [MS] | asm_off [R][MS]
        long long cur = 0;
        for (int d = 0; d < R; d++) {
            sdispl[d] = cur * 8;
            if (d != me) for (int l = 0; l < nseg; l++) if (own[l] == d) { tab[l] = cur; cur += 2 * len_of(me, l); }       // (own leaves: not packed, k_chain_assemble)
            scount[d] = cur * 8 - sdispl[d];
        }
        cur = 0;
        for (int r = 0; r < R; r++) {
            rdispl[r] = cur * 8;
            if (r != me) for (int l = 0; l < nseg; l++) if (own[l] == me) { tab[(size_t)MS * (1 + r) + l] = cur; cur += 2 * len_of(r, l); }
            rcount[r] = cur * 8 - rdispl[r];
        }
        RL_HIP(hipMemcpyAsync(t->d_own, own.data(), (size_t)MS * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RL_HIP(hipMemcpyAsync(t->d_xtab, tab.data(), tab.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    }
    const LeafExchange lx{t->d_own, t->d_xtab, t->d_xtab + MS};
    hipLaunchKernelGGL(k_chain_pack, dim3(nseg, 2, kLeafXferZ), dim3(kThreads), 0, s, (const double *)lb.xs, lb.cap_n, (const int32_t *)c.leaf_start, nseg, lx, t->d_send, me);
    if (dev_plan) {       // the mailbox: the tag is stored last (release); a device error or a dead peer must end the wait
        const auto t0w = std::chrono::steady_clock::now();
        unsigned spins = 0;
        while (__atomic_load_n(&t->h_xmail[4 * R], __ATOMIC_ACQUIRE) != t->xmail_tag) {
            if ((++spins & 0xffff) == 0) {
                const hipError_t q = hipStreamQuery(s);
                if (q != hipSuccess && q != hipErrorNotReady) return fail(RL_ERR_HIP, std::string("device error before the leaf-owner exchange: ") + hipGetErrorString(q));
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0w).count() > t->knobs.dist_timeout_s)
                    return fail(RL_ERR_COMM, "timed out waiting for the plan of the leaf-owner exchange (a rank of the job is missing from a collective?)");
            }
        }
        for (int r = 0; r < R; r++) { scount[r] = t->h_xmail[r]; sdispl[r] = t->h_xmail[R + r]; rcount[r] = t->h_xmail[2 * R + r]; rdispl[r] = t->h_xmail[3 * R + r]; }
    }
    rcd = t->dist->alltoallv(t->d_send, scount.data(), sdispl.data(), t->d_gx, rcount.data(), rdispl.data(), s);
    if (rcd) return rcd;
    hipLaunchKernelGGL(k_plan_global, dim3(1), dim3(64), 0, s, (const int32_t *)t->d_gls, R, t->lsstride, nseg, t->gchain, (const int32_t *)t->d_own, me);
    hipLaunchKernelGGL(k_chain_assemble, dim3(nseg, 2, kLeafXferZ), dim3(kThreads), 0, s, (const double *)t->d_gx, (const int32_t *)t->d_gls, R, t->lsstride, nseg, lx,
                       t->gchain, me, (const double *)lb.xs, lb.cap_n, (const int32_t *)c.leaf_start);
    ChainSource gsrc{t->gchain.xs, t->gchain.xs + t->gchain.cap_n, nullptr, nullptr, nullptr, nullptr};
    enqueue_chain(t, t->gchain, gsrc);
    if (R > 1) {       // every rank evaluated its own leaves: exchange the 2 L float sums
        rcd = t->dist->allgather(t->gchain.result, t->d_gres, (size_t)2 * MS * sizeof(float), s);
        if (rcd) return rcd;
        hipLaunchKernelGGL(k_chain_pick, dim3((2 * nseg + kThreads - 1) / kThreads), dim3(kThreads), 0, s, (const float *)t->d_gres, R, 2,
                           MS, nseg, (const int32_t *)t->d_own, t->gchain.result);
    }
    return RL_OK;
}

static void enqueue_metric_mean(rl_trainer *t, const double *ndcg_q, int Q, float *out, hipStream_t s = nullptr)
{
    if (!s) s = t->stream;
    if (Q <= 4096 || (t->p.flags & RL_FLAG_SERIAL_CHAIN)) { hipLaunchKernelGGL(k_float_mean, dim3(1), dim3(64), 0, s, ndcg_q, Q, out); return; }
    hipLaunchKernelGGL(k_plan_single, dim3(1), dim3(64), 0, s, t->metric_chain, Q);
    ChainSource src{ndcg_q, nullptr, nullptr, nullptr, nullptr, nullptr};
    enqueue_chain(t, t->metric_chain, src, s);
    hipLaunchKernelGGL(k_metric_finish, dim3(1), dim3(64), 0, s, t->metric_chain, Q, out);
}

}  // namespace rl
