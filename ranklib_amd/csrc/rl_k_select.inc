// rl_k_select.inc -- select_step: the best-first growth bookkeeping of RegressionTree.fit with speculative slots, run by the last block of the finish
// (or by k_select).  queue_insert_lds, node_chunks, prepare_children, balance_slots, can_split, stalled_nodes, select_step_t, select_step.
// Included by rl_kernels_round.inc; needs that file's i128 helpers and trace block (strict_clock), rl_k_hist.inc (chunk_docs) and
// rl_k_best.inc (half_wave_best_feature, FeatBest, RL_CLK).

namespace rl {

__device__ __forceinline__ void queue_insert_lds(int *q, double *qd, int &qsize, int node, double d)
{   // RegressionTree.insert (:147-157): before the first element whose deviance is <= the new one's
    int i = 0;
    while (i < qsize) { if (qd[i] > d) i++; else break; }
    for (int j = qsize; j > i; j--) { q[j] = q[j - 1]; qd[j] = qd[j - 1]; }
    q[i] = node; qd[i] = d;
    qsize++;
}

// histogram chunks of a node of cnt samples (as k_hist cuts it)
__device__ __forceinline__ int node_chunks(const Ctx &c, int cnt) { return cnt <= 0 ? 0 : (cnt + chunk_docs<false>(c, cnt) - 1) / chunk_docs<false>(c, cnt); }

// Put node p into slot `sl` of the next growth step: its children l, l+1 get node records (global counts / exact
// totals from p's cumulative histogram); their local sample ranges are set by the partition kernel.
// tile0 / chunk0 are filled by the caller (prefix over the slots).
__device__ __forceinline__ void prepare_children(const Ctx &c, NodeRec *N, int p, int l, SlotRec &sl)
{
    NodeRec &P = N[p];
    const int r = l + 1;
    const int cl = P.best_cl;                                    // cumulative histogram entry at the split
    const long long thi = P.best_hi; const unsigned long long tlo = P.best_lo;
    NodeRec Lc, Rc;
    Lc.start = P.start; Lc.count = 0; Lc.gcount = cl; Lc.buf = 1 - P.buf; Lc.parent = p; Lc.left = Lc.right = -1;
    Rc.start = P.start; Rc.count = 0; Rc.gcount = P.gcount - cl; Rc.buf = 1 - P.buf; Rc.parent = p; Rc.left = Rc.right = -1;
    const i128 tl = make_i128(thi, tlo);                        // exact: same sample set as the left child
    const i128 tr = make_i128(P.tot_hi, P.tot_lo) - tl;
    Lc.tot_hi = hi_of(tl); Lc.tot_lo = lo_of(tl);
    Rc.tot_hi = hi_of(tr); Rc.tot_lo = lo_of(tr);
    Lc.best_f = Lc.best_t = Rc.best_f = Rc.best_t = -1; Lc.best_S = Rc.best_S = -1.0;
    Lc.best_cl = Rc.best_cl = 0; Lc.best_hi = Rc.best_hi = 0; Lc.best_lo = Rc.best_lo = 0;
    Lc.deviance = Rc.deviance = 0.0; Lc.sum_response = Rc.sum_response = 0.0; Lc.sq_response = Rc.sq_response = 0.0;
    Lc.sq = Rc.sq = 0;
    Lc.output = Rc.output = 0.f;
    Lc.pl = Lc.pr = Rc.pl = Rc.pr = -1; Lc.fid = Rc.fid = -1; Lc.prepared = Rc.prepared = 0;
    Lc.tie = Rc.tie = 0; Lc.ph = child_hash(P.ph, 0); Rc.ph = child_hash(P.ph, 1);
    N[l] = Lc; N[r] = Rc;
    P.pl = l; P.pr = r; P.prepared = 1;
    sl.node = p; sl.left = l; sl.right = r;
    sl.build_left = (cl <= P.gcount - cl) ? 1 : 0;
    sl.pstart = P.start; sl.pcount = P.count; sl.pbuf = P.buf; sl.f = P.best_f; sl.t = P.best_t;
    sl.tile0 = 0; sl.ntiles = (P.count + kPartTile - 1) / kPartTile;
    // chunks of the child that is accumulated: exact on one GPU; an upper bound of the LOCAL part when sharded
    sl.chunk0 = 0; sl.cs = 0; sl.skip_hist = 0;
    if (!c.sharded) { sl.nchunks = node_chunks(c, sl.build_left ? cl : P.gcount - cl); sl.nleft = cl; }
    else if (c.cum_cnt_loc) {       // sharded, round 6: this rank's share of the left child from its own cumulative counts (k_hist_reduce keeps them beside the all-reduced ones)
        const int nl = c.cum_cnt_loc[((size_t)p * c.F + P.best_f) * c.TS + P.best_t];
        sl.nleft = nl; sl.nchunks = node_chunks(c, sl.build_left ? nl : P.count - nl);
        N[l].count = nl; N[r].start = P.start + nl; N[r].count = P.count - nl;
    } else { sl.nchunks = (P.count == 0) ? 0 : max(64, P.count / c.node_chunk + 1) + 1; sl.nleft = -1; }
    sl.sq_left = 0;
    atomicAdd(&c.grow_docs[0], (unsigned long long)(sl.build_left ? cl : P.gcount - cl));
    atomicAdd(&c.grow_docs[1], (unsigned long long)P.gcount);
}

// Balanced chunks for a step that fills the chip (one GPU: the built children's sizes are known).  chunk_docs gives a large node the largest
// chunk, and the first steps of a c2 tree came to 810 / 1 692 / 1 233 (chunk, group) blocks for the 768 places of the chip (three 50 KB blocks per
// CU): CUs ended up with 3 to 5 (5 to 8) blocks and the launch lasted until the fullest CU was done (HISTORY.md 10.5, profiles/r04_block_placement_*).
// Here the step's documents are cut into k x balance_target chunks of ONE size (<= 2^14 documents: what an int64 accumulator holds), the same
// size for every node of the step, and launch_hist launches exactly balance_target rows of blocks, so every block row works through k chunks.
// balance_target = 56: 56 rows x 9 feature groups = 504 blocks = TWO per CU, which is what saturates a CU's LDS atomic unit; a third block on
// some CUs (80 rows) makes those CUs 1.5 x as slow as the others (measured: 80 rows +1 %, 56 rows +3 %, 64 / 72 rows worse than none).
// Steps of at most balance_min chunks keep the per-node rule (finer cuts only add partial histograms to flush and to reduce).  One thread calls
// this, after prepare_children, before the prefix over the slots.  Exact integer sums: the cut changes no result.
__device__ __forceinline__ void balance_slots(const Ctx &c, SlotRec *slot, int ns)
{
    if ((c.sharded && !c.cum_cnt_loc) || !c.balance) return;       // (local sizes unknown: chunk_docs' rule.  Until round 6 a ONE-rank communicator was balanced while k_hist_reduce
                                                                    // cut its nodes by chunk_docs' rule: runs of more than 28 chunks a step summed the wrong partials, tools/dist_scale_check.py)
    int legacy = 0; unsigned D = 0;       // (the built children of a step are disjoint: D <= N < 2^31 -- 32-bit divisions; a 64-bit one is ~100 instructions of the step's serial tail)
    int cnt[kSpec];
    for (int j = 0; j < ns && j < kSpec; j++) {
        cnt[j] = slot[j].build_left ? slot[j].nleft : slot[j].pcount - slot[j].nleft;
        legacy += slot[j].nchunks; D += (unsigned)cnt[j];
    }
    const int T = c.balance_target, cap = c.balance_cap;
    if (legacy <= c.balance_min) return;
    const unsigned tcap = (unsigned)T * (unsigned)cap;
    const int k = (int)(D / tcap + (D % tcap != 0u ? 1u : 0u));
    const int target = k * T;
    int cs = (int)((D / (unsigned)target + (D % (unsigned)target != 0u ? 1u : 0u) + 255u) & ~255u);
    for (;;) {
        if (cs > cap) cs = cap;
        int tot = 0;
        for (int j = 0; j < ns && j < kSpec; j++) tot += (cnt[j] + cs - 1) / cs;
        if (tot <= target || cs >= cap) break;
        cs += 256;
    }
    int tot = 0;
    for (int j = 0; j < ns && j < kSpec; j++) tot += (cnt[j] + cs - 1) / cs;
    if (tot > c.maxChunks) return;   // (the partial-histogram buffers hold maxChunks rows)
    for (int j = 0; j < ns && j < kSpec; j++) { slot[j].cs = cs; slot[j].nchunks = (cnt[j] + cs - 1) / cs; }
}

__device__ __forceinline__ double variance_of(double sq, double sum, int n) { return sq - sum * sum / n; }  // :348-350

__device__ __forceinline__ void copy_words(void *dst, const void *src, int nwords8)
{
    for (int i = threadIdx.x; i < nwords8; i += blockDim.x) ((unsigned long long *)dst)[i] = ((const unsigned long long *)src)[i];
}

__device__ __forceinline__ bool can_split(const Ctx &c, const NodeRec &X)
{   // RegressionTree.fit :74-77 (too few samples) and FeatureHistogram.findBestSplit :267-269, :311-313
    if (X.gcount < 2 * c.mls) return false;
    const bool zero_dev = (X.deviance >= 0.0 && X.deviance <= 0.0);
    return !(zero_dev || X.best_S == -1.0);
}

// lazy tie-break (rl_tie.inc): of the nodes about to be partitioned, those whose exactly tied best split the Java's rounding noise decides
// and that have not been resolved yet -- several features tie (2), or only thresholds of one feature do (1) but the node is a RIGHT child,
// whose Java histogram is parent - left (FeatureHistogram.java:222-234) instead of a sum of its own samples.  One thread calls this.
// A tie of kind 1 in a right child does NOT stall: every tied threshold cuts off the same documents, so the node is partitioned at once and only
// its stored threshold is re-decided, together with the tree's other such nodes, before the tree is exported (NodeRec::tie bit 0x40, `deferred`).
__device__ __forceinline__ int stalled_nodes(NodeRec *N, const int *sel, int nsel, int32_t *out, int *deferred, bool xdefer)
{
    int n = 0;
    for (int i = 0; i < nsel; i++) {
        NodeRec &X = N[sel[i]];
        if ((X.tie & 0xc0) || (X.tie & 3) == 0) continue;
        const bool right = X.parent >= 0 && N[X.parent].pr == sel[i];
        if ((X.tie & 3) == 2) {
            if (xdefer && (X.tie & 4)) { X.tie |= 0x40; *deferred = 1; }       // several features, one cut: partition now, name the feature later
            else out[n++] = sel[i];
        } else if (right) { X.tie |= 0x40; *deferred = 1; }
    }
    return n;
}

// bytes of dynamic LDS select_step needs
__host__ __device__ inline size_t select_lds_bytes(int L, int NC, bool nodes_in_lds, int F = 0, bool sampling = false)
{
    return sizeof(TreeState) + (nodes_in_lds ? (size_t)NC * sizeof(NodeRec) : 0) + (size_t)(L + 2) * 12 + (size_t)kSpec * 2 * 16 + 64 +
           (sampling ? (size_t)2 * kSpec * F * 8 + 8 : 0);
}

// Called by every thread of ONE block (the last one of k_hist_finish).  smem: TreeState | NodeRec[NC] (only if it
// fits, else the records are used in place) | qd[L+2] | bS[2 kSpec] | q[L+2] | bf, bt[2 kSpec] | sel[kSpec]
// NL (node records in LDS) is a template parameter: with a run-time choice between the LDS copy and c.nodes every access to a record was a FLAT
// load / store followed by a wait on both counters -- the fit loop's chain of dependent record reads ran at global-memory latency.
template <bool NL, bool WIDE = false>
__device__ __forceinline__ void select_step_t(const Ctx &c, bool is_root, unsigned char *smem, bool dist)
{
    constexpr bool nodes_in_lds = NL;
    static_assert(sizeof(TreeState) % 16 == 0 && sizeof(NodeRec) % 8 == 0, "copied as 8-byte words");
    TreeState &st = *(TreeState *)smem;
    unsigned char *ptr = smem + sizeof(TreeState);
    NodeRec *N = c.nodes;
    if (nodes_in_lds) { N = (NodeRec *)ptr; ptr += (size_t)c.NC * sizeof(NodeRec); }
    const int QC = c.L + 2;              // queue capacity
    double *qd = (double *)ptr; ptr += (size_t)QC * 8;
    double *bS = (double *)ptr; ptr += 2 * kSpec * 8;
    int *q = (int *)ptr; ptr += (size_t)QC * 4;
    int *bf = (int *)ptr; ptr += 2 * kSpec * 4;
    int *bt = (int *)ptr; ptr += 2 * kSpec * 4;
    int *sel = (int *)ptr; ptr += kSpec * 4;
    unsigned long long *fkeys = (unsigned long long *)(((size_t)ptr + 7) & ~(size_t)7);      // [2 kSpec][F], only with feature sampling
    __shared__ int bcl[2 * kSpec], btie[2 * kSpec]; __shared__ long long bhi[2 * kSpec]; __shared__ unsigned long long blo[2 * kSpec];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6, nwaves = blockDim.x >> 6;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");          // see ld_agent
#ifdef RL_PHASE_CLOCKS
    { const long long t_ = strict_clock(); if (!is_root && threadIdx.x == 0) c.clk[(c.st->step & 63) * 32 + 14] = t_; }      // select entry
#endif
    copy_words(&st, c.st, sizeof(TreeState) / 8);
    __syncthreads();
    const int E = st.E, E2 = st.E2;

    if (is_root) {
        if (wave == 0) {
            double S0; int f0, t0, cl0, tie0; long long hi0; unsigned long long lo0;
            const unsigned long long h0 = root_hash(c.seed, st.tree_seq);       // tree_seq = trees started before this one
            half_wave_best_feature(c, lane < 32, 0, 0, h0, fkeys, S0, f0, t0, cl0, hi0, lo0, tie0,
                                   (long long)ld_agent((const unsigned long long *)&c.fb_root[0]), ld_agent((const unsigned long long *)&c.fb_root[1]), c.cum_cnt[(size_t)c.nthr[0] - 1]);
            if (lane == 0) {
                NodeRec R;
                R.start = 0; R.count = c.N; R.buf = 0; R.parent = -1; R.left = R.right = -1;
                R.gcount = c.cum_cnt[(size_t)c.nthr[0] - 1];            // global N (static counts; feature 0, last bin)
                R.tot_hi = (long long)ld_agent((const unsigned long long *)&c.fb_root[0]); R.tot_lo = ld_agent((const unsigned long long *)&c.fb_root[1]);
                // sharded: the all-reduced sum (st.root_sq stays this rank's own: a tree that is grown a second time reduces it again)
                R.sq = c.sharded ? c.dist_buf[(size_t)c.F * c.TS * c.limb_words] : st.root_sq;
                R.sum_response = fixed_to_double(make_i128(R.tot_hi, R.tot_lo), E);
                R.sq_response = fixed_to_double((i128)R.sq, E2);
                if (c.java) { R.sum_response = c.jtot[0]; R.sq_response = c.jtot[1]; }      // sequential sums over k = 0 .. N-1 (:133-137)
                R.deviance = 3.4028234663852886e38;           // Float.MAX_VALUE  (RegressionTree.java:60)
                R.best_S = S0; R.best_f = f0; R.best_t = t0; R.output = 0.f;
                R.best_cl = cl0; R.best_hi = hi0; R.best_lo = lo0;
                R.pl = R.pr = -1; R.fid = 0; R.prepared = 0; R.tie = c.fs_on ? 0 : tie0; R.ph = h0;
                st.n_nodes = 1; st.qsize = 0; st.taken = 0; st.done = 0; st.nslots = 0; st.n_splits = 0; st.stall_n = 0; st.defer_any = 0;
                st.step = 0; st.tree_seq++;
                st.tiles_total = 0; st.chunks_total = 0; st.arrive = 0; st.epoch++;
                for (int j = 0; j < kSpec * 16; j++) (&st.arrive1[0][0])[j] = 0;
                N[0] = R;
                if (S0 == -1.0) st.done = 1;                  // root cannot split: single-leaf tree (:64-67,86)
                else if (c.tie_on && (R.tie & 3) == 2 && !((c.tie_on & 2) && (R.tie & 4))) { st.stall_n = 1; st.stall_node[0] = 0; }      // several features tie at the root: the Java's noise decides (rl_tie.inc)
                else {
                    if (c.tie_on && (R.tie & 3) == 2) { N[0].tie |= 0x40; st.defer_any = 1; }      // ... over one and the same cut: deferred
                    prepare_children(c, N, 0, 1, st.slot[0]);
                    balance_slots(c, st.slot, 1);
                    st.n_nodes = 3; st.nslots = 1; st.tiles_total = st.slot[0].ntiles; st.chunks_total = st.slot[0].nchunks;
                    c.grow_stats[0]++; c.grow_stats[1]++;
                }
                c.grow_stats[3]++;
            }
        }
        __syncthreads();
        if (nodes_in_lds) copy_words(c.nodes, N, st.n_nodes * (int)(sizeof(NodeRec) / 8));
        copy_words(c.st, &st, sizeof(TreeState) / 8);
        if (tid == 0 && c.progress)
            __hip_atomic_store(c.progress, ((unsigned long long)(unsigned)st.tree_seq << 32) | (st.stall_n > 0 ? (1ull << 31) : 0ull) | (st.defer_any ? (1ull << 30) : 0ull) | (st.done ? 1ull : 0ull),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }

    RL_CLK(true, 8);
    // A. best split per (slot, side) by one wavefront each; LDS copies of the node records and the queue
    const int ns = st.nslots, qs0 = st.qsize, nn0 = st.n_nodes;
    long long sq_left_v = 0;        // unsharded: sum of lambda^2 over the left child, reduced from the partition's per-tile partials by block (0, slot)
    if (!dist && tid < ns) sq_left_v = (long long)ld_agent(&c.fb_sq[tid]);
    // the node records and the queue are fetched first: their loads are in flight while the per-feature records are reduced
    constexpr int kPre = 8;
    const int nw8 = nodes_in_lds ? nn0 * (int)(sizeof(NodeRec) / 8) : 0;
    unsigned long long pre[kPre];
#pragma unroll
    for (int u = 0; u < kPre; u++) { const int i = tid + u * (int)blockDim.x; pre[u] = i < nw8 ? ((const unsigned long long *)c.nodes)[i] : 0ull; }
    const int q_pre = tid < qs0 ? c.queue[tid] : 0;
#ifdef RL_PHASE_CLOCKS
    if (tid == 0) c.clk[(c.st->step & 63) * 32 + 16] = (long long)wall_clock64();      // (no wait: the loads above stay in flight)
#endif
    for (int p0 = 2 * wave; p0 < 2 * ns; p0 += 2 * nwaves) {
        const int pi = p0 + (lane >> 5);
        double S; int f, t, cl, tie; long long hi; unsigned long long lo;
        unsigned long long h = 0;
        if (c.fs_on && pi < 2 * ns) h = c.nodes[(pi & 1) ? st.slot[pi >> 1].right : st.slot[pi >> 1].left].ph;
        long long nthi = 0; unsigned long long ntlo = 0; int nctot = 0;
        if (c.tie_on && pi < 2 * ns) { const NodeRec &Ch = c.nodes[(pi & 1) ? st.slot[pi >> 1].right : st.slot[pi >> 1].left]; nthi = Ch.tot_hi; ntlo = Ch.tot_lo; nctot = Ch.gcount; }
        half_wave_best_feature<WIDE>(c, pi < 2 * ns, pi >> 1, pi & 1, h, fkeys + (size_t)min(pi, 2 * kSpec - 1) * c.F, S, f, t, cl, hi, lo, tie, nthi, ntlo, nctot);
        if ((lane & 31) == 0 && pi < 2 * ns) { bS[pi] = S; bf[pi] = f; bt[pi] = t; bcl[pi] = cl; bhi[pi] = hi; blo[pi] = lo; btie[pi] = c.fs_on ? 0 : tie; }
    }
    RL_CLK(true, 15);
#pragma unroll
    for (int u = 0; u < kPre; u++) { const int i = tid + u * (int)blockDim.x; if (i < nw8) ((unsigned long long *)N)[i] = pre[u]; }
    for (int i = tid + kPre * (int)blockDim.x; i < nw8; i += blockDim.x) ((unsigned long long *)N)[i] = ((const unsigned long long *)c.nodes)[i];
    if (tid < qs0) q[tid] = q_pre;
    for (int i = tid + (int)blockDim.x; i < qs0; i += blockDim.x) q[i] = c.queue[i];
    __syncthreads();
    RL_CLK(true, 9);
    // B. complete the children of the nodes prepared by the step that just ran (one thread per slot)
    if (!dist) { if (tid < ns) st.slot[tid].sq_left = sq_left_v; }
    else if (tid < ns) st.slot[tid].sq_left = c.dist_buf[(size_t)tid * ((size_t)c.F * c.TS * c.limb_words + 4) + (size_t)c.F * c.TS * c.limb_words];     // all-reduced
    __syncthreads();
    if (tid < ns) {
        const SlotRec &sl = st.slot[tid];
        NodeRec &P = N[sl.node]; NodeRec &Lc = N[sl.left]; NodeRec &Rc = N[sl.right];
        if (sl.build_left) { Lc.sq = sl.sq_left; Rc.sq = P.sq - Lc.sq; }       // sq_left: the BUILT child's sum (k_part_scatter)
        else { Rc.sq = sl.sq_left; Lc.sq = P.sq - Rc.sq; }
        Lc.sum_response = fixed_to_double(make_i128(Lc.tot_hi, Lc.tot_lo), E);
        Rc.sum_response = fixed_to_double(make_i128(Rc.tot_hi, Rc.tot_lo), E);
        Lc.sq_response = fixed_to_double((i128)Lc.sq, E2);
        Rc.sq_response = fixed_to_double((i128)Rc.sq, E2);
        if (c.java) {       // left: sequential sums over its samples (:182-186); right: parent - left (:202-203)
            Lc.sum_response = c.jtot[2 * tid]; Lc.sq_response = c.jtot[2 * tid + 1];
            Rc.sum_response = P.sum_response - Lc.sum_response; Rc.sq_response = P.sq_response - Lc.sq_response;
        }
        Lc.deviance = variance_of(Lc.sq_response, Lc.sum_response, Lc.gcount);
        Rc.deviance = variance_of(Rc.sq_response, Rc.sum_response, Rc.gcount);
        Lc.best_S = bS[2 * tid]; Lc.best_f = bf[2 * tid]; Lc.best_t = bt[2 * tid];
        Lc.best_cl = bcl[2 * tid]; Lc.best_hi = bhi[2 * tid]; Lc.best_lo = blo[2 * tid];
        Rc.best_S = bS[2 * tid + 1]; Rc.best_f = bf[2 * tid + 1]; Rc.best_t = bt[2 * tid + 1];
        Rc.best_cl = bcl[2 * tid + 1]; Rc.best_hi = bhi[2 * tid + 1]; Rc.best_lo = blo[2 * tid + 1];
        Lc.tie = btie[2 * tid]; Rc.tie = btie[2 * tid + 1];
    }
    __syncthreads();
    RL_CLK(true, 10);
    // C. RegressionTree.fit's loop (:70-85), as far as prepared nodes allow, then the choice of the next slots.
    if (QC <= 64) {
        // Wavefront version: lane p holds queue entry p (node, deviance, can-split, prepared) in registers;
        // insert = ballot + shift, pop = shift.  (A single lane walking LDS pays ~50 ns per dependent access.)
        if (wave == 0) {
            int qn = (lane < qs0) ? q[lane] : -1;
            double qdv = 0.0; bool cs = false, prep = false;
            if (qn >= 0) { const NodeRec &X = N[qn]; qdv = X.deviance; cs = can_split(c, X); prep = X.prepared != 0; }
            int qsize = qs0, taken = st.taken, n_splits = st.n_splits, ncommit = 0;
            const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
            auto insert = [&](int node, double d, bool ncs) {          // RegressionTree.insert (:147-157)
                const int pos = __builtin_popcountll(__ballot(lane < qsize && qdv > d));
                const int un = __shfl_up(qn, 1); const double ud = __shfl_up(qdv, 1);
                const int uc = __shfl_up((int)cs, 1), up = __shfl_up((int)prep, 1);
                if (lane > pos) { qn = un; qdv = ud; cs = uc != 0; prep = up != 0; }
                else if (lane == pos) { qn = node; qdv = d; cs = ncs; prep = false; }
                qsize++;
            };
            auto pop = [&]() {
                qn = __shfl_down(qn, 1); qdv = __shfl_down(qdv, 1);
                cs = __shfl_down((int)cs, 1) != 0; prep = __shfl_down((int)prep, 1) != 0;
                qsize--;
            };
            // a split becomes part of the tree: sp.set(.., var) (:352), children enter the queue (:66-67, :82-83)
            auto commit = [&](int p) {
                NodeRec &X = N[p];
                const int l = X.pl, r = X.pr;
                const int child = (lane == 0) ? l : r;
                double dch = 0.0; int cch = 0;
                if (lane < 2) { dch = N[child].deviance; cch = can_split(c, N[child]) ? 1 : 0; }
                const double dl = __shfl(dch, 0), dr = __shfl(dch, 1);
                const int csl = __shfl(cch, 0), csr = __shfl(cch, 1);
                if (lane == 0) {
                    X.left = l; X.right = r;
                    X.deviance = variance_of(X.sq_response, X.sum_response, X.gcount);
                    N[l].fid = 2 * n_splits + 1; N[r].fid = 2 * n_splits + 2;
                    c.grow_docs[2] += (unsigned long long)N[l].gcount; c.grow_docs[3] += (unsigned long long)X.gcount;
                    if (c.steplog && X.tie) {       // debug: committed splits whose best candidate was tied, and the Java-order derivation chain they hang on
                        const int e = atomicAdd(&c.steplog[0], 1);
                        if (e < kStepLogCap) {
                            int *o = c.steplog + 8 + 8 * e;
                            int cur = p, nchain = 1, mx = X.gcount; long long tot = X.gcount;
                            const bool is_right = X.parent >= 0 && N[X.parent].pr == p;
                            while (N[cur].parent >= 0 && N[N[cur].parent].pr == cur) {       // a right child: parent - left sibling
                                const int par = N[cur].parent, sib = N[par].pl;
                                mx = max(mx, N[sib].gcount); tot += N[sib].gcount; nchain++;
                                cur = par;
                            }
                            if (cur != p) { mx = max(mx, N[cur].gcount); tot += N[cur].gcount; nchain++; }
                            o[0] = st.tree_seq; o[1] = 1; o[2] = X.tie & 255; o[3] = (is_right ? 1 : 0) | ((X.tie >> 8) << 1); o[4] = X.gcount; o[5] = mx; o[6] = nchain; o[7] = (int)min(tot, (long long)0x7fffffff);
                        }
                    }
                }
                n_splits++; ncommit++;
                insert(l, dl, csl != 0);
                insert(r, dr, csr != 0);
            };
            if (ns == 1 && st.slot[0].node == 0) commit(0);              // the root is split unconditionally (:62-67)
            bool done = true;
            while (taken + qsize < c.L && qsize > 0) {
                const int leaf = __shfl(qn, 0);
                const bool cs0 = __shfl((int)cs, 0) != 0, prep0 = __shfl((int)prep, 0) != 0;
                if (!cs0) { pop(); taken++; continue; }
                if (prep0) { pop(); commit(leaf); continue; }
                done = false;
                break;
            }
            // next step: the first kSpec unprepared nodes in queue order that the leaf budget can still reach
            int nsel = 0, err = 0;
            if (!done) {
                const int budget = c.L - (taken + qsize);                         // splits left (>= 1)
                const bool inq = lane < qsize;
                const int ahead = __builtin_popcountll(__ballot(inq && cs) & below);          // splittable nodes before p
                const bool cand = inq && cs && !prep && ahead < budget;
                const unsigned long long cmask = __ballot(cand);
                const int rank = __builtin_popcountll(cmask & below);
                nsel = min(__builtin_popcountll(cmask), kSpec);
                while (nsel > 0 && nn0 + 2 * nsel > c.NC) nsel--;
                if (cand && rank < nsel) sel[rank] = qn;
                if (nsel == 0) { done = true; err = 1; }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            int nstall = 0;
            if (c.tie_on && lane == 0) nstall = stalled_nodes(N, sel, nsel, st.stall_node, &st.defer_any, (c.tie_on & 2) != 0);
            nstall = __shfl(nstall, 0);
            if (nstall > 0) nsel = 0;                 // nothing is partitioned until the host has resolved the ties (rl_tie.inc)
            if (lane == 0) st.stall_n = nstall;
            if (lane < qsize) c.queue[lane] = qn;
            if (lane == 0) {
                st.done = done ? 1 : 0; if (err && !st.error) st.error = 1;
                st.nslots = nsel; st.qsize = qsize; st.taken = taken; st.n_splits = n_splits;
                c.grow_stats[2] += ncommit;
                if (nsel > 0) { c.grow_stats[0]++; c.grow_stats[1] += nsel; }
            }
        }
    } else {
        for (int i = tid; i < qs0; i += blockDim.x) qd[i] = N[q[i]].deviance;
        __syncthreads();
        if (tid == 0) {       // serial version for very wide trees
            int head = 0, qsize = qs0, ncommit = 0;
            auto commit = [&](int p) {
                NodeRec &X = N[p];
                X.left = X.pl; X.right = X.pr;
                X.deviance = variance_of(X.sq_response, X.sum_response, X.gcount);
                N[X.left].fid = 2 * st.n_splits + 1; N[X.right].fid = 2 * st.n_splits + 2;
                c.grow_docs[2] += (unsigned long long)N[X.left].gcount; c.grow_docs[3] += (unsigned long long)X.gcount;
                st.n_splits++;
                ncommit++;
                int n = qsize - head;
                queue_insert_lds(q + head, qd + head, n, X.left, N[X.left].deviance);
                queue_insert_lds(q + head, qd + head, n, X.right, N[X.right].deviance);
                qsize = head + n;
            };
            if (ns == 1 && st.slot[0].node == 0) commit(0);
            bool done = true;
            while ((c.L == -1 || st.taken + (qsize - head) < c.L) && (qsize - head) > 0) {
                const int leaf = q[head];
                const NodeRec &X = N[leaf];
                if (!can_split(c, X)) { head++; st.taken++; continue; }
                if (X.prepared) { head++; commit(leaf); continue; }
                done = false;
                break;
            }
            st.done = done ? 1 : 0;
            int nsel = 0;
            if (!done) {
                const int budget = (c.L == -1) ? 0x7fffffff : c.L - (st.taken + (qsize - head));
                int ahead = 0;
                for (int p = head; p < qsize && nsel < kSpec && ahead < budget; p++) {
                    const NodeRec &X = N[q[p]];
                    if (!can_split(c, X)) continue;
                    ahead++;
                    if (X.prepared) continue;
                    if (nn0 + 2 * (nsel + 1) > c.NC) { if (nsel == 0) st.error = 1; break; }
                    sel[nsel++] = q[p];
                }
                if (nsel == 0) { st.done = 1; if (!st.error) st.error = 2; }
            }
            st.stall_n = c.tie_on ? stalled_nodes(N, sel, nsel, st.stall_node, &st.defer_any, (c.tie_on & 2) != 0) : 0;
            if (st.stall_n > 0) nsel = 0;
            st.nslots = nsel;
            st.qsize = qsize - head;
            for (int i = 0; i < st.qsize; i++) c.queue[i] = q[head + i];
            c.grow_stats[2] += ncommit;
            if (nsel > 0) { c.grow_stats[0]++; c.grow_stats[1] += nsel; }
        }
    }
    __syncthreads();
    RL_CLK(true, 11);
    // D. children records of the selected nodes (one thread per slot: the histogram reads are independent)
    const int nsel = st.nslots;
    if (tid < nsel) prepare_children(c, N, sel[tid], nn0 + 2 * tid, st.slot[tid]);
    if (c.steplog && tid < nsel) {        // debug: what every growth step works on
        const int e = atomicAdd(&c.steplog[0], 1);
        if (e < kStepLogCap) {
            int *o = c.steplog + 8 + 8 * e; const NodeRec &P = N[sel[tid]];
            o[0] = st.tree_seq; o[1] = 0; o[2] = st.step + 1; o[3] = tid; o[4] = P.gcount; o[5] = st.slot[tid].build_left ? P.best_cl : P.gcount - P.best_cl; o[6] = P.tie; o[7] = nsel;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int tiles = 0, chunks = 0;
        balance_slots(c, st.slot, nsel);
        for (int j = 0; j < nsel; j++) {
            st.slot[j].tile0 = tiles; tiles += st.slot[j].ntiles;
            st.slot[j].chunk0 = chunks; chunks += st.slot[j].nchunks;
        }
        st.tiles_total = tiles; st.chunks_total = chunks;
        st.n_nodes = nn0 + 2 * nsel;
        st.arrive = 0; st.epoch++;
        for (int j = 0; j < kSpec * 16; j++) (&st.arrive1[0][0])[j] = 0;
    }
    __syncthreads();
    RL_CLK(true, 12);
    if (nodes_in_lds) copy_words(c.nodes, N, st.n_nodes * (int)(sizeof(NodeRec) / 8));
    RL_CLK(true, 13);
#ifdef RL_PHASE_CLOCKS
    if (tid == 0 && st.tree_seq == c.trace_tree) c.clk[(st.step & 63) * 32 + 28] = (long long)wall_clock64();      // end of this step's bookkeeping
#endif
    if (tid == 0) st.step++;
    __syncthreads();
    copy_words(c.st, &st, sizeof(TreeState) / 8);
    // tell the host how far the tree is (relaxed system-scope store: no fence, nothing else is read through it)
    if (tid == 0 && c.progress)
        __hip_atomic_store(c.progress, ((unsigned long long)(unsigned)st.tree_seq << 32) | (st.stall_n > 0 ? (1ull << 31) : 0ull) | (st.defer_any ? (1ull << 30) : 0ull) |
                                           ((unsigned long long)((unsigned)st.step & 0x1fffffffu) << 1) | (st.done ? 1ull : 0ull),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <bool WIDE = false>
__device__ __forceinline__ void select_step(const Ctx &c, bool is_root, unsigned char *smem, bool nodes_in_lds, bool dist)
{
    if (nodes_in_lds) select_step_t<true, WIDE>(c, is_root, smem, dist);
    else select_step_t<false, WIDE>(c, is_root, smem, dist);
}

}  // namespace rl
