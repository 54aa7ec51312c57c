// rl_k_finish.inc -- K4/K5, the kernels: hist_finish_body (chunk reduction, prefix over thresholds, sibling = parent - built child, gain scan) and
// its three entry points k_hist_finish, k_hist_finish_wide and k_select.  Included by rl_kernels_round.inc; needs that file's i128 helpers and
// trace block (RL_TR_*), rl_k_hist.inc (chunk_docs), rl_k_reduce.inc, rl_k_best.inc and rl_k_select.inc.

namespace rl {

// SELECT: the last block to arrive runs select_step (one launch per growth step's finish).  !SELECT: the per-feature work only; the bookkeeping
// follows as a launch of its own (k_select) -- for wide data, see k_hist_finish_wide.
constexpr int kFinWideThreads = 192;     // three wavefronts: 10 blocks a CU at 8 wavefronts per SIMD (2 560 resident blocks)
template <bool ROOT, bool DIST, bool JAVA, bool SELECT>
__device__ __forceinline__ void hist_finish_body(const Ctx &c, int nodes_in_lds, unsigned long long *sh_raw)
{   // grid (F, slots)
    TreeState *st = c.st;
    RL_TR_BEGIN();
    constexpr int kNT = SELECT ? kFinThreads : kFinWideThreads;      // threads of the block (blockDim.x is a load from the dispatch packet)
    // B = the node whose histogram was accumulated from its samples, S = its sibling (= parent - B)
    int nodeB = 0, nodeS = -1, nodeP = -1, sideB = 0, ch0 = 0;
    const int slot = blockIdx.y;
    // everything the block needs from the step's tables is requested at once (the slot record is copied whole, valid or not: slot < kSpec), and the
    // feature's threshold count comes from a table parallel to `live`: each of these was a dependent memory round trip at the top of every block
    const int st_done = st->done, st_nslots = st->nslots, E = st->E;
#ifndef RL_FIN_BATCH
#define RL_FIN_BATCH 1
#endif
#if RL_FIN_BATCH
    SlotRec sl_c;
    if (!ROOT) sl_c = st->slot[slot];
#else
    const SlotRec &sl_c = st->slot[ROOT ? 0 : slot];
#endif
    const int f = (!DIST && c.live) ? c.live[blockIdx.x] : (int)blockIdx.x;
    const int TS = c.TS, T = (!DIST && c.live) ? c.live_nthr[blockIdx.x] : c.nthr[f];
    if (!ROOT) {
        if (st_done || slot >= st_nslots) return;
        const SlotRec &sl = sl_c;
        nodeP = sl.node; ch0 = sl.chunk0;
        if (sl.build_left) { nodeB = sl.left; nodeS = sl.right; sideB = 0; }
        else { nodeB = sl.right; nodeS = sl.left; sideB = 1; }
    }
    [[maybe_unused]] const bool clk0 = !ROOT && blockIdx.x == 0 && blockIdx.y == 0;
    RL_CLK(clk0, 0);
    RL_TR_MARK(1);
    long long *s_hi = (long long *)sh_raw;
    unsigned long long *s_lo = sh_raw + TS;
    int *s_cnt = (int *)(sh_raw + 2 * TS);
    [[maybe_unused]] double *s_j = (double *)((unsigned char *)sh_raw + (((size_t)TS * 20 + 7) & ~(size_t)7));   // JAVA: f64 cumulative sums of the left child / the root
    // the parent's cumulative entries, kept as the gain scan reads them: the tie check and the sibling's published record used to fetch theirs from memory again
    // (a dependent round trip each, at the end of every block)
    unsigned char *s_par = (unsigned char *)sh_raw + (((size_t)TS * 20 + 7) & ~(size_t)7) + (JAVA ? (size_t)TS * 8 : 0);
    [[maybe_unused]] long long *s_phi = (long long *)s_par;
    [[maybe_unused]] unsigned long long *s_plo = (unsigned long long *)(s_par + (size_t)TS * 8);
    [[maybe_unused]] int *s_pcn = (int *)(s_par + (size_t)TS * 16);
    const bool pcache = TS <= kParCacheTS;          // (threshold tables beyond that keep the old behaviour: twice the LDS would not fit a CU at -tc 4095)
    __shared__ Best sh_best[2 * (kFinThreads / 64)];
    __shared__ i128 sh_red[kFinThreads / 64];
    __shared__ int sh_redc[kFinThreads / 64];

    // block (0, slot) also folds the partition's per-tile lambda^2 partials of its slot (select_step used to do that in the serial tail)
    __shared__ long long sh_sqw[kFinThreads / 64];
    long long sqacc = 0;
    const bool sq_block = !ROOT && !DIST && blockIdx.x == 0;
    if (sq_block) {
        const SlotRec &sl = sl_c;
        // (eight per thread and trip, unconditional from a clamped index: one at a time the 1 841 tile partials of a 3.8 M-document parent were six serial round trips)
        constexpr int kSqBatch = 8;
        for (int i0 = (int)threadIdx.x; i0 < sl.ntiles; i0 += kSqBatch * kNT) {
            long long v[kSqBatch];
#pragma unroll
            for (int u = 0; u < kSqBatch; u++) v[u] = c.tile_sq[sl.tile0 + min(i0 + u * kNT, sl.ntiles - 1)];
#pragma unroll
            for (int u = 0; u < kSqBatch; u++) if (i0 + u * kNT < sl.ntiles) sqacc += v[u];
        }
    }
    int cntB_ = ROOT ? c.N : 0;
    if (!ROOT) {
        const SlotRec &slb = sl_c;
        cntB_ = (slb.nleft >= 0) ? (slb.build_left ? slb.nleft : slb.pcount - slb.nleft) : c.nodes[nodeB].count;      // one GPU: known from the slot
    }
    const int cntB = cntB_;
    const int csB = (!ROOT && sl_c.cs > 0) ? sl_c.cs : chunk_docs<ROOT>(c, cntB);      // (balance_slots)
    const int nch = (cntB + csB - 1) / csB;
    const size_t slotB = ((size_t)nodeB * c.F + f) * TS;
    // the parent's cumulative entry this thread needs in the gain scan: requested now, with the chunk partials, not after the prefix
    // (every gain-scan iteration of the thread: two with the 192-thread blocks of k_hist_finish_wide and 257 bins)
    constexpr int kPreIt = SELECT ? 1 : 2;
    long long pre_phi[kPreIt]; unsigned long long pre_plo[kPreIt]; int pre_pcnt[kPreIt];
#pragma unroll
    for (int u = 0; u < kPreIt; u++) {
        pre_phi[u] = 0; pre_plo[u] = 0; pre_pcnt[u] = 0;
        if (RL_FIN_BATCH && !ROOT) {
            const size_t o = ((size_t)nodeP * c.F + f) * TS + min((int)threadIdx.x + u * kNT, TS - 1);       // (clamped, unconditional)
            pre_phi[u] = c.cum_hi[o]; pre_plo[u] = c.cum_lo[o]; pre_pcnt[u] = c.cum_cnt[o];
        }
    }
    // ... the parent's totals (its last cumulative entry; the same address for every thread) ...
    long long tp_hi = 0; unsigned long long tp_lo = 0; int tp_cn = 0;
    if (!ROOT) { const size_t o = ((size_t)nodeP * c.F + f) * TS + (T - 1); tp_hi = c.cum_hi[o]; tp_lo = c.cum_lo[o]; tp_cn = c.cum_cnt[o]; }
    // ... and what the mode-bin rebuild needs: this thread's chunk total and the feature's mode bin
    long long pre_tot = 0; int pre_mode = 0;
    if (!DIST) { pre_tot = c.part_tot[ch0 + max(min((int)threadIdx.x, nch - 1), 0)]; pre_mode = c.mode[f]; }
    if (DIST) {     // totals were reduced over the chunks by k_hist_reduce and over the ranks by the all-reduce
        const int W = c.limb_words;
        const size_t slot_words = (size_t)c.F * TS * W + 4;
        const long long *in = c.dist_buf + slot * slot_words + (size_t)f * TS * W;
        for (int t = threadIdx.x; t < T; t += kNT) {
            long long hi, lo, cn;
            if (W == 3) { hi = in[3 * t]; lo = in[3 * t + 1]; cn = in[3 * t + 2]; }
            else { const long long w0 = in[2 * t]; cn = w0 & 0xffffffffll; hi = w0 >> 32; lo = in[2 * t + 1]; }   // the counts of all ranks sum to < 2^31
            const i128 acc = (((i128)hi) << kLimbShift) + (i128)lo;
            s_hi[t] = hi_of(acc); s_lo[t] = lo_of(acc); s_cnt[t] = (int)cn;
        }
    } else {
        const size_t cstride = (size_t)c.F * TS;
        for (int t = threadIdx.x; t < T; t += kNT) {
            i128 acc = 0;
            int cacc = 0;
            const long long *ps = c.part_sum + ((size_t)ch0 * c.F + f) * TS + t;
            const int *pc = c.part_cnt + ((size_t)ch0 * c.F + f) * TS + t;
            // Latency-bound: kFinBatch chunk partials are requested before the first is used (the 64-bit halves are summed separately so that no carry chain
            // ties a load to the previous one).  The loads are written as a batch of their own, unconditional, from a clamped chunk index: left to the scheduler
            // under k_hist_finish_wide's 64-register cap every load was completed before the next was issued (ten serial round trips for the five chunks of a
            // c3 node: 10 of the block's 22 us).
            constexpr int kFinBatch = ROOT ? 32 : (SELECT ? 16 : 8);        // (the root pass has hundreds of chunks and no counts to load)
            unsigned long long lo = 0; long long hi = 0;
            for (int ch = 0; ch < nch; ch += kFinBatch) {
                long long v[kFinBatch]; int cn[kFinBatch];
#pragma unroll
                for (int u = 0; u < kFinBatch; u++) {
                    const size_t o = (size_t)min(ch + u, nch - 1) * cstride;
                    v[u] = ps[o];
                    cn[u] = ROOT ? 0 : pc[o];
                }
#pragma unroll
                for (int u = 0; u < kFinBatch; u++)
                    if (ch + u < nch) { lo += (unsigned long long)(unsigned)v[u]; hi += (v[u] >> 32); cacc += cn[u]; }
            }
            acc += (i128)lo + (((i128)hi) << 32);
            s_hi[t] = hi_of(acc); s_lo[t] = lo_of(acc); s_cnt[t] = cacc;
        }
    }
    if (JAVA) for (int t = threadIdx.x; t < T; t += kNT) s_j[t] = c.jbin[((size_t)slot * c.F + f) * TS + t];
    if (sq_block) {
        for (int o = 32; o > 0; o >>= 1) sqacc += __shfl_xor(sqacc, o);
        if (lane_id() == 0) sh_sqw[threadIdx.x >> 6] = sqacc;
    }
    __syncthreads();
    if (sq_block && threadIdx.x == 0) { sqacc = 0; for (int w = 0; w < (kNT >> 6); w++) sqacc += sh_sqw[w]; }
    RL_CLK(clk0, 1);
    RL_TR_MARK(2);
    if (!DIST) rebuild_mode_bin(c, f, T, ch0, nch, cntB, !ROOT, s_hi, s_lo, s_cnt, sh_red, sh_redc, true, pre_tot, pre_mode);
    RL_CLK(clk0, 2);
    // prefix over t by wavefront 0: lane-local segment scan + wave scan of segment totals
    if (threadIdx.x < 64) {
        const int seg = (T + 63) / 64;
        const int b0 = min((int)threadIdx.x * seg, T), b1 = min(b0 + seg, T);
        i128 run = 0; int crun = 0;
        for (int t = b0; t < b1; t++) {
            run += make_i128(s_hi[t], s_lo[t]); crun += s_cnt[t];
            s_hi[t] = hi_of(run); s_lo[t] = lo_of(run); s_cnt[t] = crun;
        }
        i128 inc = run; int cinc = crun;
        for (int d = 1; d < 64; d <<= 1) {
            i128 u = shfl_up_i128(inc, d); int cu = __shfl_up(cinc, d);
            if ((int)threadIdx.x >= d) { inc += u; cinc += cu; }
        }
        const i128 off = inc - run; const int coff = cinc - crun;
        for (int t = b0; t < b1; t++) {
            const i128 v = make_i128(s_hi[t], s_lo[t]) + off;
            s_hi[t] = hi_of(v); s_lo[t] = lo_of(v); s_cnt[t] += coff;
        }
    } else if (JAVA && threadIdx.x == 64) {
        // sum[f][t] += sum[f][t-1] for t = 1 .. T-1, in that order (FeatureHistogram.java:141-145,189-194): one dependent chain
        double run = s_j[0];
        for (int t = 1; t < T; t++) { run = s_j[t] + run; s_j[t] = run; }
    }
    __syncthreads();

    RL_CLK(clk0, 3);
    RL_TR_MARK(3);
    const size_t slotP = ROOT ? 0 : ((size_t)nodeP * c.F + f) * TS;
    const size_t slotS = ROOT ? 0 : ((size_t)nodeS * c.F + f) * TS;
    // node totals = last cumulative bin (identical for every feature because the sums are exact)
    const i128 totB = make_i128(s_hi[T - 1], s_lo[T - 1]);
    i128 totS = 0;
    int ctotB, ctotS = 0;
    if (ROOT) {
        ctotB = c.cum_cnt[slotB + T - 1];
    } else {
        ctotB = s_cnt[T - 1];
        totS = make_i128(tp_hi, tp_lo) - totB;
        ctotS = tp_cn - ctotB;
    }
    double sumB = fixed_to_double(totB, E), sumS = fixed_to_double(totS, E);
    if (JAVA) {
        // node totals in the Java's order: the built (left) node's sumResponse is the sequential sum over its samples, the right
        // sibling's is parent - left (:202-203); B / S are whichever of the two the exact path accumulated / derived
        const double sumL = c.jtot[2 * slot];
        const double sumR = ROOT ? 0.0 : c.nodes[nodeP].sum_response - sumL;
        sumB = (sideB == 0) ? sumL : sumR; sumS = (sideB == 0) ? sumR : sumL;
    }
    Best bb = {-1.0, -1}, bs = {-1.0, -1};
    bool eqb = false, eqs = false;        // a later threshold of this thread reaches the thread's best S exactly
    bool eqbd = false, eqsd = false;      // ... with another left count (different sample sets: only possible beyond kFinThreads thresholds)
    int bbc = 0, bsc = 0;                 // left counts at the thread's best candidates
    for (int t = threadIdx.x; t < T; t += kNT) {
        const i128 vb = make_i128(s_hi[t], s_lo[t]);
        c.cum_hi[slotB + t] = s_hi[t]; c.cum_lo[slotB + t] = s_lo[t];
        int cb;
        if (ROOT) cb = c.cum_cnt[slotB + t];
        else { cb = s_cnt[t]; c.cum_cnt[slotB + t] = cb; }
        bool ok;
        double vbd, vsd = 0.0;
        if (JAVA) {
            const double jl_t = s_j[t];                                                  // left child (or root), cumulative
            const double jr_t = ROOT ? 0.0 : c.jcum[slotP + t] - jl_t;                   // FeatureHistogram.java:230
            vbd = (sideB == 0) ? jl_t : jr_t; vsd = (sideB == 0) ? jr_t : jl_t;
            c.jcum[slotB + t] = vbd;
            if (!ROOT) c.jcum[slotS + t] = vsd;
        } else vbd = fixed_to_double(vb, E);
        double S = gain_S(vbd, cb, sumB, ctotB, c.mls, ok);
        if (ok && S == bb.S) { eqb = true; eqbd |= (cb != bbc); }
        if (ok && S > bb.S) { bb.S = S; bb.t = t; bbc = cb; eqb = false; eqbd = false; }
        if (!ROOT) {
            const int it = (t - (int)threadIdx.x) / kNT;
            long long phi; unsigned long long plo; int pcn;
            if (RL_FIN_BATCH && it == 0) { phi = pre_phi[0]; plo = pre_plo[0]; pcn = pre_pcnt[0]; }
            else if (RL_FIN_BATCH && kPreIt > 1 && it == 1) { phi = pre_phi[kPreIt - 1]; plo = pre_plo[kPreIt - 1]; pcn = pre_pcnt[kPreIt - 1]; }
            else { phi = c.cum_hi[slotP + t]; plo = c.cum_lo[slotP + t]; pcn = c.cum_cnt[slotP + t]; }
            if (pcache) { s_phi[t] = phi; s_plo[t] = plo; s_pcn[t] = pcn; }
            const i128 vs = make_i128(phi, plo) - vb;      // FeatureHistogram.java:230-231
            const int cs2 = pcn - cb;
            c.cum_hi[slotS + t] = hi_of(vs); c.cum_lo[slotS + t] = lo_of(vs); c.cum_cnt[slotS + t] = cs2;
            if (!JAVA) vsd = fixed_to_double(vs, E);
            S = gain_S(vsd, cs2, sumS, ctotS, c.mls, ok);
            if (ok && S == bs.S) { eqs = true; eqsd |= (cs2 != bsc); }
            if (ok && S > bs.S) { bs.S = S; bs.t = t; bsc = cs2; eqs = false; eqsd = false; }
        }
    }
    RL_CLK(clk0, 4);
    RL_TR_MARK(4);
    const Best myb = bb, mys = bs;
    block_best2(bb, bs, sh_best, kNT >> 6);
    // exact ties inside the feature: some other threshold reaches the winner's S bit for bit (the same two sample sets: an empty-bin plateau).
    // The first one wins here as in the Java -- unless the Java's node histogram is a difference (a right child), see rl_tie.inc
    // (__syncthreads_or answers "any thread non-zero", not the bitwise OR of the arguments: one call per side)
    int tiebits = 0;
    if (!JAVA) {
        tiebits = __syncthreads_or((myb.t >= 0 && myb.S == bb.S && (myb.t != bb.t || eqb)) ? 1 : 0) ? 1 : 0;
        if (!ROOT) tiebits |= __syncthreads_or((mys.t >= 0 && mys.S == bs.S && (mys.t != bs.t || eqs)) ? 1 : 0) ? 2 : 0;
        // Do all tied thresholds cut off the SAME documents?  Thresholds of one feature are nested, so an equal left count means identical sets:
        // the partition is then known whatever the Java's noise picks and only the stored threshold has to wait for it (rl_tie.inc: deferred).
        if (tiebits & 1) {
            const int wc = ROOT ? c.cum_cnt[slotB + bb.t] : s_cnt[bb.t];
            if (__syncthreads_or((myb.t >= 0 && myb.S == bb.S && ((myb.t != bb.t && bbc != wc) || eqbd)) ? 1 : 0)) tiebits |= 4;
        }
        if (tiebits & 2) {
            const int wc = (pcache ? s_pcn[bs.t] : c.cum_cnt[slotP + bs.t]) - s_cnt[bs.t];
            if (__syncthreads_or((mys.t >= 0 && mys.S == bs.S && ((mys.t != bs.t && bsc != wc) || eqsd)) ? 1 : 0)) tiebits |= 8;
        }
    }
    RL_CLK(clk0, 5);
    RL_TR_MARK(5);

    // publish this feature's results, then count the block as arrived; the last block runs the growth bookkeeping
    __shared__ int sh_last;
    if (threadIdx.x == 0) {
        {
            const int t = max(bb.t, 0);
            publish_best(c, slot, sideB, f, bb.S, bb.t, ROOT ? c.cum_cnt[slotB + t] : s_cnt[t], s_hi[t], s_lo[t], (tiebits & 1) | ((tiebits >> 1) & 2));
        }
        if (!ROOT) {
            const int t = max(bs.t, 0);
            const i128 vs = (pcache ? make_i128(s_phi[t], s_plo[t]) : make_i128(c.cum_hi[slotP + t], c.cum_lo[slotP + t])) - make_i128(s_hi[t], s_lo[t]);
            publish_best(c, slot, 1 - sideB, f, bs.S, bs.t, (pcache ? s_pcn[t] : c.cum_cnt[slotP + t]) - s_cnt[t], hi_of(vs), lo_of(vs), ((tiebits >> 1) & 1) | ((tiebits >> 2) & 2));
        }
        if (sq_block) st_agent(&c.fb_sq[slot], (unsigned long long)sqacc);
        if (ROOT && blockIdx.x == 0) { st_agent((unsigned long long *)&c.fb_root[0], (unsigned long long)hi_of(totB)); st_agent((unsigned long long *)&c.fb_root[1], lo_of(totB)); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        RL_CLK(clk0, 6);
        if (!ROOT) RL_TR_END(2, blockIdx.y * gridDim.x + blockIdx.x);
        if (!SELECT) return;
        // two-level arrival: hundreds of blocks on ONE counter serialise in L2 (the last block saw ~11 us of it); <= 16 groups
        // of features per slot count first, the last block of a group counts on the top-level word
        const int F = (int)gridDim.x, gs = (F + 15) / 16, grp = (int)blockIdx.x / gs, ngrp = (F + gs - 1) / gs;
        const int in_grp = min(gs, F - grp * gs);
        sh_last = 0;
        // (release on arrival, acquire for the block that arrives last: ADVICE r04 -- the relaxed form rested on every producer store being a write-through
        // st_agent and on the consumer's one acquire fence; the fused kernel is the fall-back path since round 5 / 6, the ordering costs it nothing measurable)
        if (__hip_atomic_fetch_add(&st->arrive1[slot][grp], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1) {
            const int target = ROOT ? ngrp : ngrp * st_nslots;
            sh_last = (__hip_atomic_fetch_add(&st->arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == target - 1) ? 1 : 0;
        }
    }
    RL_CLK(clk0, 7);
    if (!SELECT) return;
    __syncthreads();
    if (!sh_last) return;
    // the growth steps' fused kernel carries ONE instantiation of the bookkeeping (node records in LDS: the host takes the two-launch path when
    // they do not fit, enqueue_growth_step) -- its speed depends on its size: a second inlined copy costs scalar spills and scratch in every block
    if (!ROOT && !DIST && !JAVA) select_step_t<true>(c, false, (unsigned char *)sh_raw, false);
    else select_step(c, ROOT, (unsigned char *)sh_raw, nodes_in_lds != 0, DIST);
}

template <bool ROOT, bool DIST, bool JAVA = false>
#ifndef RL_FIN_WAVES
#define RL_FIN_WAVES 4
#endif
#if RL_FIN_WAVES
__attribute__((amdgpu_waves_per_eu(RL_FIN_WAVES)))
#endif
__global__ __launch_bounds__(kFinThreads) void k_hist_finish(const Ctx c, int nodes_in_lds)
{   // grid (F, slots); the last block to arrive also runs select_step
    extern __shared__ unsigned long long sh_raw[];
    hist_finish_body<ROOT, DIST, JAVA, true>(c, nodes_in_lds, sh_raw);
}

// Wide data (hundreds of live features x kSpec slots = thousands of blocks a step): the bookkeeping that ONE block runs sets the register budget of
// all of them (96 VGPRs = 5 blocks a CU = 1280 resident blocks: a step's blocks came in two rounds and the last block waited 15-45 us for the
// second).  Without it the per-feature work needs 56 registers: 8 blocks a CU, one round; select_step then costs a launch of its own (~5 us).
__attribute__((amdgpu_waves_per_eu(8)))
__global__ __launch_bounds__(kFinWideThreads) void k_hist_finish_wide(const Ctx c)
{
    extern __shared__ unsigned long long sh_raw[];
    hist_finish_body<false, false, false, false>(c, 0, sh_raw);
}
__global__ __launch_bounds__(kFinThreads) void k_select(const Ctx c, int nodes_in_lds)
{
    extern __shared__ unsigned long long sh_raw[];
    if (c.st->done || c.st->nslots <= 0) return;        // a finished or stalled tree: the step is empty (the fused kernel's blocks all leave before they arrive)
    select_step<true>(c, false, (unsigned char *)sh_raw, nodes_in_lds != 0, false);
}

}  // namespace rl
