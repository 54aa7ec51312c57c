// rl_k_best.inc -- K4/K5, second part: how a feature's best split reaches the block that runs select_step.  RL_CLK, FeatBest, the agent-scope
// stores and loads, publish_best, PartKey and half_wave_best_feature (the best feature of a new node, with the tie flags).
// Included by rl_kernels_round.inc; needs that file's i128 helpers and, under RL_PHASE_CLOCKS, the strict_clock of its trace block.

namespace rl {

// ------------------------------------------------------------------------------------------------
#ifdef RL_PHASE_CLOCKS
#define RL_CLK(cond, k) do { if (cond) { const long long t_ = strict_clock(); if (threadIdx.x == 0) c.clk[(c.st->step & 63) * 32 + (k)] = t_; } } while (0)
#else
#define RL_CLK(cond, k) do { } while (0)
#endif

// Growth bookkeeping (select_step), run by the LAST block of k_hist_finish to arrive: best split of the new nodes
// across features (lowest feature index wins a tie, FeatureHistogram.java:302-309), then the best-first
// bookkeeping of RegressionTree.fit (:58-87) on LDS copies of TreeState, the node records and the queue (a single
// lane walking device memory pays ~1 us per dependent access).
//
// Speculative best-first growth.  RegressionTree.fit pops one node at a time, so a literal device version pays the
// latency of a chain of dependent kernels per split.  Here every step PREPARES up to kSpec nodes from the front of
// the queue at once (partition, child histograms, child best splits); the fit loop itself is replayed exactly and
// only COMMITS prepared nodes in the order the Java pops them.  Preparing a node writes nothing a committed node can
// see (new node records, the other ping-pong half of the node's own sample range, new histogram slots), so a
// prepared node that the loop never reaches (leaf budget exhausted) simply stays a leaf.
// ------------------------------------------------------------------------------------------------
// Per-feature results of k_hist_finish travel from its blocks to the one block that runs select_step INSIDE the same
// launch: agent-scope (write-through) stores, s_waitcnt, arrival counter -- no device-wide fence (on this 8-XCD
// part a __threadfence() per block costs an L2 write-back each).
struct FeatBest {           // best split of one feature for one new node + the cumulative histogram entry there
    unsigned long long S;    // double bits
    unsigned long long hi, lo;   // exact cumulative fixed-point sum at the split (= the left child's total)
    unsigned long long tc;   // (t << 32) | count at the split; bit 62: another threshold of this feature reaches the same S exactly
};
constexpr unsigned long long kFbTie = 1ull << 62, kFbTieDiff = 1ull << 61;
constexpr int kStepLogCap = 8192;      // entries of Ctx::steplog
template <class T> __device__ __forceinline__ void st_agent(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// What the finish blocks published (write-through stores, completed before they arrived) is read by the block that runs select_step with PLAIN loads
// behind ONE agent-scope acquire fence at its entry (it invalidates the stale lines this CU / XCD may hold of the records' fixed addresses).  Relaxed
// atomic loads were correct too, but the compiler completes each group of them (s_waitcnt vmcnt(0)) before it issues the next: a lane's five
// records were five dependent memory round trips in the step's serial tail, 22 with 700 features.
template <class T> __device__ __forceinline__ T ld_agent(const T *p) { return *p; }

// tie: bit 0 = another threshold of the feature reaches the same S, bit 1 = ... and cuts off other documents
__device__ __forceinline__ void publish_best(const Ctx &c, int slot, int side, int f, double S, int t, int cl, long long hi, unsigned long long lo, int tie = 0)
{
    FeatBest *o = c.fb + ((size_t)slot * 2 + side) * c.F + f;         // one 32-byte record: a single write-through line
    st_agent(&o->S, (unsigned long long)__double_as_longlong(S));
    st_agent(&o->hi, (unsigned long long)hi); st_agent(&o->lo, lo);
    st_agent(&o->tc, ((unsigned long long)(unsigned)t << 32) | (unsigned)cl | ((tie & 1) ? kFbTie : 0ull) | ((tie & 2) ? kFbTieDiff : 0ull));
}

// best split across features (lowest feature index wins a tie, FeatureHistogram.java:302-309).  A HALF wavefront per
// (slot, side): the 2 * kSpec reductions of a step then fit into one pass over the block's wavefronts.  `valid` is uniform
// in the half; every lane of the wavefront must call (shuffles).
// Feature sampling (c.fs_size < F, Random Forests): the node's draw = the fs_size features with the smallest keys
// feature_key(h, f), visited in key order, so a feature's RANK among the keys replaces its index: rank >= fs_size = not
// drawn, lowest rank wins a tie (:283-309).  fkeys: F words of LDS scratch owned by this half.
// The two sample sets a candidate cuts a node into, as an exact key: (documents, fixed-point sum) of the SMALLER side (of the side with the
// smaller sum when the counts are equal).  Candidates with equal keys have exactly equal true gains -- the same cut, or a mirrored one whose
// f64 S differs in the last bits only because sumRight = total - sumLeft is rounded (rl_tie.inc re-decides both kinds in the Java's order).
#ifndef RL_FB_BATCH
#define RL_FB_BATCH 8
#endif
struct PartKey { int cnt; i128 sum; };
__device__ __forceinline__ PartKey part_key(int cl, i128 sl, int ctot, i128 tot)
{
    const int cr = ctot - cl; const i128 sr = tot - sl;
    PartKey k;
    if (cl < cr) { k.cnt = cl; k.sum = sl; }
    else if (cl > cr) { k.cnt = cr; k.sum = sr; }
    else { k.cnt = cl; k.sum = sl < sr ? sl : sr; }
    return k;
}

// nthi / ntlo / nctot: the node's exact totals (for the mirrored-cut check; unused without the lazy tie-break)
// WIDE (k_select: the bookkeeping kernel of data with hundreds of features, where the block is alone on the chip and registers are free): all the gains
// of the lane's share (up to kWideS x 32 features) are requested at once and stay in registers for the tie pass -- at 700 features the three batches of
// eight, the winner's fields and the tie pass's second scan of the gains were seven dependent round trips (8-9 us of every growth step).
constexpr int kWideS = 24;
template <bool WIDE = false>
__device__ __forceinline__ void half_wave_best_feature(const Ctx &c, bool valid, int slot, int side, unsigned long long h, unsigned long long *fkeys,
                                       double &S, int &f, int &t, int &cl, long long &hi, unsigned long long &lo, int &tie,
                                       long long nthi = 0, unsigned long long ntlo = 0, int nctot = 0)
{
    const FeatBest *o = c.fb + ((size_t)slot * 2 + side) * c.F;
    const int hl = lane_id() & 31, hbase = lane_id() & 32;
    const bool sampling = c.fs_on != 0;
    if (sampling) {       // (the draw is over the REAL features: every run of a split threshold table carries its column's key -- Ctx::fcol, rl_init)
        if (valid) for (int i = hl; i < c.F; i += 32) fkeys[i] = feature_key(h, c.fcol[i] & 0x7fffffff);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    // every lane keeps the whole record of its best feature: the winner's fields come from a lane, not from a second
    // round trip to memory
    double bs = -1.0; int bf = -1, br = 0x7fffffff;
    unsigned long long bhi = 0, blo = 0, btc = 0;
    bool eq = false;            // another feature of this lane's share reaches the lane's best S exactly
    // Up to 32 * kFbFull features (the MSLR shape: 136): every lane asks for the WHOLE records of its share at once -- one memory round trip for the
    // gains, the winner's fields and the tie pass below, instead of three dependent ones (6-9 us of the step's serial tail were these loads).
    constexpr int kFbFull = 5;
    const bool small = !sampling && c.F <= 32 * kFbFull;
    unsigned long long kS[kFbFull], kH[kFbFull], kL[kFbFull], kT[kFbFull];
    [[maybe_unused]] unsigned long long wS[WIDE ? kWideS : 1];
#pragma unroll
    for (int u = 0; u < kFbFull; u++) { kS[u] = 0xbff0000000000000ull; kH[u] = kL[u] = kT[u] = 0ull; }
    if (valid && small) {
#pragma unroll
        for (int u = 0; u < kFbFull; u++) {
            const int i = hl + 32 * u;
            if (i < c.F) { kS[u] = ld_agent(&o[i].S); kH[u] = ld_agent(&o[i].hi); kL[u] = ld_agent(&o[i].lo); kT[u] = ld_agent(&o[i].tc); }
        }
#pragma unroll
        for (int u = 0; u < kFbFull; u++) {
            const int i = hl + 32 * u;
            const double s = __longlong_as_double((long long)kS[u]);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs) { eq = false; bs = s; bf = i; br = i; bhi = kH[u]; blo = kL[u]; btc = kT[u]; }         // (ascending i: the first of equal gains stays)
        }
    } else if (WIDE && valid && !sampling && c.F <= 32 * kWideS) {
#pragma unroll
        for (int u = 0; u < kWideS; u++) wS[u] = ld_agent(&o[min(hl + 32 * u, c.F - 1)].S);
#pragma unroll
        for (int u = 0; u < kWideS; u++) {
            const int i = hl + 32 * u;
            if (i >= c.F) wS[u] = 0xbff0000000000000ull /* -1.0 */;
            const double s = __longlong_as_double((long long)wS[u]);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs) { eq = false; bs = s; bf = i; br = i; }         // (ascending i: the first of equal gains stays)
        }
        if (bf >= 0) { bhi = ld_agent(&o[bf].hi); blo = ld_agent(&o[bf].lo); btc = ld_agent(&o[bf].tc); }
    } else if (valid && !sampling) {
        // Eight gains per lane are requested at once (the loads are agent-scope atomics: one at a time they cost a memory round trip per feature of
        // the lane's share -- 22 of them with 700 features, 16-19 us of this block's serial tail); the rest of a record is fetched for the lane's best only.
        constexpr int B = RL_FB_BATCH;
        for (int i0 = hl; i0 < c.F; i0 += 32 * B) {
            unsigned long long rs[B];
#pragma unroll
            for (int u = 0; u < B; u++) { const int i = i0 + 32 * u; rs[u] = (i < c.F) ? ld_agent(&o[i].S) : 0xbff0000000000000ull /* -1.0 */; }
#pragma unroll
            for (int u = 0; u < B; u++) {
                const int i = i0 + 32 * u;
                const double s = __longlong_as_double((long long)rs[u]);
                if (s == bs && s > -1.0) eq = true;
                if (s > bs) { eq = false; bs = s; bf = i; br = i; }         // (ascending i: the first of equal gains stays)
            }
        }
        if (bf >= 0) { bhi = ld_agent(&o[bf].hi); blo = ld_agent(&o[bf].lo); btc = ld_agent(&o[bf].tc); }
    } else if (valid) {
        for (int i = hl; i < c.F; i += 32) {
            const unsigned long long rs = ld_agent(&o[i].S), rh = ld_agent(&o[i].hi), rl = ld_agent(&o[i].lo), rt = ld_agent(&o[i].tc);
            int rank = i;
            {
                const unsigned long long ki = fkeys[i];
                rank = 0;
                // one count per real column: fcol[g] < 0 marks the later runs of a split table (they share their column's rank; the lower run wins an equal gain)
                const int ci = c.fcol[i] & 0x7fffffff;
                for (int g = 0; g < c.F; g++) { const int cg = c.fcol[g]; const unsigned long long kg = fkeys[g]; rank += (cg >= 0) && ((kg < ki) || (kg == ki && cg < ci)); }
                if (rank >= c.fs_size) continue;
            }
            const double s = __longlong_as_double((long long)rs);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs || (s == bs && s > -1.0 && rank < br)) { if (s > bs) eq = false; bs = s; bf = i; br = rank; bhi = rh; blo = rl; btc = rt; }
        }
    }
    RL_CLK(slot == 0 && side == 0 && valid, 17);       // the lane's share of the records has arrived and is reduced
    const int own = bf;         // this lane's candidate (its fields are in bhi / blo / btc)
    const double own_s = bs;
    for (int d = 16; d > 0; d >>= 1) {
        const double s = __shfl_xor(bs, d); const int ff = __shfl_xor(bf, d), rr = __shfl_xor(br, d);
        if (s > bs || (s == bs && ff >= 0 && (bf < 0 || rr < br || (rr == br && ff < bf)))) { bs = s; bf = ff; br = rr; }
    }
    S = bs; f = bf; t = -1; cl = 0; hi = 0; lo = 0;
    // the winner is the own candidate of exactly one lane of this half (ranks are distinct)
    RL_CLK(slot == 0 && side == 0 && valid, 18);       // ... across the half wavefront
    const unsigned long long ownmask = __ballot(bf >= 0 && own == bf) >> hbase;
    const int src = hbase + (int)__builtin_ctzll(ownmask | (1ull << 63));
    const unsigned long long tc = (unsigned long long)__shfl((long long)btc, src);
    const long long h2 = __shfl((long long)bhi, src); const unsigned long long l2 = (unsigned long long)__shfl((long long)blo, src);
    // exact ties (rl_tie.inc): several features reach the best S (2), or only other thresholds of the winning feature do (1)
    unsigned long long cross = __ballot(bf >= 0 && own >= 0 && own_s == bs && (own != bf || eq)) >> hbase;
    bool other_cut = false;     // a tied candidate of this lane's share does not have the winner's (left count, left sum): a mirrored or a different cut
    if (c.tie_on) {       // mirrored cuts of other features: equal partition keys although the f64 S differ by a rounding
        bool mir = false;
        if (valid && bf >= 0 && small) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
#pragma unroll
            for (int u = 0; u < kFbFull; u++) {
                const int i = hl + 32 * u;
                if (i == bf) continue;
                const double s = __longlong_as_double((long long)kS[u]);
                if (!(s > -1.0) || fabs(s - bs) > 1e-9 * fabs(bs)) continue;
                const unsigned long long itc = kT[u];
                const i128 isl = make_i128((long long)kH[u], kL[u]);
                const PartKey k = part_key((int)(unsigned)itc, isl, nctot, ntot);
                const bool keq = (k.cnt == wk.cnt && k.sum == wk.sum);
                mir |= keq;
                if (keq || s == bs) other_cut |= !((unsigned)itc == (unsigned)tc && isl == wsl) || (itc & kFbTieDiff) != 0;
            }
        } else if (WIDE && valid && bf >= 0 && !sampling && c.F <= 32 * kWideS) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
            // the near-equal gains of the share as bit masks (registers cannot be indexed by a run-time u); the records behind them -- rare -- come from memory
            unsigned near = 0u, exact = 0u;
#pragma unroll
            for (int u = 0; u < kWideS; u++) {
                const double s = __longlong_as_double((long long)wS[u]);
                if (hl + 32 * u != bf && s > -1.0 && !(fabs(s - bs) > 1e-9 * fabs(bs))) { near |= 1u << u; if (s == bs) exact |= 1u << u; }
            }
            while (near) {
                const int u = __builtin_ctz(near);
                near &= near - 1u;
                const int i = hl + 32 * u;
                const unsigned long long itc = ld_agent(&o[i].tc);
                const i128 isl = make_i128((long long)ld_agent(&o[i].hi), ld_agent(&o[i].lo));
                const PartKey k = part_key((int)(unsigned)itc, isl, nctot, ntot);
                const bool keq = (k.cnt == wk.cnt && k.sum == wk.sum);
                mir |= keq;
                if (keq || ((exact >> u) & 1u)) other_cut |= !((unsigned)itc == (unsigned)tc && isl == wsl) || (itc & kFbTieDiff) != 0;
            }
        } else if (valid && bf >= 0) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
            constexpr int B = RL_FB_BATCH;
            for (int i0 = hl; i0 < c.F; i0 += 32 * B) {
              unsigned long long rs[B];
#pragma unroll
              for (int u = 0; u < B; u++) { const int i = i0 + 32 * u; rs[u] = (i < c.F) ? ld_agent(&o[i].S) : 0xbff0000000000000ull; }
#pragma unroll
              for (int u = 0; u < B; u++) {
                const int i = i0 + 32 * u;
                if (i == bf) continue;
                const double s = __longlong_as_double((long long)rs[u]);
                if (!(s > -1.0) || fabs(s - bs) > 1e-9 * fabs(bs)) continue;
                const unsigned long long itc = ld_agent(&o[i].tc);
                const i128 isl = make_i128((long long)ld_agent(&o[i].hi), ld_agent(&o[i].lo));
                const PartKey k = part_key((int)(unsigned)itc, isl, nctot, ntot);
                const bool keq = (k.cnt == wk.cnt && k.sum == wk.sum);
                mir |= keq;
                if (keq || s == bs) other_cut |= !((unsigned)itc == (unsigned)tc && isl == wsl) || (itc & kFbTieDiff) != 0;
              }
            }
        }
        cross |= __ballot(mir) >> hbase;
    }
    RL_CLK(slot == 0 && side == 0 && valid, 19);       // tie pass
    const bool any_other = (__ballot(other_cut) >> hbase) & 0xffffffffull;
    tie = 0;
    if (bf >= 0) {
        t = (int)((tc >> 32) & 0xffffu); cl = (int)(unsigned)tc; hi = h2; lo = l2;
        // 2 = the Java's noise picks among several features, or among thresholds with other counts; 1 = thresholds of the winning feature that all cut
        // off the same documents; 4 (with 2) = every tied candidate of every feature cuts off the winner's (left count, exact left sum) -- the same
        // documents unless a coincidence of lambdas says otherwise, which the deferred tie-break verifies (rl_tie.inc); bits 8..: lanes (of 32)
        // whose share holds a tied feature
        tie = (cross & 0xffffffffull) ? (2 | (__builtin_popcountll(cross & 0xffffffffull) << 8)) : ((tc & kFbTieDiff) ? 2 : ((tc & kFbTie) ? 1 : 0));
        if ((cross & 0xffffffffull) && !any_other && !(tc & kFbTieDiff)) tie |= 4;
    }
}

}  // namespace rl
