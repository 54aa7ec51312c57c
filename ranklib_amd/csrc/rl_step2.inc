// rl_step2.inc -- the growth step's second half as two short launches (round 5): k_fin2 (per-feature finish of the new nodes) and
// k_select2 (the best-first bookkeeping), replacing the fused k_hist_finish<false> + last-block select_step on the plain one-GPU path.
//
// Why.  Block-level traces (profiles/r04_step_trace_*) put 16 us of every 98-us growth step into the finish blocks and 17 us into the
// one-block bookkeeping behind the last of them -- for a few hundred KB.  The ISA said what that time is made of: every `__shfl_xor` /
// `__shfl_up` is a ds_bpermute_b32 followed by `s_waitcnt lgkmcnt(0)`, i.e. each step of a wave reduction is a round trip through the LDS
// pipe (~0.06 us), a 128-bit scan is 6 of them, and the two kernels were chains of ~25 such reductions between ~12 block barriers, plus
// write-through stores, two levels of arrival atomics and an acquire fence to hand the per-feature records to the last block.
// Here: one bin per thread, ONE wave scan on the DPP data path (rl_wave.h) that yields the chunk-reduced prefix, the mode bin and the wave
// totals at once, two block barriers, plain stores (the launch boundary publishes them), and a bookkeeping kernel of its own whose
// reductions are DPP as well.  Results are bit-identical to hist_finish_body / select_step_t (same formulas, same candidate order).
//
// Reference: FeatureHistogram.java:141-145,189-194 (prefix), :222-234 (sibling = parent - built), :236-264 (gain scan, first maximum wins),
// :302-309 (first maximum over the features); RegressionTree.java:58-87,147-157 (fit loop, insert).

namespace rl {

constexpr int kFin2Threads = 320;       // one thread per bin: the -tc 256 tables have 257 entries
constexpr int kFin2Waves = kFin2Threads / 64;
constexpr int kFin2MaxT = kFin2Threads;

struct Fin2WaveRec { double S; int t, c, flags; };       // a wavefront's best candidate of one side; flags: 1 = another threshold of the wave ties with it, 2 = .. with another left count

// grid (live features, kSpec slots).  Thread t owns bin t of feature f of the slot's BUILT child B (the smaller one, accumulated from its
// documents by k_hist<false>); its sibling S = parent - B.
// DIST (round 6, sharded runs): the bins come from the all-reduced limbs (k_hist_reduce has summed this rank's chunk partials and rebuilt the mode
// bin, the all-reduce the ranks: exact integers, FeatureHistogram.java:296-309 is the cross-worker merge this replaces) instead of the chunk
// partials; the built child's global document count is the last cumulative count; block (0, slot) hands the all-reduced lambda^2 sum on.
template <bool DIST = false>
__global__ __launch_bounds__(kFin2Threads) void k_fin2(const Ctx c)
{
    const TreeState *st = c.st;
    RL_TR_BEGIN();
    const int slot = blockIdx.y;
    const int st_done = st->done, st_nslots = st->nslots, E = st->E;
    const SlotRec sl = st->slot[slot];                      // (copied whole, valid or not: slot < kSpec)
    const int f = (!DIST && c.live) ? c.live[blockIdx.x] : (int)blockIdx.x;
    const int TS = c.TS, T = (!DIST && c.live) ? c.live_nthr[blockIdx.x] : c.nthr[f];
    if (st_done || slot >= st_nslots) return;
    const bool sq_block = blockIdx.x == 0;                  // block (0, slot) also folds the partition's per-tile lambda^2 partials of the built child
    if (sl.skip_hist && !sq_block) return;                  // (the split that fills the leaf budget: no child histogram exists, k_select2)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nodeP = sl.node, nodeB = sl.build_left ? sl.left : sl.right, nodeS = sl.build_left ? sl.right : sl.left, sideB = sl.build_left ? 0 : 1;
    const int ch0 = sl.chunk0;
    const int cntB_local = DIST ? 0 : (sl.build_left ? sl.nleft : sl.pcount - sl.nleft);         // one GPU: known from the count histogram
    const int csB = sl.cs > 0 ? sl.cs : chunk_docs<false>(c, cntB_local);
    const int nch = DIST ? 0 : (cntB_local + csB - 1) / csB;
    const bool has = tid < T;
    const int tc = min(tid, T - 1);                         // every load below is unconditional, from a clamped index
    RL_TR_MARK(1);
    // ---- everything the block reads is requested before anything is used
    const size_t oP = ((size_t)nodeP * c.F + f) * TS;
    const long long par_hi = c.cum_hi[oP + tc]; const unsigned long long par_lo = c.cum_lo[oP + tc]; const int par_cn = c.cum_cnt[oP + tc];
    const long long tp_hi = c.cum_hi[oP + T - 1]; const unsigned long long tp_lo = c.cum_lo[oP + T - 1]; const int tp_cn = c.cum_cnt[oP + T - 1];
    const int mode = c.mode[f];
    i128 ptot = 0;                                          // this thread's share of the chunk totals (sum of q over the chunk's documents)
    if (!DIST) {
        const long long v0 = c.part_tot[ch0 + max(min(tid, nch - 1), 0)];
        if (tid < nch) ptot = (i128)v0;
        for (int ch = tid + kFin2Threads; ch < nch; ch += kFin2Threads) ptot += (i128)c.part_tot[ch0 + ch];
    }
    long long sqacc = 0;
    const size_t slot_words = DIST ? (size_t)c.F * TS * c.limb_words + 4 : 0;
    if (DIST) { if (sq_block && tid == 0) sqacc = c.dist_buf[slot * slot_words + (size_t)c.F * TS * c.limb_words]; }       // all-reduced by the step's collective
    else if (sq_block) {
        constexpr int kSqBatch = 8;
        for (int i0 = tid; i0 < sl.ntiles; i0 += kSqBatch * kFin2Threads) {
            long long v[kSqBatch];
#pragma unroll
            for (int u = 0; u < kSqBatch; u++) v[u] = c.tile_sq[sl.tile0 + min(i0 + u * kFin2Threads, sl.ntiles - 1)];
#pragma unroll
            for (int u = 0; u < kSqBatch; u++) if (i0 + u * kFin2Threads < sl.ntiles) sqacc += v[u];
        }
    }
    __shared__ long long s_wsq[kFin2Waves];
    if (sl.skip_hist) {       // (uniform) only the lambda^2 sum
        const long long wsq = (long long)wave_sum_u64((unsigned long long)sqacc);
        if (lane == 63) s_wsq[wave] = wsq;
        __syncthreads();
        if (tid == 0) { long long v = 0; for (int w = 0; w < kFin2Waves; w++) v += s_wsq[w]; c.fb_sq[slot] = (unsigned long long)v; }
        return;
    }
    i128 raw = 0; unsigned rawc = 0;
    if (DIST) {
        const int W = c.limb_words;
        const long long *in = c.dist_buf + slot * slot_words + (size_t)f * TS * W;
        long long hi, lo, cn;
        if (W == 3) { hi = in[3 * tc]; lo = in[3 * tc + 1]; cn = in[3 * tc + 2]; }
        else { const long long w0 = in[2 * tc]; cn = w0 & 0xffffffffll; hi = w0 >> 32; lo = in[2 * tc + 1]; }   // the counts of all ranks sum to < 2^31
        if (has) { raw = (((i128)hi) << kLimbShift) + (i128)lo; rawc = (unsigned)cn; }
    } else {
        const size_t cstride = (size_t)c.F * TS;
        const long long *ps = c.part_sum + ((size_t)ch0 * c.F + f) * TS + tc;
        const int *pc = c.part_cnt + ((size_t)ch0 * c.F + f) * TS + tc;
#ifndef RL_FIN2_BATCH
#define RL_FIN2_BATCH 16
#endif
        constexpr int kBatch = RL_FIN2_BATCH;               // chunk partials in flight; the 64-bit halves are summed apart: no carry chain ties a load to the one before
        unsigned long long lo = 0; long long hi = 0; int cacc = 0;
        for (int ch = 0; ch < nch; ch += kBatch) {
            long long v[kBatch]; int cn[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; u++) { const size_t o = (size_t)min(ch + u, nch - 1) * cstride; v[u] = ps[o]; cn[u] = pc[o]; }
#pragma unroll
            for (int u = 0; u < kBatch; u++) if (ch + u < nch) { lo += (unsigned long long)(unsigned)v[u]; hi += (v[u] >> 32); cacc += cn[u]; }
        }
        if (has) { raw = (i128)lo + (((i128)hi) << 32); rawc = (unsigned)cacc; }
    }
    RL_TR_MARK(2);
    // ---- one scan: prefix inside the wavefront, wave totals for the block prefix and for the mode-bin rebuild
    const i128 inc = wave_scan_i128(raw);
    const unsigned cinc = wave_scan_u32(rawc);
    const i128 wpt = wave_sum_i128(ptot);
    __shared__ i128 s_wtot[kFin2Waves], s_wpt[kFin2Waves];
    __shared__ unsigned s_wcnt[kFin2Waves];
    __shared__ Fin2WaveRec s_rec[2][kFin2Waves];
    if (lane == 63) { s_wtot[wave] = inc; s_wcnt[wave] = cinc; s_wpt[wave] = wpt; }
    if (sq_block) { const long long wsq = (long long)wave_sum_u64((unsigned long long)sqacc); if (lane == 63) s_wsq[wave] = wsq; }
    __syncthreads();
    i128 others = 0, off = 0, totB = 0; unsigned oc = 0, coff = 0;
#pragma unroll
    for (int w = 0; w < kFin2Waves; w++) {
        const i128 wt = s_wtot[w]; const unsigned wc = s_wcnt[w];
        others += wt; oc += wc; totB += s_wpt[w];
        if (w < wave) { off += wt; coff += wc; }
    }
    // the mode bin was never accumulated (k_hist): node total - the other bins, exact in fixed point (DIST: k_hist_reduce has rebuilt it before the all-reduce)
    if (DIST) totB = others;
    const int cntB = DIST ? (int)oc : cntB_local;
    const i128 mv = DIST ? (i128)0 : totB - others; const unsigned mc = DIST ? 0u : (unsigned)cntB - oc;
    const i128 vb = inc + off + (tid >= mode ? mv : (i128)0);
    const int cb = (int)(cinc + coff + (tid >= mode ? mc : 0u));
    const i128 vs = make_i128(par_hi, par_lo) - vb;         // FeatureHistogram.java:230-231
    const int cs2 = par_cn - cb;
    const i128 totS = make_i128(tp_hi, tp_lo) - totB;
    const int ctotB = cntB, ctotS = tp_cn - cntB;
    if (has) {
        const size_t oB = ((size_t)nodeB * c.F + f) * TS + tid, oS = ((size_t)nodeS * c.F + f) * TS + tid;
        c.cum_hi[oB] = hi_of(vb); c.cum_lo[oB] = lo_of(vb); c.cum_cnt[oB] = cb;
        c.cum_hi[oS] = hi_of(vs); c.cum_lo[oS] = lo_of(vs); c.cum_cnt[oS] = cs2;
    }
    RL_TR_MARK(3);
    const double sumB = fixed_to_double(totB, E), sumS = fixed_to_double(totS, E);
    bool okb = false, oks = false;
    double Sb = -1.0, Ss = -1.0;
    if (has) {
        Sb = gain_S(fixed_to_double(vb, E), cb, sumB, ctotB, c.mls, okb);
        Ss = gain_S(fixed_to_double(vs, E), cs2, sumS, ctotS, c.mls, oks);
    }
    RL_TR_MARK(4);
    // first maximum of the wavefront: S >= 0 orders like its bit pattern, the lowest lane is the lowest threshold (one bin per thread); exact ties
    // inside the feature (rl_tie.inc): another threshold reaches the best S bit for bit -- thresholds are nested, so an equal left count means
    // the same documents
    {
        const unsigned long long kb = okb ? d2bits(Sb) + 1ull : 0ull, ks = oks ? d2bits(Ss) + 1ull : 0ull;
        const unsigned long long mxb = wave_max_u64(kb), mxs = wave_max_u64(ks);
        const unsigned long long mkb = __ballot(kb == mxb && kb != 0ull), mks = __ballot(ks == mxs && ks != 0ull);
        const int lb_ = mkb ? (int)__builtin_ctzll(mkb) : 0, ls_ = mks ? (int)__builtin_ctzll(mks) : 0;
        const int wcb = (int)readlane_u32((uint32_t)cb, lb_), wcs = (int)readlane_u32((uint32_t)cs2, ls_);
        const int fb_ = (__builtin_popcountll(mkb) > 1 ? 1 : 0) | (__ballot(kb == mxb && kb != 0ull && cb != wcb) ? 2 : 0);
        const int fs_ = (__builtin_popcountll(mks) > 1 ? 1 : 0) | (__ballot(ks == mxs && ks != 0ull && cs2 != wcs) ? 2 : 0);
        if (lane == 0) {
            Fin2WaveRec r;
            r.S = mkb ? bits2d(mxb - 1ull) : -1.0; r.t = mkb ? wave * 64 + lb_ : -1; r.c = wcb; r.flags = fb_; s_rec[0][wave] = r;
            r.S = mks ? bits2d(mxs - 1ull) : -1.0; r.t = mks ? wave * 64 + ls_ : -1; r.c = wcs; r.flags = fs_; s_rec[1][wave] = r;
        }
    }
    __syncthreads();
    WBest gb = {-1.0, -1, 0}, gs = {-1.0, -1, 0};
#pragma unroll
    for (int w = 0; w < kFin2Waves; w++) {
        const Fin2WaveRec rb = s_rec[0][w], rs = s_rec[1][w];
        WBest x; x.S = rb.S; x.t = rb.t; x.c = rb.c; gb = wbetter(gb, x);
        x.S = rs.S; x.t = rs.t; x.c = rs.c; gs = wbetter(gs, x);
    }
    int tieb = 0, ties = 0;
#pragma unroll
    for (int w = 0; w < kFin2Waves; w++) {
        const Fin2WaveRec rb = s_rec[0][w], rs = s_rec[1][w];
        if (rb.t >= 0 && rb.S == gb.S) { if (rb.t != gb.t || (rb.flags & 1)) tieb |= 1; if (rb.c != gb.c || (rb.flags & 2)) tieb |= 2; }
        if (rs.t >= 0 && rs.S == gs.S) { if (rs.t != gs.t || (rs.flags & 1)) ties |= 1; if (rs.c != gs.c || (rs.flags & 2)) ties |= 2; }
    }
    if (!(tieb & 1)) tieb = 0;
    if (!(ties & 1)) ties = 0;
    RL_TR_MARK(5);
    // the thread that owns the winning bin has the whole record in registers (plain stores: the next launch reads them)
    if (tid == max(gb.t, 0)) {
        FeatBest *o = c.fb + ((size_t)slot * 2 + sideB) * c.F + f;
        o->S = (unsigned long long)__double_as_longlong(gb.S); o->hi = (unsigned long long)hi_of(vb); o->lo = lo_of(vb);
        o->tc = ((unsigned long long)(unsigned)gb.t << 32) | (unsigned)cb | ((tieb & 1) ? kFbTie : 0ull) | ((tieb & 2) ? kFbTieDiff : 0ull);
    }
    if (tid == max(gs.t, 0)) {
        FeatBest *o = c.fb + ((size_t)slot * 2 + (1 - sideB)) * c.F + f;
        o->S = (unsigned long long)__double_as_longlong(gs.S); o->hi = (unsigned long long)hi_of(vs); o->lo = lo_of(vs);
        o->tc = ((unsigned long long)(unsigned)gs.t << 32) | (unsigned)cs2 | ((ties & 1) ? kFbTie : 0ull) | ((ties & 2) ? kFbTieDiff : 0ull);
    }
    if (sq_block && tid == 0) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kFin2Waves; w++) v += s_wsq[w];
        c.fb_sq[slot] = (unsigned long long)v;
    }
    RL_TR_END(2, blockIdx.y * gridDim.x + blockIdx.x);
}


// The root's finish (FeatureHistogram.update's prefix :141-145 + the root's gain scan): the same kernel shape with three chunk groups of 320
// threads each -- the root pass leaves N / 16384 chunk partials per bin (231 at 3.77 M documents), and one thread per bin walked them in
// fifteen dependent batches.  Counts are static (the root's, from rl_init); no sibling.  grid (live features).
constexpr int kFin2RootGroups = 3, kFin2RootThreads = kFin2RootGroups * kFin2Threads;
__global__ __launch_bounds__(kFin2RootThreads) void k_fin2_root(const Ctx c, int nch)
{
    const TreeState *st = c.st;
    const int E = st->E;
    const int f = c.live ? c.live[blockIdx.x] : (int)blockIdx.x;
    const int TS = c.TS, T = c.live ? c.live_nthr[blockIdx.x] : c.nthr[f];
    const int tid = threadIdx.x, grp = tid / kFin2Threads, bt = tid - grp * kFin2Threads;      // bin of this thread
    const int lane = tid & 63;
    const bool has = bt < T;
    const int tc = min(bt, T - 1);
    const int mode = c.mode[f];
    const int cb = c.cum_cnt[(size_t)f * TS + tc];           // node 0: the static cumulative counts (FeatureHistogram.java:138 "count doesn't change")
    const int ctotB = c.cum_cnt[(size_t)f * TS + T - 1];
    i128 ptot = 0;
    for (int ch = tid; ch < nch; ch += kFin2RootThreads) ptot += (i128)c.part_tot[ch];
    unsigned long long lo = 0; long long hi = 0;
    {
        const size_t cstride = (size_t)c.F * TS;
        const long long *ps = c.part_sum + (size_t)f * TS + tc;
        constexpr int kBatch = 16;
        for (int ch = grp; ch < nch; ch += kBatch * kFin2RootGroups) {
            long long v[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; u++) v[u] = ps[(size_t)min(ch + u * kFin2RootGroups, nch - 1) * cstride];
#pragma unroll
            for (int u = 0; u < kBatch; u++) if (ch + u * kFin2RootGroups < nch) { lo += (unsigned long long)(unsigned)v[u]; hi += (v[u] >> 32); }
        }
    }
    __shared__ unsigned long long s_lo[kFin2RootGroups - 1][kFin2Threads];
    __shared__ long long s_hi[kFin2RootGroups - 1][kFin2Threads];
    __shared__ i128 s_gpt[kFin2RootThreads / 64];
    __shared__ i128 s_wtot[kFin2Waves];
    __shared__ Fin2WaveRec s_rec[kFin2Waves];
    const i128 wpt = wave_sum_i128(ptot);
    if (lane == 63) s_gpt[tid >> 6] = wpt;
    if (grp > 0) { s_lo[grp - 1][bt] = lo; s_hi[grp - 1][bt] = hi; }
    __syncthreads();
    if (grp > 0) return;
    const int wave = tid >> 6;
#pragma unroll
    for (int g2 = 0; g2 < kFin2RootGroups - 1; g2++) { lo += s_lo[g2][bt]; hi += s_hi[g2][bt]; }
    const i128 raw = has ? ((i128)lo + (((i128)hi) << 32)) : (i128)0;
    const i128 inc = wave_scan_i128(raw);
    if (lane == 63) s_wtot[wave] = inc;
    __syncthreads();
    i128 others = 0, off = 0, totB = 0;
#pragma unroll
    for (int w = 0; w < kFin2Waves; w++) { const i128 wt = s_wtot[w]; others += wt; if (w < wave) off += wt; }
#pragma unroll
    for (int w = 0; w < kFin2RootThreads / 64; w++) totB += s_gpt[w];
    const i128 mv = totB - others;
    const i128 vb = inc + off + (bt >= mode ? mv : (i128)0);
    if (has) { const size_t oB = (size_t)f * TS + bt; c.cum_hi[oB] = hi_of(vb); c.cum_lo[oB] = lo_of(vb); }
    const double sumB = fixed_to_double(totB, E);
    bool okb = false; double Sb = -1.0;
    if (has) Sb = gain_S(fixed_to_double(vb, E), cb, sumB, ctotB, c.mls, okb);
    WBest mb; mb.S = okb ? Sb : -1.0; mb.t = okb ? bt : -1; mb.c = cb;
    const WBest wb = wave_best(mb);
    {
        const bool eqb = mb.t >= 0 && mb.S == wb.S && mb.t != wb.t, dfb = mb.t >= 0 && mb.S == wb.S && mb.c != wb.c;
        const int fb_ = (__ballot(eqb) ? 1 : 0) | (__ballot(dfb) ? 2 : 0);
        if (lane == 0) { Fin2WaveRec r; r.S = wb.S; r.t = wb.t; r.c = wb.c; r.flags = fb_; s_rec[wave] = r; }
    }
    __syncthreads();
    WBest gb = {-1.0, -1, 0};
#pragma unroll
    for (int w = 0; w < kFin2Waves; w++) { const Fin2WaveRec rb = s_rec[w]; WBest x; x.S = rb.S; x.t = rb.t; x.c = rb.c; gb = wbetter(gb, x); }
    int tieb = 0;
#pragma unroll
    for (int w = 0; w < kFin2Waves; w++) {
        const Fin2WaveRec rb = s_rec[w];
        if (rb.t >= 0 && rb.S == gb.S) { if (rb.t != gb.t || (rb.flags & 1)) tieb |= 1; if (rb.c != gb.c || (rb.flags & 2)) tieb |= 2; }
    }
    if (!(tieb & 1)) tieb = 0;
    if (bt == max(gb.t, 0)) {
        FeatBest *o = c.fb + f;                              // (slot 0, side 0)
        o->S = (unsigned long long)__double_as_longlong(gb.S); o->hi = (unsigned long long)hi_of(vb); o->lo = lo_of(vb);
        o->tc = ((unsigned long long)(unsigned)gb.t << 32) | (unsigned)cb | ((tieb & 1) ? kFbTie : 0ull) | ((tieb & 2) ? kFbTieDiff : 0ull);
    }
    if (blockIdx.x == 0 && tid == 0) { c.fb_root[0] = (unsigned long long)hi_of(totB); c.fb_root[1] = lo_of(totB); }
}

// the root's bookkeeping (select_step's is_root branch: the root record, its children's slot) as a launch of its own behind k_fin2_root
__global__ __launch_bounds__(kFinThreads) void k_select_root(const Ctx c, int nodes_in_lds)
{
    extern __shared__ unsigned long long sh_raw[];
    select_step(c, true, (unsigned char *)sh_raw, nodes_in_lds != 0, false);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// k_select2: the growth bookkeeping as a launch of its own (one block of four wavefronts).  What select_step_t does, in the same order and with the
// same results -- best split of the new nodes over the features (lowest feature wins, FeatureHistogram.java:302-309), the children's
// deviances (:348-350), RegressionTree.fit's loop (:58-87, insert :147-157) as far as prepared nodes allow, the next step's slots -- but
// laid out for latency: every global load is issued in the first instructions (the per-feature records, ALL node records, the queue, the
// tree state: nothing depends on anything), three block barriers, cross-lane traffic on the DPP path, the serial part on one wavefront
// without barriers.  Conditions (enqueue_growth_step): one GPU, default mode (no strict order, no feature sampling), at most 160 histogram
// features (five records per lane of a half wavefront), node records and queue in LDS (<= 62 leaves).
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int kSel2Threads = 64 * kSpec > 256 ? 64 * kSpec : 256;      // one wavefront per slot
constexpr int kSel2MaxF = 160;           // k_select2<false>: whole records in registers; up to 32 x kWideS features: k_select2<true>

struct HB { double s; int f; };
__device__ __forceinline__ HB hb_better(HB a, HB b)
{   // larger S; on equal S the lower feature index (>= 0)
    if (b.s > a.s || (b.s == a.s && b.f >= 0 && (a.f < 0 || b.f < a.f))) return b;
    return a;
}
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ HB dpp_hb(HB v)
{
    HB r;
    r.s = bits2d(dpp_u64<CTRL, ROWMASK>(d2bits(v.s), 0xbff0000000000000ull));
    r.f = (int)dpp_u32<CTRL, ROWMASK>((uint32_t)v.f, 0xffffffffu);
    return r;
}

// half_wave_best_feature's `small` path with the lane's records already in registers (kS .. kT: feature hl + 32 u, S = -1.0 beyond F) and the
// reductions on the DPP path.  Every lane of the wavefront calls; `valid` is uniform in the half.
__device__ __forceinline__ void half_best_small(const Ctx &c, bool valid, const unsigned long long (&kS)[5], const unsigned long long (&kH)[5],
                                                const unsigned long long (&kL)[5], const unsigned long long (&kT)[5],
                                                long long nthi, unsigned long long ntlo, int nctot,
                                                double &S, int &f, int &t, int &cl, long long &hi, unsigned long long &lo, int &tie)
{
    const int lane = lane_id(), hl = lane & 31, hbase = lane & 32;
    double bs = -1.0; int bf = -1;
    unsigned long long bhi = 0, blo = 0, btc = 0;
    bool eq = false;
    if (valid) {
#pragma unroll
        for (int u = 0; u < 5; u++) {
            const int i = hl + 32 * u;
            const double s = __longlong_as_double((long long)kS[u]);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs) { eq = false; bs = s; bf = i; bhi = kH[u]; blo = kL[u]; btc = kT[u]; }         // (ascending i: the first of equal gains stays)
        }
    }
    const int own = bf; const double own_s = bs;
    HB v; v.s = bs; v.f = bf;
    v = hb_better(v, dpp_hb<kDppShr1>(v)); v = hb_better(v, dpp_hb<kDppShr2>(v)); v = hb_better(v, dpp_hb<kDppShr4>(v)); v = hb_better(v, dpp_hb<kDppShr8>(v));
    v = hb_better(v, dpp_hb<kDppBcast15, 0xa>(v));         // lane 31 / lane 63: the half's best
    {
        const double s0 = readlane_f64(v.s, 31), s1 = readlane_f64(v.s, 63);
        const int f0 = (int)readlane_u32((uint32_t)v.f, 31), f1 = (int)readlane_u32((uint32_t)v.f, 63);
        bs = hbase ? s1 : s0; bf = hbase ? f1 : f0;
    }
    S = bs; f = bf; t = -1; cl = 0; hi = 0; lo = 0;
    // the winner is the own candidate of exactly one lane of the half
    const unsigned long long ownb = __ballot(bf >= 0 && own == bf);
    const int src0 = (int)__builtin_ctzll((ownb & 0xffffffffull) | (1ull << 63)) & 63, src1 = (int)__builtin_ctzll((ownb >> 32) | (1ull << 31)) + 32;
    const unsigned long long tc0 = readlane_u64(btc, src0), tc1 = readlane_u64(btc, min(src1, 63));
    const unsigned long long h0 = readlane_u64(bhi, src0), h1 = readlane_u64(bhi, min(src1, 63));
    const unsigned long long l0 = readlane_u64(blo, src0), l1 = readlane_u64(blo, min(src1, 63));
    const unsigned long long tc = hbase ? tc1 : tc0;
    const long long h2 = (long long)(hbase ? h1 : h0); const unsigned long long l2 = hbase ? l1 : l0;
    unsigned long long cross = __ballot(bf >= 0 && own >= 0 && own_s == bs && (own != bf || eq)) >> hbase;
    bool other_cut = false;
    if (c.tie_on) {       // mirrored cuts of other features: equal partition keys although the f64 S differ by a rounding
        bool mir = false;
        if (valid && bf >= 0) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
#pragma unroll
            for (int u = 0; u < 5; u++) {
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
        }
        cross |= __ballot(mir) >> hbase;
    }
    const bool any_other = ((__ballot(other_cut) >> hbase) & 0xffffffffull) != 0;
    tie = 0;
    if (bf >= 0) {
        t = (int)((tc >> 32) & 0xffffu); cl = (int)(unsigned)tc; hi = h2; lo = l2;
        tie = (cross & 0xffffffffull) ? (2 | (__builtin_popcountll(cross & 0xffffffffull) << 8)) : ((tc & kFbTieDiff) ? 2 : ((tc & kFbTie) ? 1 : 0));
        if ((cross & 0xffffffffull) && !any_other && !(tc & kFbTieDiff)) tie |= 4;
    }
}

// The same for data with hundreds of histogram features (up to 32 x kWideS = 768: the Yahoo-set1 shape): the lane's share is up to kWideS records, so only
// their GAINS are requested up front (wS: feature hl + 32 u, -1.0 beyond F); every lane then fetches the rest of its own best record (one more round
// trip, all lanes at once), and the tie pass reads the records of the near-equal gains -- rare -- from memory.  half_wave_best_feature<WIDE>'s logic
// (rl_k_best.inc) with the reductions on the DPP path.
__device__ __forceinline__ void half_best_wide(const Ctx &c, bool valid, const FeatBest *o, const unsigned long long (&wS)[kWideS],
                                               long long nthi, unsigned long long ntlo, int nctot,
                                               double &S, int &f, int &t, int &cl, long long &hi, unsigned long long &lo, int &tie)
{
    const int lane = lane_id(), hl = lane & 31, hbase = lane & 32;
    double bs = -1.0; int bf = -1;
    bool eq = false;
    if (valid) {
#pragma unroll
        for (int u = 0; u < kWideS; u++) {
            const int i = hl + 32 * u;
            const double s = __longlong_as_double((long long)wS[u]);
            if (s == bs && s > -1.0) eq = true;
            if (s > bs) { eq = false; bs = s; bf = i; }         // (ascending i: the first of equal gains stays)
        }
    }
    unsigned long long bhi = 0, blo = 0, btc = 0;
    if (bf >= 0) { bhi = o[bf].hi; blo = o[bf].lo; btc = o[bf].tc; }
    const int own = bf; const double own_s = bs;
    HB v; v.s = bs; v.f = bf;
    v = hb_better(v, dpp_hb<kDppShr1>(v)); v = hb_better(v, dpp_hb<kDppShr2>(v)); v = hb_better(v, dpp_hb<kDppShr4>(v)); v = hb_better(v, dpp_hb<kDppShr8>(v));
    v = hb_better(v, dpp_hb<kDppBcast15, 0xa>(v));         // lane 31 / lane 63: the half's best
    {
        const double s0 = readlane_f64(v.s, 31), s1 = readlane_f64(v.s, 63);
        const int f0 = (int)readlane_u32((uint32_t)v.f, 31), f1 = (int)readlane_u32((uint32_t)v.f, 63);
        bs = hbase ? s1 : s0; bf = hbase ? f1 : f0;
    }
    S = bs; f = bf; t = -1; cl = 0; hi = 0; lo = 0;
    const unsigned long long ownb = __ballot(bf >= 0 && own == bf);
    const int src0 = (int)__builtin_ctzll((ownb & 0xffffffffull) | (1ull << 63)) & 63, src1 = (int)__builtin_ctzll((ownb >> 32) | (1ull << 31)) + 32;
    const unsigned long long tc0 = readlane_u64(btc, src0), tc1 = readlane_u64(btc, min(src1, 63));
    const unsigned long long h0 = readlane_u64(bhi, src0), h1 = readlane_u64(bhi, min(src1, 63));
    const unsigned long long l0 = readlane_u64(blo, src0), l1 = readlane_u64(blo, min(src1, 63));
    const unsigned long long tc = hbase ? tc1 : tc0;
    const long long h2 = (long long)(hbase ? h1 : h0); const unsigned long long l2 = hbase ? l1 : l0;
    unsigned long long cross = __ballot(bf >= 0 && own >= 0 && own_s == bs && (own != bf || eq)) >> hbase;
    bool other_cut = false;
    if (c.tie_on) {       // mirrored cuts of other features: equal partition keys although the f64 S differ by a rounding
        bool mir = false;
        if (valid && bf >= 0) {
            const i128 ntot = make_i128(nthi, ntlo);
            const i128 wsl = make_i128(h2, l2);
            const PartKey wk = part_key((int)(unsigned)tc, wsl, nctot, ntot);
            unsigned near = 0u, exact = 0u;       // (registers cannot be indexed by a run-time u: the near-equal gains of the share as bit masks)
#pragma unroll
            for (int u = 0; u < kWideS; u++) {
                const double s = __longlong_as_double((long long)wS[u]);
                if (hl + 32 * u != bf && s > -1.0 && !(fabs(s - bs) > 1e-9 * fabs(bs))) { near |= 1u << u; if (s == bs) exact |= 1u << u; }
            }
            while (near) {
                const int u = __builtin_ctz(near);
                near &= near - 1u;
                const int i = hl + 32 * u;
                const unsigned long long itc = o[i].tc;
                const i128 isl = make_i128((long long)o[i].hi, o[i].lo);
                const PartKey k = part_key((int)(unsigned)itc, isl, nctot, ntot);
                const bool keq = (k.cnt == wk.cnt && k.sum == wk.sum);
                mir |= keq;
                if (keq || ((exact >> u) & 1u)) other_cut |= !((unsigned)itc == (unsigned)tc && isl == wsl) || (itc & kFbTieDiff) != 0;
            }
        }
        cross |= __ballot(mir) >> hbase;
    }
    const bool any_other = ((__ballot(other_cut) >> hbase) & 0xffffffffull) != 0;
    tie = 0;
    if (bf >= 0) {
        t = (int)((tc >> 32) & 0xffffu); cl = (int)(unsigned)tc; hi = h2; lo = l2;
        tie = (cross & 0xffffffffull) ? (2 | (__builtin_popcountll(cross & 0xffffffffull) << 8)) : ((tc & kFbTieDiff) ? 2 : ((tc & kFbTie) ? 1 : 0));
        if ((cross & 0xffffffffull) && !any_other && !(tc & kFbTieDiff)) tie |= 4;
    }
}

__host__ __device__ inline size_t select2_lds_bytes(int L, int NC)
{
    return sizeof(TreeState) + (size_t)NC * sizeof(NodeRec) + (size_t)(L + 2) * 4 + 64;
}

template <bool WIDE = false>
__global__ __launch_bounds__(kSel2Threads) void k_select2(const Ctx c)
{
    extern __shared__ unsigned long long sh_raw[];
    static_assert(kSpec <= kSel2Threads / 64, "one wavefront per slot");
    static_assert(sizeof(TreeState) % 8 == 0 && sizeof(NodeRec) % 8 == 0, "copied as 8-byte words");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef RL_PHASE_CLOCKS
    long long tk_[8]; tk_[0] = (long long)wall_clock64();
#define RL_S2_MARK(k) do { tk_[k] = strict_clock(); } while (0)
#else
#define RL_S2_MARK(k) do { } while (0)
#endif
    // ---- every load of the kernel, at once (the buffers are allocated to their capacities: nothing depends on the tree state)
    constexpr int kStW = (int)(sizeof(TreeState) / 8), kNodeW = (int)(sizeof(NodeRec) / 8);
    static_assert(kStW <= kSel2Threads, "tree state: one word per thread");
    const unsigned long long stw = ((const unsigned long long *)c.st)[min(tid, kStW - 1)];
    const int nwcap = c.NC * kNodeW;
    constexpr int kPre = 12;                 // 12 x 256 words = 24 KB of node records in flight; more are fetched by the loop below
    unsigned long long pre[kPre];
#pragma unroll
    for (int u = 0; u < kPre; u++) pre[u] = ((const unsigned long long *)c.nodes)[min(tid + u * kSel2Threads, nwcap - 1)];
    const int QC = c.L + 2;
    const int q_pre = c.queue[min(tid, QC - 1)];
    const unsigned long long sq_pre = c.fb_sq[min(tid, kSpec - 1)];
    [[maybe_unused]] unsigned long long kS[5], kH[5], kL[5], kT[5];
    [[maybe_unused]] unsigned long long wS[WIDE ? kWideS : 1];
    const FeatBest *fbo = c.fb + ((size_t)min(wave, kSpec - 1) * 2 + (lane >> 5)) * c.F;      // wavefront w: slot w; half: side
    if constexpr (WIDE) {
        const int hl = lane & 31;
#pragma unroll
        for (int u = 0; u < kWideS; u++) wS[u] = fbo[min(hl + 32 * u, c.F - 1)].S;
#pragma unroll
        for (int u = 0; u < kWideS; u++) if (hl + 32 * u >= c.F) wS[u] = 0xbff0000000000000ull;
    } else {
        const FeatBest *o = fbo;
        const int hl = lane & 31;
#pragma unroll
        for (int u = 0; u < 5; u++) { const FeatBest *r = o + min(hl + 32 * u, c.F - 1); kS[u] = r->S; kH[u] = r->hi; kL[u] = r->lo; kT[u] = r->tc; }
#pragma unroll
        for (int u = 0; u < 5; u++) if (hl + 32 * u >= c.F) { kS[u] = 0xbff0000000000000ull; kH[u] = kL[u] = kT[u] = 0ull; }
    }
    TreeState &st = *(TreeState *)sh_raw;
    NodeRec *N = (NodeRec *)((unsigned char *)sh_raw + sizeof(TreeState));
    int *q = (int *)((unsigned char *)N + (size_t)c.NC * sizeof(NodeRec));
    __shared__ double bS[2 * kSpec]; __shared__ int bf[2 * kSpec], bt[2 * kSpec], bcl[2 * kSpec], btie[2 * kSpec];
    __shared__ long long bhi[2 * kSpec]; __shared__ unsigned long long blo[2 * kSpec];
    __shared__ int sel[kSpec];
    if (tid < kStW) ((unsigned long long *)&st)[tid] = stw;
#pragma unroll
    for (int u = 0; u < kPre; u++) { const int i = tid + u * kSel2Threads; if (i < nwcap) ((unsigned long long *)N)[i] = pre[u]; }
    for (int i = tid + kPre * kSel2Threads; i < nwcap; i += kSel2Threads) ((unsigned long long *)N)[i] = ((const unsigned long long *)c.nodes)[i];
    if (tid < QC) q[tid] = q_pre;
    __syncthreads();
    if (st.done || st.nslots <= 0) return;          // a finished or stalled tree: the step is empty (uniform)
    RL_S2_MARK(1);
    const int E = st.E, E2 = st.E2;
    const int ns = st.nslots, qs0 = st.qsize, nn0 = st.n_nodes;
    // ---- A. best split per (slot, side): one half wavefront each
    {
        const int pi = 2 * wave + (lane >> 5);
        const bool valid = wave < ns && !st.slot[min(wave, kSpec - 1)].skip_hist;
        long long nthi = 0; unsigned long long ntlo = 0; int nctot = 0;
        if (c.tie_on && wave < ns) { const NodeRec &Ch = N[(pi & 1) ? st.slot[wave].right : st.slot[wave].left]; nthi = Ch.tot_hi; ntlo = Ch.tot_lo; nctot = Ch.gcount; }
        double S; int f, t, cl, tie; long long hi; unsigned long long lo;
        if constexpr (WIDE) half_best_wide(c, valid, fbo, wS, nthi, ntlo, nctot, S, f, t, cl, hi, lo, tie);
        else half_best_small(c, valid, kS, kH, kL, kT, nthi, ntlo, nctot, S, f, t, cl, hi, lo, tie);
        if ((lane & 31) == 0 && wave < ns) { bS[pi] = S; bf[pi] = f; bt[pi] = t; bcl[pi] = cl; bhi[pi] = hi; blo[pi] = lo; btie[pi] = tie; }
    }
    if (tid < ns) st.slot[tid].sq_left = (long long)sq_pre;
    __syncthreads();
    RL_S2_MARK(2);
    // ---- B, C, D on wavefront 0 (no block barriers: LDS operations of one wavefront execute in order)
    if (wave == 0) {
        if (lane < ns) {          // B. the children of the nodes prepared by the step that just ran
            const SlotRec &sl = st.slot[lane];
            NodeRec &P = N[sl.node]; NodeRec &Lc = N[sl.left]; NodeRec &Rc = N[sl.right];
            if (sl.build_left) { Lc.sq = sl.sq_left; Rc.sq = P.sq - Lc.sq; }       // sq_left: the BUILT child's sum (k_part_scatter)
            else { Rc.sq = sl.sq_left; Lc.sq = P.sq - Rc.sq; }
            Lc.sum_response = fixed_to_double(make_i128(Lc.tot_hi, Lc.tot_lo), E);
            Rc.sum_response = fixed_to_double(make_i128(Rc.tot_hi, Rc.tot_lo), E);
            Lc.sq_response = fixed_to_double((i128)Lc.sq, E2);
            Rc.sq_response = fixed_to_double((i128)Rc.sq, E2);
            Lc.deviance = variance_of(Lc.sq_response, Lc.sum_response, Lc.gcount);
            Rc.deviance = variance_of(Rc.sq_response, Rc.sum_response, Rc.gcount);
            if (!sl.skip_hist) {
                Lc.best_S = bS[2 * lane]; Lc.best_f = bf[2 * lane]; Lc.best_t = bt[2 * lane];
                Lc.best_cl = bcl[2 * lane]; Lc.best_hi = bhi[2 * lane]; Lc.best_lo = blo[2 * lane];
                Rc.best_S = bS[2 * lane + 1]; Rc.best_f = bf[2 * lane + 1]; Rc.best_t = bt[2 * lane + 1];
                Rc.best_cl = bcl[2 * lane + 1]; Rc.best_hi = bhi[2 * lane + 1]; Rc.best_lo = blo[2 * lane + 1];
                Lc.tie = btie[2 * lane]; Rc.tie = btie[2 * lane + 1];
            }       // (skip_hist: the split that fills the leaf budget -- its children are leaves whatever their histograms would say; best_S stays -1)
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        RL_S2_MARK(3);
        // C. RegressionTree.fit's loop (:70-85) on one wavefront: lane p holds queue entry p
        int qn = (lane < qs0) ? q[lane] : -1;
        double qdv = 0.0; bool cs = false, prep = false;
        if (qn >= 0) { const NodeRec &X = N[qn]; qdv = X.deviance; cs = can_split(c, X); prep = X.prepared != 0; }
        int qsize = qs0, taken = st.taken, n_splits = st.n_splits, ncommit = 0;
        unsigned long long gd2 = 0, gd3 = 0;
        const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        auto insert = [&](int node, double d, bool ncs) {          // RegressionTree.insert (:147-157)
            const int pos = __builtin_popcountll(__ballot(lane < qsize && qdv > d));
            const int un = (int)dpp_u32<0x138>((uint32_t)qn); const double ud = bits2d(dpp_u64<0x138>(d2bits(qdv)));       // wave_shr:1
            const int ucp = (int)dpp_u32<0x138>((uint32_t)((cs ? 1 : 0) | (prep ? 2 : 0)));
            if (lane > pos) { qn = un; qdv = ud; cs = (ucp & 1) != 0; prep = (ucp & 2) != 0; }
            else if (lane == pos) { qn = node; qdv = d; cs = ncs; prep = false; }
            qsize++;
        };
        auto pop = [&]() {
            qn = (int)dpp_u32<0x130>((uint32_t)qn); qdv = bits2d(dpp_u64<0x130>(d2bits(qdv)));                              // wave_shl:1
            const int ucp = (int)dpp_u32<0x130>((uint32_t)((cs ? 1 : 0) | (prep ? 2 : 0)));
            cs = (ucp & 1) != 0; prep = (ucp & 2) != 0;
            qsize--;
        };
        auto commit = [&](int p) {       // a split becomes part of the tree: sp.set(.., var) (:352), children enter the queue (:66-67, :82-83)
            NodeRec &X = N[p];
            const int l = X.pl, r = X.pr;
            const int child = (lane == 0) ? l : r;
            double dch = 0.0; int cch = 0;
            if (lane < 2) { dch = N[child].deviance; cch = can_split(c, N[child]) ? 1 : 0; }
            const double dl = readlane_f64(dch, 0), dr = readlane_f64(dch, 1);
            const int csl = (int)readlane_u32((uint32_t)cch, 0), csr = (int)readlane_u32((uint32_t)cch, 1);
            if (lane == 0) {
                X.left = l; X.right = r;
                X.deviance = variance_of(X.sq_response, X.sum_response, X.gcount);
                N[l].fid = 2 * n_splits + 1; N[r].fid = 2 * n_splits + 2;
                gd2 += (unsigned long long)N[l].gcount; gd3 += (unsigned long long)X.gcount;       // (folded into c.grow_docs once, below: a read-modify-write of global memory per commit was a dependent round trip inside the loop)
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
            const int leaf = (int)readlane_u32((uint32_t)qn, 0);
            const int cp0 = (int)readlane_u32((uint32_t)((cs ? 1 : 0) | (prep ? 2 : 0)), 0);
            if (!(cp0 & 1)) { pop(); taken++; continue; }
            if (cp0 & 2) { pop(); commit(leaf); continue; }
            done = false;
            break;
        }
        RL_S2_MARK(4);
        // next step: the first kSpec unprepared nodes in queue order that the leaf budget can still reach
        int nsel = 0, err = 0, budget = 0;
        if (!done) {
            budget = c.L - (taken + qsize);                         // splits left (>= 1)
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
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        int nstall = 0;
        if (c.tie_on && lane == 0) nstall = stalled_nodes(N, sel, nsel, st.stall_node, &st.defer_any, (c.tie_on & 2) != 0);
        nstall = (int)readlane_u32((uint32_t)nstall, 0);
        if (nstall > 0) nsel = 0;                 // nothing is partitioned until the host has resolved the ties (rl_tie.inc)
        if (lane < qsize) c.queue[lane] = qn;
        if (lane == 0) {
            st.stall_n = nstall;
            st.done = done ? 1 : 0; if (err && !st.error) st.error = 1;
            if (done) c.grow_docs[8] = wall_clock64();       // (RL_ARR_BUBBLES: the tree ends here; k_leaf_table looks at its clock on entry)
            st.nslots = nsel; st.qsize = qsize; st.taken = taken; st.n_splits = n_splits;
            if (ncommit) { atomicAdd(&c.grow_stats[2], ncommit); atomicAdd(&c.grow_docs[2], gd2); atomicAdd(&c.grow_docs[3], gd3); }
            if (nsel > 0) { atomicAdd(&c.grow_stats[0], 1); atomicAdd(&c.grow_stats[1], nsel); }
        }
        // D. children records of the selected nodes (one lane per slot), chunk / tile ranges
        if (lane < nsel) {
            prepare_children(c, N, sel[lane], nn0 + 2 * lane, st.slot[lane]);
            st.slot[lane].skip_hist = 0;
            if (c.steplog) {        // debug: what every growth step works on
                const int e = atomicAdd(&c.steplog[0], 1);
                if (e < kStepLogCap) {
                    int *o = c.steplog + 8 + 8 * e; const NodeRec &P = N[sel[lane]];
                    o[0] = st.tree_seq; o[1] = 0; o[2] = st.step + 1; o[3] = lane; o[4] = P.gcount; o[5] = st.slot[lane].build_left ? P.best_cl : P.gcount - P.best_cl; o[6] = P.tie; o[7] = nsel;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            // The split that fills the leaf budget: its children are leaves whatever their histograms would say (RegressionTree.java:70: the loop
            // ends with this commit), so the step partitions the node and neither accumulates nor finishes a child histogram.
            if (nsel == 1 && budget == 1 && c.skip_last) {
                SlotRec &s0 = st.slot[0];
                s0.skip_hist = 1; s0.nchunks = 0;
                atomicAdd(&c.grow_docs[0], (unsigned long long)(-(long long)(s0.build_left ? s0.nleft : s0.pcount - s0.nleft)));
            }
            int tiles = 0, chunks = 0;
            if (!(nsel == 1 && st.slot[0].skip_hist)) balance_slots(c, st.slot, nsel);
            for (int j = 0; j < nsel; j++) {
                st.slot[j].tile0 = tiles; tiles += st.slot[j].ntiles;
                st.slot[j].chunk0 = chunks; chunks += st.slot[j].nchunks;
            }
            st.tiles_total = tiles; st.chunks_total = chunks;
            st.n_nodes = nn0 + 2 * nsel;
            st.arrive = 0; st.epoch++;
#ifdef RL_PHASE_CLOCKS
            if (st.tree_seq == c.trace_tree) {
                long long *o_ = c.clk + (st.step & 63) * 32;
                const long long t5_ = strict_clock();
                o_[20] = tk_[0]; o_[21] = tk_[1]; o_[22] = tk_[2]; o_[23] = tk_[3]; o_[24] = tk_[4]; o_[25] = t5_; o_[28] = t5_;       // 28: end of this step's bookkeeping (tools/step_trace.py)
            }
#endif
            st.step++;
        }
    }
    __syncthreads();
    // ---- write back: node records (the prepared children included), tree state, the host's progress word
    {
        const int nw = st.n_nodes * kNodeW;
        for (int i = tid; i < nw; i += kSel2Threads) ((unsigned long long *)c.nodes)[i] = ((const unsigned long long *)N)[i];
        if (tid < kStW) ((unsigned long long *)c.st)[tid] = ((const unsigned long long *)&st)[tid];
        if (tid == 0 && c.progress)
            __hip_atomic_store(c.progress, ((unsigned long long)(unsigned)st.tree_seq << 32) | (st.stall_n > 0 ? (1ull << 31) : 0ull) | (st.defer_any ? (1ull << 30) : 0ull) |
                                               ((unsigned long long)((unsigned)st.step & 0x1fffffffu) << 1) | (st.done ? 1ull : 0ull),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace rl
