// rl_k_reduce.inc -- K4/K5, first part: what the finish shares with the sharded reduction.  Best and block_best2, gain_S, rebuild_mode_bin,
// and k_hist_reduce (a rank's bin totals as limbs for the all-reduce).  Included by rl_kernels_round.inc; needs that file's i128 helpers
// and rl_k_hist.inc (chunk_docs, slot_sq_left).

namespace rl {

// ------------------------------------------------------------------------------------------------
// K4/K5: one block per feature.
//   * sum the chunk partials of the (left) node into exact 128-bit bin totals
//   * inclusive prefix over threshold index -> cumulative sum / count   (FeatureHistogram.java:141-145,189-194)
//   * right sibling = parent - left                                     (FeatureHistogram.java:222-234)
//   * gain scan S = sl^2/cl + sr^2/cr per child, first maximum wins     (FeatureHistogram.java:236-264)
// LDS: TS x (hi, lo, cnt).
// ------------------------------------------------------------------------------------------------
constexpr int kParCacheTS = 1024;     // hist_finish_body keeps the parent's cumulative entries in LDS up to this many bins per feature
struct Best { double S; int t; };
__device__ __forceinline__ Best better(Best a, Best b)
{   // larger S wins; on equal S the lower threshold index (the one the Java loop meets first)
    if (b.S > a.S || (b.S == a.S && b.t >= 0 && (a.t < 0 || b.t < a.t))) return b;
    return a;
}

// block-wide best of two candidates at once (built child, sibling): one pair of barriers for both
__device__ void block_best2(Best &a, Best &b, Best *sh /* [2 * kFinThreads / 64] */, int nw_ = 0)
{
    for (int o = 32; o > 0; o >>= 1) {
        Best u; u.S = __shfl_xor(a.S, o); u.t = __shfl_xor(a.t, o);
        a = better(a, u);
        Best w; w.S = __shfl_xor(b.S, o); w.t = __shfl_xor(b.t, o);
        b = better(b, w);
    }
    const int NW = nw_ ? nw_ : (int)(blockDim.x >> 6);          // (the finish kernels run with 320 threads, or 192 on wide data: k_hist_finish_wide; blockDim.x is a load)
    __syncthreads();
    if (lane_id() == 0) { sh[threadIdx.x >> 6] = a; sh[NW + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    a = sh[0]; b = sh[NW];
    for (int i = 1; i < NW; i++) { a = better(a, sh[i]); b = better(b, sh[NW + i]); }
}

__device__ __forceinline__ double gain_S(double sl, int cl, double total, int ctot, int mls, bool &ok)
{
    const int cr = ctot - cl;
    ok = !(cl < mls || cr < mls);
    if (!ok) return -1.0;
    const double sr = total - sl;                                    // FeatureHistogram.java:251
    return sl * sl / cl + sr * sr / cr;                              // :253
}


// The mode bin was skipped by k_hist: bin[mode] = (sum over the node's samples) - (sum of the other bins), exact in
// fixed point.  s_hi/s_lo/s_cnt hold the per-bin totals (mode bin = 0); every thread calls this.
// have_pre: the caller has requested the thread's first chunk total (chunk ch0 + threadIdx.x) and the feature's mode bin already, together with its
// other loads (each was a dependent memory round trip in the middle of every finish block)
__device__ void rebuild_mode_bin(const Ctx &c, int f, int T, int ch0, int nch, int cnt_local, bool with_counts, long long *s_hi,
                                 unsigned long long *s_lo, int *s_cnt, i128 *sh_red /* kFinThreads/64 */, int *sh_redc,
                                 bool have_pre = false, long long tot_pre = 0, int mode_pre = 0)
{
    i128 part = 0; int cpart = 0;
    for (int t = threadIdx.x; t < T; t += (int)blockDim.x) { part += make_i128(s_hi[t], s_lo[t]); cpart += s_cnt[t]; }
    for (int ch = threadIdx.x; ch < nch; ch += (int)blockDim.x)
        part -= (i128)((have_pre && ch == (int)threadIdx.x) ? tot_pre : c.part_tot[ch0 + ch]);      // others - total
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t w0 = (uint32_t)(u128)part, w1 = (uint32_t)((u128)part >> 32), w2 = (uint32_t)((u128)part >> 64), w3 = (uint32_t)((u128)part >> 96);
        w0 = __shfl_xor(w0, o); w1 = __shfl_xor(w1, o); w2 = __shfl_xor(w2, o); w3 = __shfl_xor(w3, o);
        part += (i128)(((u128)w3 << 96) | ((u128)w2 << 64) | ((u128)w1 << 32) | (u128)w0);
        cpart += __shfl_xor(cpart, o);
    }
    if (lane_id() == 0) { sh_red[threadIdx.x >> 6] = part; sh_redc[threadIdx.x >> 6] = cpart; }
    __syncthreads();
    if (threadIdx.x == 0) {
        i128 others_minus_total = 0; int oc = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); i++) { others_minus_total += sh_red[i]; oc += sh_redc[i]; }
        const int m = have_pre ? mode_pre : c.mode[f];
        const i128 v = -others_minus_total;
        s_hi[m] = hi_of(v); s_lo[m] = lo_of(v);
        if (with_counts) s_cnt[m] = cnt_local - oc;
    }
    __syncthreads();
}

// multi-GPU: bin totals of the accumulated node as int64 limbs (a = v >> 44, b = v & (2^44-1), count) so that a plain
// int64 sum all-reduce of the limbs is exact; tail = the per-split scalars that travel with it
constexpr int kLimbShift = 44;
__global__ __launch_bounds__(kFinThreads) void k_hist_reduce(const Ctx c, int is_root)
{   // grid (F, slots)
    extern __shared__ unsigned long long sh_raw[];
    __shared__ i128 sh_red[kFinThreads / 64];
    __shared__ int sh_redc[kFinThreads / 64];
    const TreeState *st = c.st;
    const int slot = blockIdx.y;
    int nodeB = 0, ch0 = 0, nodeS = 0, nodeP = 0, sl_cs = 0, sl_cnt = -1;
    const bool active = is_root || (!st->done && slot < st->nslots);
    if (!is_root && active) {
        const SlotRec &sl = st->slot[slot];
        nodeB = sl.build_left ? sl.left : sl.right; nodeS = sl.build_left ? sl.right : sl.left; nodeP = sl.node; ch0 = sl.chunk0; sl_cs = sl.cs;
        if (sl.nleft >= 0) sl_cnt = sl.build_left ? sl.nleft : sl.pcount - sl.nleft;
    }
    const int f = blockIdx.x;
    const int TS = c.TS, T = c.nthr[f];
    long long *s_hi = (long long *)sh_raw;
    unsigned long long *s_lo = sh_raw + TS;
    int *s_cnt = (int *)(sh_raw + 2 * TS);
    const int cntB = is_root ? c.N : (active ? (sl_cnt >= 0 ? sl_cnt : c.nodes[nodeB].count) : 0);
    const int csB = is_root ? chunk_docs<true>(c, cntB) : (sl_cs > 0 ? sl_cs : chunk_docs<false>(c, cntB));      // (balance_slots)
    const int nch = (cntB + csB - 1) / csB;
    const int W = c.limb_words;
    const size_t slot_words = (size_t)c.F * TS * W + 4;
    long long *out = c.dist_buf + slot * slot_words + (size_t)f * TS * W;
    for (int t = threadIdx.x; t < T; t += kFinThreads) {
        i128 acc = 0; int cacc = 0;
        // (batches of eight chunk partials in flight, as in hist_finish_body: one at a time every chunk was a memory round trip)
        constexpr int kRedBatch = 8;
        const size_t cstride = (size_t)c.F * TS;
        const long long *ps = c.part_sum + ((size_t)ch0 * c.F + f) * TS + t;
        const int *pc = c.part_cnt + ((size_t)ch0 * c.F + f) * TS + t;
        unsigned long long lo = 0; long long hi = 0;
        for (int ch = 0; ch < nch; ch += kRedBatch) {
            long long v[kRedBatch]; int cn[kRedBatch];
#pragma unroll
            for (int u = 0; u < kRedBatch; u++) { const size_t o = (size_t)min(ch + u, nch - 1) * cstride; v[u] = ps[o]; cn[u] = is_root ? 0 : pc[o]; }
#pragma unroll
            for (int u = 0; u < kRedBatch; u++)
                if (ch + u < nch) { lo += (unsigned long long)(unsigned)v[u]; hi += (v[u] >> 32); cacc += cn[u]; }
        }
        acc += (i128)lo + (((i128)hi) << 32);
        s_hi[t] = hi_of(acc); s_lo[t] = lo_of(acc); s_cnt[t] = cacc;
    }
    __syncthreads();
    rebuild_mode_bin(c, f, T, ch0, nch, cntB, !is_root, s_hi, s_lo, s_cnt, sh_red, sh_redc);
    if (!is_root && active && c.cum_cnt_loc) {
        // this rank's cumulative counts of the built child and (parent - built) of its sibling: what tells the next partition of either node its
        // local left size (prepare_children)
        __syncthreads();
        __shared__ int sh_wc[kFinThreads / 64];
        int32_t *cb = c.cum_cnt_loc + ((size_t)nodeB * c.F + f) * TS, *cs_ = c.cum_cnt_loc + ((size_t)nodeS * c.F + f) * TS;
        const int32_t *cp = c.cum_cnt_loc + ((size_t)nodeP * c.F + f) * TS;
        int carry = 0;
        for (int t0 = 0; t0 < T; t0 += kFinThreads) {
            const int t = t0 + (int)threadIdx.x;
            const int v = t < T ? s_cnt[t] : 0, pv = t < T ? cp[t] : 0;
            const int inc = (int)wave_scan_u32((unsigned)v);
            if (lane_id() == 63) sh_wc[threadIdx.x >> 6] = inc;
            __syncthreads();
            int off = carry, all = 0;
#pragma unroll
            for (int w = 0; w < kFinThreads / 64; w++) { if (w < (int)(threadIdx.x >> 6)) off += sh_wc[w]; all += sh_wc[w]; }
            if (t < T) { cb[t] = off + inc; cs_[t] = pv - (off + inc); }
            carry += all;
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < T; t += kFinThreads) {
        const i128 acc = make_i128(s_hi[t], s_lo[t]);
        const long long hi = (long long)(acc >> kLimbShift), lo = (long long)(acc & ((((i128)1) << kLimbShift) - 1));
        const long long cn = is_root ? 0 : (long long)s_cnt[t];
        if (W == 3) { out[3 * t] = hi; out[3 * t + 1] = lo; out[3 * t + 2] = cn; }
        else { out[2 * t] = hi * 4294967296ll + cn; out[2 * t + 1] = lo; }       // |hi| < 2^30 and the global count < 2^31 (checked at init)
    }
    if (f == 0) {
        __shared__ long long sh_sq[kFinThreads / 64];
        const long long sqv = is_root ? st->root_sq : (active ? slot_sq_left(c, st->slot[slot], sh_sq) : 0);
        if (threadIdx.x == 0) c.dist_buf[slot * slot_words + (size_t)c.F * TS * W] = sqv;
    }
}

}  // namespace rl
