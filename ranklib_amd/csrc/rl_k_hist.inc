// rl_k_hist.inc -- K2/K3: the LDS-staged per-chunk histograms of a node (FeatureHistogram.java:126-146,166-195).  chunk_docs, bin8_of / pbin8_of,
// slot_sq_left, slot_of_chunk / slot_of_tile (the growth step's pieces use these as well), hist_chunk and k_hist, whose instantiations
// launch_hist (rl_launch.inc) chooses among.
// Included by rl_kernels_round.inc; needs that file's trace block ahead of the include (RL_TR_*) and rl_k_quant.inc (quant_exponents, rint_ll_small).

namespace rl {

// ------------------------------------------------------------------------------------------------
// K2/K3: histogram of one node.  grid = (feature groups, chunks).  A block owns FG features x one chunk of
// <= kChunk samples and accumulates them in LDS with native ds_add_u64 / ds_add_u32, then flushes its
// partial histogram (plain coalesced stores, no global atomics).  ROOT: samples are 0..N-1 and counts are
// static (FeatureHistogram.java:138 "count doesn't change").
// ------------------------------------------------------------------------------------------------
// docs per chunk for a node of `cnt` samples: big nodes use the largest chunk (least flush traffic), small
// nodes are cut finer so that a split step still spreads over the whole chip (a chunk's samples are
// processed serially by one block).  Must be identical in k_hist and k_hist_finish.
template <bool ROOT>
__device__ __forceinline__ int chunk_docs(const Ctx &c, int cnt)
{
    // a node is cut into ~node_div chunks (64 for the root pass): every chunk costs a partial histogram (F x T x 12 bytes)
    // that is flushed and read back, which outweighs the extra parallelism of finer cuts (measured at c2, same box: 64 -> 225.8, 12 -> 230.6, 8 -> 229.5, 6 -> 229.4 rounds/s)
    const int div = ROOT ? 64 : c.node_div;
    const int cs = ((cnt + div - 1) / div + 255) & ~255;
    return min(ROOT ? kChunk : c.node_chunk, max(ROOT ? kMinChunk : max(c.node_min, 256), cs));     // never 0: callers divide by it, also for empty (cnt == 0) slots
}

// gbins holds PRE-SCALED bin ids: 8 * bin = the byte offset of the bin's int64 accumulator inside its feature's LDS row.
__device__ __forceinline__ unsigned bin8_of(const uint4 &a, const uint4 &b, int fl)
{
    const unsigned w = fl < 8 ? (fl < 4 ? (fl < 2 ? a.x : a.y) : (fl < 6 ? a.z : a.w))
                              : (fl < 12 ? (fl < 10 ? b.x : b.y) : (fl < 14 ? b.z : b.w));
    return (fl & 1) ? (w >> 16) : (w & 0xffffu);
}

// Packed rows (P8; threshold tables of at most 257 entries, the -tc 256 case): a bin id is one byte plus, for the single bin that does not fit
// (bin 256: values above the last finite threshold), one bit of a 16-bit mask per (document, group): bin = byte + bit.  A (document, group)
// row is 16 + 2 bytes instead of 32: the root pass streams 170 instead of 296 bytes per document, a child's document-major row is 192 bytes
// -- two 128-byte memory lines -- instead of 384.
__device__ __forceinline__ unsigned pbin8_of(const uint4 &lo, unsigned hi, int fl)
{
    const unsigned w = fl < 8 ? (fl < 4 ? lo.x : lo.y) : (fl < 12 ? lo.z : lo.w);
    const unsigned byte = __builtin_amdgcn_ubfe(w, 8 * (fl & 3), 8), bit = __builtin_amdgcn_ubfe(hi, fl, 1);
    return (byte + bit) << 3;
}

// sum of the per-tile lambda^2 partials of a slot (exact integers: any order); every thread of the block calls it
__device__ long long slot_sq_left(const Ctx &c, const SlotRec &sl, long long *sh /* kThreads/64 */)
{
    long long v = 0;
    for (int i = threadIdx.x; i < sl.ntiles; i += blockDim.x) v += c.tile_sq[sl.tile0 + i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) r += sh[w];
    return r;
}

// slot of the growth step that owns global tile / chunk id `x` (ranges are consecutive); -1 = none.  Every start is loaded before any is looked at
// (a loop that loads the next start only after comparing the previous one is a chain of dependent memory round trips at the top of every block).
__device__ __forceinline__ int slot_of_chunk(const TreeState *st, int y)
{
    const int done = st->done, total = st->chunks_total, ns = st->nslots;
    int c0[kSpec];
#pragma unroll
    for (int i = 0; i < kSpec; i++) c0[i] = st->slot[i].chunk0;
    if (done || y >= total) return -1;
    int j = 0;
#pragma unroll
    for (int i = 1; i < kSpec; i++) j += (i < ns && y >= c0[i]) ? 1 : 0;
    return j;
}
__device__ __forceinline__ int slot_of_tile(const TreeState *st, int x)
{
    const int done = st->done, total = st->tiles_total, ns = st->nslots;
    int t0[kSpec];
#pragma unroll
    for (int i = 0; i < kSpec; i++) t0[i] = st->slot[i].tile0;
    if (done || x >= total) return -1;
    int j = 0;
#pragma unroll
    for (int i = 1; i < kSpec; i++) j += (i < ns && x >= t0[i]) ? 1 : 0;
    return j;
}

// grid = (feature groups x sub-passes, chunks).  A block owns SUB features of one group x one chunk of samples.
// Per sample it reads ONE 32-byte row gbins[group][k][0..15] (two 16-byte loads: full sectors for the sparse
// sample lists of child nodes, perfectly coalesced for the root) and the fixed-point lambda from the
// list-ordered copy ql (contiguous), then issues SUB ds_add_u64 (+ SUB ds_add_u32 on the counts of child nodes).
// The inner loop is kept to extract / compare-with-mode / LDS add per feature: bin ids arrive pre-scaled, padding
// features (their bins are 0 and their "mode" is 0) need no test, and with the usual <= 264 bins the LDS row stride is a
// compile-time constant (TSC), so every accumulator address is the extracted value plus an immediate offset.
// RUNS: the instantiation for data sets with columns that come in runs of equal bins (Ctx::runs; query-level features: the wavefront's 64
// consecutive samples share a bin, and 64 atomics on one LDS address serialise at ~5 cycles a lane).  Those columns leave the main loop and
// get a pass of their own in which the four samples of a quad that agree are folded into one atomic by DPP quad permutes (no LDS traffic).
// A separate instantiation because the larger loop body slows the ordinary columns down as well (HISTORY.md 4.1).
// NT: threads per block.  Child passes of few chunks leave most of the chip idle and are bound by the latency of the row gathers: a block of NT = 1024
// threads keeps four times as many gathers in flight per chunk (launch_hist picks NT; RLHIP_HIST_NT).
template <bool ROOT, int SUB, int TSC, bool RUNS, bool P8, int NT, bool CR, bool FQ>
__device__ __forceinline__ void hist_chunk(const Ctx &c, const TreeState *st, const int bx, const int by, unsigned long long *lsum)
{
    RL_TR_BEGIN();
    int node = 0, ychunk = by;
    int s_start = -1, s_count = 0, s_buf = 0, s_cs = 0;             // the accumulated child's list range straight from the slot (one GPU: its size is known)
    if (!ROOT) {
        const int j = slot_of_chunk(st, by);
        if (j < 0) return;
        const SlotRec sl = st->slot[j];                             // (copied whole: one batch of loads)
        node = sl.build_left ? sl.left : sl.right;                  // the smaller child (exact sums: order-free)
        ychunk = by - sl.chunk0; s_cs = sl.cs;
        if (sl.nleft >= 0) {        // saves the dependent load of the node record (written by the partition kernel with these very values)
            s_start = sl.build_left ? sl.pstart : sl.pstart + sl.nleft;
            s_count = sl.build_left ? sl.nleft : sl.pcount - sl.nleft;
            s_buf = 1 - sl.pbuf;
        }
    }
    NodeRec nd_s; nd_s.start = s_start; nd_s.count = s_count; nd_s.buf = s_buf;
    const NodeRec &nd = (ROOT || s_start < 0) ? c.nodes[node] : nd_s;
    const int cnt = ROOT ? c.N : nd.count;
    const int cs = (!ROOT && s_cs > 0) ? s_cs : chunk_docs<ROOT>(c, cnt);      // (balance_slots)
    const int p0 = ychunk * cs;
    if (p0 >= cnt) return;
    const int p1 = min(p0 + cs, cnt);
    const int TS = c.TS;
    const int LT = TSC ? TSC : TS;                  // LDS row stride (bins)
    constexpr int NSUB = kHistFG / SUB;
    const int grp = bx / NSUB, sp = bx % NSUB;
    const int fl0 = sp * SUB;                       // first feature of the group handled here
    const int f0 = grp * kHistFG + fl0;
    const int nf = min(SUB, c.F - f0);
    if (nf <= 0) return;
    const bool want_tot = (bx == 0);
    // root pass: the groups of sparse columns are accumulated from their entry lists by k_hist_sp (rl_csc.inc); block 0 still sums the
    // chunk's lambdas here (every column's mode bin is rebuilt from the chunk totals)
    const bool no_rows = ROOT && c.sp_on && c.sp_grp[grp];
    if (no_rows && !want_tot) return;
    unsigned char *lsum_b = (unsigned char *)lsum;
    unsigned char *lcnt_b = lsum_b + (size_t)SUB * LT * 8;         // one 32-bit count per bin (child nodes only)
    RL_TR_MARK(1);
    const int *idx = ROOT ? nullptr : c.idx[nd.buf] + nd.start;
    const long long *ql = ROOT ? c.q : c.ql[nd.buf] + nd.start;
    // rows of this feature group: group-major (dense passes: every byte of a memory line is used) or document-major (sparse nodes)
    const bool dm = ROOT ? (c.dm_root != 0) : (c.dm_div > 0 && (long long)cnt * c.dm_div <= (long long)c.N);
    const uint4 *rows = dm ? (const uint4 *)c.dbins + 2 * grp : (const uint4 *)(c.gbins + (size_t)grp * c.Npad * kHistFG);
    const size_t rstride = dm ? (size_t)2 * c.dm_gstride : (size_t)2;
    // packed rows: low bytes and the 16-bit mask of the group, document-major (one row per document) or group-major
    const unsigned char *plo = nullptr, *phi = nullptr; size_t plo_stride = 0, phi_stride = 0;
    if (P8) {
        if (dm) { plo = c.pdbins + 16 * grp; phi = c.pdbins + 16 * c.numFG + 2 * grp; plo_stride = phi_stride = (size_t)c.pd_stride; }
        else { plo = c.pbins + (size_t)grp * c.Npad * 16; phi = (const unsigned char *)c.phib + (size_t)grp * c.Npad * 2; plo_stride = 16; phi_stride = 2; }
    }
    // The most populated bin of a feature (zero for count-like features) is never accumulated: it would serialise
    // most lanes of a wavefront on one LDS address.  It is rebuilt exactly as (chunk total - other bins) downstream.
    // (one coalesced load by the first SUB lanes and a read-lane per feature: SUB loads of one word each were SUB dependent round trips)
    unsigned md8[SUB];
    {
        const int lj = lane_id();
        const unsigned mv = (lj < nf) ? 8u * (unsigned)c.mode[f0 + lj] : 0u;
#pragma unroll
        for (int j = 0; j < SUB; j++) md8[j] = (unsigned)__builtin_amdgcn_readlane((int)mv, j);
    }
    long long tot = 0;
    // FQ (root pass of the plain one-GPU path): the fixed-point lambdas are made HERE from the f64 lambdas -- k_quantize's pass over the documents
    // (a launch of ~38 us at c2) is gone; the blocks of feature group 0 store q / r for the child passes and sum r for the root's deviance.
    int qE = 0, qE2 = 0; long long sq_acc = 0;
    if (FQ) quant_exponents(st->maxabs_bits, c.Nglobal, qE, qE2);
    // (the extra stores are spread: group 0 stores q, group 1 -- when there is one -- r and its sum; a block that did both set the launch's tail)
    const bool fq_q = FQ && bx == 0, fq_r = FQ && bx == ((int)gridDim.x > 1 ? 1 : 0);
    constexpr int D = kHistDocs;
    const unsigned runmask = RUNS ? ((c.runs[grp] >> fl0) & ((1u << SUB) - 1u)) : 0u;      // block-uniform
    if (no_rows) {       // totals only
        for (int p = p0 + threadIdx.x; p < p1; p += NT) tot += ql[p];
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
        __shared__ long long wtot0[NT / 64];
        if (lane_id() == 0) wtot0[threadIdx.x >> 6] = tot;
        __syncthreads();
        if (threadIdx.x == 0) { long long v = 0; for (int w = 0; w < NT / 64; w++) v += wtot0[w]; c.part_tot[by] = v; }
        return;
    }
    const bool cr = CR && c.cr_grp[grp] != 0;         // block-uniform: this group's rows are compact
    int kn[D];
#pragma unroll
    for (int d = 0; d < D; d++) { const int p = p0 + threadIdx.x + d * NT; kn[d] = (p < p1) ? (ROOT ? p : idx[p]) : -1; }
    // (the LDS histogram is zeroed AFTER the first sample ids -- and the mode bins -- have been requested: behind the barrier their round trip was
    // serial set-up time of every chunk, ~1.8 us of a small child's 10-20 us block)
    for (int i = threadIdx.x; i < SUB * LT; i += NT) lsum[i] = 0;
    if (!ROOT) for (int i = threadIdx.x; i < SUB * LT; i += NT) ((unsigned *)lcnt_b)[i] = 0;
    __syncthreads();
    RL_TR_MARK(2);
    RL_TR_MARK(3);
    // One iteration's inputs (sample ids, fixed-point lambdas, bin rows) and its LDS atomics are two stages.  The root pass runs them back to back
    // (a perfectly coalesced stream, bound by the atomics).  Child passes request the rows of iteration i + 1 BEFORE the atomics of iteration i:
    // a row gather through a sample list is a ~2-us round trip, and with two blocks (eight wavefronts) on a CU -- one, in the small steps of a
    // late tree -- nothing else hides it: an iteration of 512 documents took 3.5 us for 1.3 us of LDS work.
    struct Stage { int k[D]; unsigned long long qv[D]; uint4 ra[D], rb[D]; unsigned hb[D]; };
    auto stage_load = [&](const int pb, const int (&kin)[D], Stage &S) {
        int (&k)[D] = S.k; unsigned long long (&qv)[D] = S.qv; uint4 (&ra)[D] = S.ra; uint4 (&rb)[D] = S.rb; unsigned (&hb)[D] = S.hb;
#pragma unroll
        for (int d = 0; d < D; d++) {
            k[d] = kin[d];
            const int p = pb + d * NT;
            if (FQ) {       // (ROOT: k == p; clamped, unconditional load)
                const double l = c.lw[min(p, p1 - 1)].x;
                const long long qq = rint_ll_small(ldexp(l, qE));
                qv[d] = (k[d] >= 0) ? (unsigned long long)qq : 0ull;
                if (fq_q && k[d] >= 0) c.q[p] = qq;
                if (fq_r && k[d] >= 0) {
                    const long long r = __double2ll_rn(ldexp(l * l, qE2));      // (r < 2^(61 - lg N): beyond the one-addition conversion on small data)
                    c.r[p] = r; sq_acc += r;
                }
            } else qv[d] = (k[d] >= 0) ? (unsigned long long)ql[p] : 0ull;
            tot += (long long)qv[d];
            const size_t kk = (size_t)max(k[d], 0);
            // (rb is the dense rows' second half only: a copy `rb = ra` here made the wavefront wait for document d's row before it asked for document d + 1's)
            if (CR && cr) { ra[d] = c.crows[(size_t)c.cr_stride * kk + grp]; rb[d] = make_uint4(0u, 0u, 0u, 0u); hb[d] = 0u; }      // compact row: one 16-byte request per (document, group)
            else if (P8) { ra[d] = *(const uint4 *)(plo + plo_stride * kk); hb[d] = *(const unsigned short *)(phi + phi_stride * kk); rb[d] = make_uint4(0u, 0u, 0u, 0u); }
            else { ra[d] = rows[rstride * kk]; rb[d] = rows[rstride * kk + 1]; hb[d] = 0u; }
        }
    };
    auto stage_acc = [&](const Stage &S) {
        const int (&k)[D] = S.k; const unsigned long long (&qv)[D] = S.qv; const uint4 (&ra)[D] = S.ra; const uint4 (&rb)[D] = S.rb; const unsigned (&hb)[D] = S.hb;
        if (CR && cr) {
            // Compact rows (sparse data: Ctx::crows): a (document, group) row lists the document's entries OUTSIDE the columns' mode bins -- up to eight
            // 16-bit words (column-in-group << 12 | bin), ascending, 0xffff = none -- so a row of mostly mode-bin cells costs one 16-byte request and
            // a couple of atomics instead of two requests and sixteen extract-and-compare steps.  The same atomics as the dense loop issues (the
            // mode bin is skipped there too), so the partial histograms are bit-identical.  A row with more than eight entries carries 0xfffe and
            // is read from the 32-byte dense row instead.
#pragma unroll
            for (int d = 0; d < D; d++) {
                if (k[d] < 0) continue;
                const unsigned w4[4] = {ra[d].x, ra[d].y, ra[d].z, ra[d].w};
                if ((w4[0] & 0xffffu) == 0xfffeu) {
                    const size_t kk = (size_t)k[d];
                    const uint4 *drow = (const uint4 *)c.dbins + 2 * grp + (size_t)2 * c.dm_gstride * kk;
                    const uint4 da = drow[0], db = drow[1];
#pragma unroll
                    for (int j = 0; j < SUB; j++) {
                        const unsigned t8 = bin8_of(da, db, fl0 + j);
                        if (t8 != md8[j]) {
                            atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), qv[d]);
                            if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), 1u);
                        }
                    }
                    continue;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const unsigned ent = (u & 1) ? (w4[u >> 1] >> 16) : (w4[u >> 1] & 0xffffu);
                    if (ent == 0xffffu) break;                  // entries are packed at the front
                    const unsigned j = ent >> 12, t8 = (ent & 0xfffu) << 3;
                    atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), qv[d]);
                    if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), 1u);
                }
            }
        } else
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (k[d] >= 0) {
#pragma unroll
                for (int j = 0; j < SUB; j++) {
                    if (RUNS && ((runmask >> j) & 1u)) continue;
                    const unsigned t8 = P8 ? pbin8_of(ra[d], hb[d], fl0 + j) : bin8_of(ra[d], rb[d], fl0 + j);
                    if (t8 != md8[j]) {
                        atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), qv[d]);
                        if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), 1u);
                    }
                }
            }
        }
        if (RUNS && runmask) {
#pragma unroll
            for (int d = 0; d < D; d++) {
                if (k[d] < 0) continue;
#pragma unroll
                for (int j = 0; j < SUB; j++) {
                    if (!((runmask >> j) & 1u)) continue;                   // block-uniform: a scalar branch
                    const unsigned t8 = P8 ? pbin8_of(ra[d], hb[d], fl0 + j) : bin8_of(ra[d], rb[d], fl0 + j);
                    // a neighbour that is not running (past the end of the chunk) reads as different: `old` = ~t8
                    const unsigned k1 = (unsigned)__builtin_amdgcn_update_dpp((int)~t8, (int)t8, 0xB1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
                    const unsigned k2 = (unsigned)__builtin_amdgcn_update_dpp((int)~t8, (int)t8, 0x4E, 0xf, 0xf, false);      // quad_perm [2,3,0,1]
                    const unsigned k3 = (unsigned)__builtin_amdgcn_update_dpp((int)~t8, (int)t8, 0x1B, 0xf, 0xf, false);      // quad_perm [3,2,1,0]
                    const unsigned mdj = md8[j];
                    unsigned long long add = qv[d]; unsigned cadd = 1u; bool mine = true;
                    if (t8 == k1 && t8 == k2 && t8 == k3) {
                        const unsigned lo = (unsigned)add, hi = (unsigned)(add >> 32);
                        add += ((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, 0xB1, 0xf, 0xf, false) << 32) |
                               (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xf, 0xf, false);
                        const unsigned lo1 = (unsigned)add, hi1 = (unsigned)(add >> 32);
                        add += ((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(0, (int)hi1, 0x4E, 0xf, 0xf, false) << 32) |
                               (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo1, 0x4E, 0xf, 0xf, false);
                        cadd = 4u; mine = (threadIdx.x & 3) == 0;
                    }
                    if (mine && t8 != mdj) {
                        atomicAdd((unsigned long long *)(lsum_b + (size_t)j * LT * 8 + t8), add);
                        if (!ROOT) atomicAdd((unsigned *)(lcnt_b + (size_t)j * LT * 4 + (t8 >> 1)), cadd);
                    }
                }
            }
        }
        };
    auto next_ids = [&](const int pb, int (&ko)[D]) {
#pragma unroll
        for (int d = 0; d < D; d++) { const int p = pb + d * NT; ko[d] = (p < p1) ? (ROOT ? p : idx[p]) : -1; }
    };
    constexpr bool PF = !ROOT && !FQ && RL_HIST_PREFETCH;
    constexpr bool PF2 = PF && RL_HIST_PREFETCH == 2;        // the two stages ping-pong between two register sets (no copy at the loop's end)
    if (PF2) {
        Stage S0, S1;
        int kB[D], kC[D];
        const int tb = p0 + (int)threadIdx.x;
        next_ids(tb + D * NT, kB);
        stage_load(tb, kn, S0);
        for (int pb = tb; pb < p1; pb += 2 * D * NT) {
            const int ub = pb - (int)threadIdx.x;           // block-uniform
            next_ids(pb + 2 * D * NT, kC);
            const bool h1 = ub + D * NT < p1;
            if (h1) stage_load(pb + D * NT, kB, S1);
            stage_acc(S0);
            if (!h1) break;
            next_ids(pb + 3 * D * NT, kB);
            if (ub + 2 * D * NT < p1) stage_load(pb + 2 * D * NT, kC, S0);
            stage_acc(S1);
        }
    } else if (!PF) {
        for (int pb = p0 + threadIdx.x; pb < p1; pb += D * NT) {
            Stage S;
            stage_load(pb, kn, S);
            next_ids(pb + D * NT, kn);
            stage_acc(S);
        }
    } else {
        Stage S0, S1;
        int k2[D];
        next_ids(p0 + (int)threadIdx.x + D * NT, k2);       // (kn: iteration 0, k2: iteration 1)
        stage_load(p0 + (int)threadIdx.x, kn, S0);
        for (int pb = p0 + threadIdx.x; pb < p1; pb += D * NT) {
            int k3[D];
            next_ids(pb + 2 * D * NT, k3);
            if (pb - (int)threadIdx.x + D * NT < p1) stage_load(pb + D * NT, k2, S1);      // (block-uniform)
            stage_acc(S0);
            S0 = S1;
#pragma unroll
            for (int d = 0; d < D; d++) k2[d] = k3[d];
        }
    }
    RL_TR_MARK(4);
    if (want_tot) {         // sum of q over the chunk (|q| < 2^48, <= 2^14 samples: fits int64)
        tot = (long long)wave_sum_u64((unsigned long long)tot);
        __shared__ long long wtot[NT / 64];
        if (lane_id() == 0) wtot[threadIdx.x >> 6] = tot;
        __syncthreads();
        if (threadIdx.x == 0) { long long v = 0; for (int w = 0; w < NT / 64; w++) v += wtot[w]; c.part_tot[by] = v; }
        if (FQ && threadIdx.x == 0 && by == 0) { c.st->E = qE; c.st->E2 = qE2; }
    }
    if (fq_r) {       // the root's sum of r (k_quantize's tail)
        for (int o = 32; o > 0; o >>= 1) sq_acc += __shfl_xor(sq_acc, o);
        __shared__ long long wsq[NT / 64];
        if (lane_id() == 0) wsq[threadIdx.x >> 6] = sq_acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long v = 0; for (int w = 0; w < NT / 64; w++) v += wsq[w];
            atomicAdd((unsigned long long *)&c.st->root_sq, (unsigned long long)v);
        }
    }
    __syncthreads();
    RL_TR_MARK(5);
    long long *ps = c.part_sum + ((size_t)by * c.F + f0) * TS;
    int *pc = c.part_cnt + ((size_t)by * c.F + f0) * TS;
    if (TSC) {       // (LT is a compile-time constant: no run-time division per element)
        for (int i = threadIdx.x; i < nf * LT; i += NT) {
            const int j = i / LT, t = i - j * LT;
            if (t < TS) {
                ps[j * TS + t] = (long long)lsum[i];
                if (!ROOT) pc[j * TS + t] = (int)((const unsigned *)lcnt_b)[i];
            }
        }
    } else
    for (int i = threadIdx.x; i < nf * TS; i += NT) {
        const int j = i / TS, t = i - j * TS;
        ps[i] = (long long)lsum[j * LT + t];
        if (!ROOT) pc[i] = (int)((const unsigned *)lcnt_b)[j * LT + t];
    }
    if (!ROOT) RL_TR_END(1, by * (int)gridDim.x + bx);
}


// Child passes run on a BOUNDED grid (launch_hist: about one resident set of blocks) and every block walks the chunks by, by + gridDim.y, ..: the
// number of chunks of a step is only known on the device, and a grid sized for the worst case (N / 8192 + 270 chunks x 9 groups = 6 624 blocks at
// c2) spent ~5 us per launch dispatching blocks that leave at once -- more than the working blocks of a small step need.
template <bool ROOT, int SUB, int TSC, bool RUNS = false, bool P8 = false, int NT = kThreads, bool CR = false, bool FQ = false>
__global__ __launch_bounds__(NT) void k_hist(const Ctx c)
{
    extern __shared__ unsigned long long lsum[];
    const TreeState *st = c.st;
    // XCD-aware block -> (feature group, chunk) map.  Block b is observed to run on XCD b % 8 and every XCD has its own L2: the
    // feature-group blocks of ONE chunk all read that chunk's lambdas and sample ids, so they are given ids that are congruent
    // mod 8 (chunk y lives on XCD y % 8) instead of consecutive ids that spread a chunk over all eight L2s (the PMC pass counted
    // the 8-byte lambda stream nine times).  A speed choice only; gridDim.y is a multiple of 8 (launch_hist).
#ifndef RL_HIST_NO_XCD
    const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x, lk = lin >> 3;
    const int bx = (int)(lk % gridDim.x), by = (int)((lk / gridDim.x) * 8 + (lin & 7));
#else
    const int bx = blockIdx.x, by = blockIdx.y;
#endif
    if (ROOT) { hist_chunk<ROOT, SUB, TSC, RUNS, P8, NT, CR, FQ>(c, st, bx, by, lsum); return; }
    const int total = st->done ? 0 : st->chunks_total;
    for (int y = by; y < total; y += (int)gridDim.y) {
        hist_chunk<ROOT, SUB, TSC, RUNS, P8, NT, CR, FQ>(c, st, bx, y, lsum);
        __syncthreads();        // the flush has read the LDS histogram: the next chunk may zero it
    }
}

}  // namespace rl
