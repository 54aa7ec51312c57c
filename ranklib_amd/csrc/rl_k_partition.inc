// rl_k_partition.inc -- K6: the stable partition of the sample lists.  k_part_count (sharded runs), the tile descriptors, both decoupled look-backs and
// k_part_scatter.  Included by rl_kernels_round.inc; needs that file's trace block (RL_TR_*), rl_k_hist.inc (slot_of_tile) and none of
// the other pieces.

namespace rl {

// ------------------------------------------------------------------------------------------------
// K6: stable partition of the sample lists of the step's nodes by bin[f*][k] <= t*.  grid = tiles of all slots.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_part_count(const Ctx c)
{   // sharded runs only: left members per tile
    const TreeState *st = c.st;
    const int j = slot_of_tile(st, blockIdx.x);
    if (j < 0) return;
    const SlotRec &sl = st->slot[j];
    const int cnt = sl.pcount, t = sl.t;
    const bool root = (sl.node == 0);
    const int *src = root ? nullptr : c.idx[sl.pbuf] + sl.pstart;
    const int base = (blockIdx.x - sl.tile0) * kPartTile;
    const uint16_t *b = c.bins + (size_t)sl.f * c.Npad;
    constexpr int PER = kPartTile / kThreads;
    int ks[PER]; unsigned short bv[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int pos = base + i * kThreads + threadIdx.x;
        ks[i] = (pos < cnt) ? (root ? pos : src[pos]) : -1;
    }
#pragma unroll
    for (int i = 0; i < PER; i++) bv[i] = b[max(ks[i], 0)];          // unconditional gathers (see k_part_scatter)
    int n = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) n += (ks[i] >= 0) && ((int)bv[i] <= t);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    __shared__ int part[4];
    if (lane_id() == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) c.tile_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Tile descriptors of the single-pass partition (decoupled look-back): (epoch << 34) | (status << 32) | left count.
// epoch = growth step counter, so descriptors of earlier steps are simply invalid (no clearing pass).
constexpr unsigned long long kDescAgg = 1ull, kDescPrefix = 2ull;
__device__ __forceinline__ unsigned long long make_desc(int epoch, unsigned long long status, int v)
{
    return ((unsigned long long)(epoch & 0x3fffffff) << 34) | (status << 32) | (unsigned)v;
}

// exclusive number of left members in the tiles before local tile `ltile` of this slot; publishes this tile's
// aggregate first and its inclusive prefix afterwards.  Called by wavefront 0 of the block (all 64 lanes).
// Blocks are dispatched in blockIdx order, so every tile looked at belongs to a block that is running or finished.
__device__ int lookback_exclusive(unsigned long long *desc, int ltile, int epoch, int tile_left, int *error)
{
    const int lane = lane_id();
    if (ltile == 0) {
        if (lane == 0) __hip_atomic_store(&desc[0], make_desc(epoch, kDescPrefix, tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return 0;
    }
    if (lane == 0) __hip_atomic_store(&desc[ltile], make_desc(epoch, kDescAgg, tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long tag = (unsigned long long)(epoch & 0x3fffffff);
    int excl = 0, look = ltile - 1, spins = 0;
    // kLookWin windows of 64 predecessors are requested at once: the tiles of a step run concurrently, so their aggregates are all there after one
    // memory round trip, while a prefix only appears once a tile has finished its own look-back -- walking back 64 tiles per round trip put
    // (tiles / 64) round trips on the last tile of a large node (8 for a 1 M-document parent).  The windows are consumed nearest first exactly as
    // before; the first one that is not complete yet ends the batch and is asked for again.
#ifndef RL_LOOK_WIN
#define RL_LOOK_WIN 8
#endif
    constexpr int kLookWin = RL_LOOK_WIN;
    bool found = false;
    while (!found) {
        unsigned long long dw[kLookWin];
#pragma unroll
        for (int u = 0; u < kLookWin; u++) {
            const int i = look - 64 * u - lane;               // lane 0 = nearest predecessor of the window
            dw[u] = make_desc(epoch, kDescPrefix, 0);         // before the first tile: prefix 0
            if (i >= 0) dw[u] = __hip_atomic_load(&desc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // (one reduction per batch, on the DPP path: a __shfl_xor is a ds_bpermute, and six dependent LDS round trips per window -- 48 per batch -- were
        // most of the 4-5 us a tile waited AFTER its last predecessor had published)
        bool stale = false;
        unsigned acc = 0u;
#pragma unroll
        for (int u = 0; u < kLookWin; u++) {
            if (found || stale) continue;
            const unsigned long long d = dw[u];
            const bool valid = ((d >> 34) == tag) && (((d >> 32) & 3ull) != 0ull);
            const bool isp = valid && (((d >> 32) & 3ull) == kDescPrefix);
            const unsigned long long vmask = __ballot(valid), pmask = __ballot(isp);
            const int fp = pmask ? __builtin_ctzll(pmask) : 64;                // nearest lane holding an inclusive prefix
            const unsigned long long need = (fp >= 63) ? ~0ull : ((1ull << (fp + 1)) - 1ull);
            if ((vmask & need) == need) {
                acc += (lane <= fp) ? (unsigned)d : 0u;
                if (pmask) found = true;
                else look -= 64;
            } else stale = true;
        }
        excl += (int)wave_sum_u32(acc);
        if (stale && !found) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1 << 22)) { if (lane == 0) atomicExch(error, 3); break; }      // never hang the GPU
        }
    }
    if (lane == 0) __hip_atomic_store(&desc[ltile], make_desc(epoch, kDescPrefix, excl + tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

// Two-level form of the same (round 5).  With every tile of a large node resident at once nobody finds a published PREFIX to stop at: tile i walked
// back over all i aggregates -- n^2 / 128 uncached wave loads on 15 KB of descriptors (13.6 MB at 1 841 tiles, a handful of memory channels) -- and
// the look-back ended 9-17 us after the last count had been published (profiles/r05c_step_trace_*).  Here a tile reads ONE window: the aggregates
// of its own group of 64 tiles; the last tile of a group publishes the group's total, and a tile adds the totals of the groups before its own
// (one more window per 4 096 tiles): 1 KB per tile, two dependent round trips behind the slowest publication.
__device__ __forceinline__ unsigned long long ld_desc(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ int lookback2_exclusive(unsigned long long *desc, unsigned long long *gdesc, int ltile, int epoch, int tile_left, int *error)
{
    const int lane = lane_id();
    const int g = ltile >> 6, r = ltile & 63;
    if (lane == 0) __hip_atomic_store(&desc[ltile], make_desc(epoch, kDescAgg, tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long tag = (unsigned long long)(epoch & 0x3fffffff);
    const int ngw = (g + 63) >> 6;                       // windows of group totals before this tile's group
    constexpr int kGW = 8;                               // in flight together (32 768 tiles); more are walked in further trips
    int excl = 0, spins = 0;
    // own group: aggregates of the tiles before this one
    bool have_in = (r == 0);
    unsigned gdone = 0u;                                 // bit u: window u of the group totals has been summed
    int gw0 = 0;
    while (true) {
        unsigned long long din = make_desc(epoch, kDescAgg, 0);
        if (!have_in && lane < r) din = ld_desc(&desc[(g << 6) + lane]);
        unsigned long long dg[kGW];
#pragma unroll
        for (int u = 0; u < kGW; u++) {
            dg[u] = make_desc(epoch, kDescPrefix, 0);
            const int gi = ((gw0 + u) << 6) + lane;
            if (gw0 + u < ngw && !((gdone >> u) & 1u) && gi < g) dg[u] = ld_desc(&gdesc[gi]);
        }
        unsigned acc = 0u;
        if (!have_in) {
            const bool ok = ((din >> 34) == tag) && (((din >> 32) & 3ull) != 0ull);
            if (__ballot(!ok) == 0ull) {
                const unsigned mine = (lane < r) ? (unsigned)din : 0u;
                const unsigned in_sum = wave_sum_u32(mine);
                excl += (int)in_sum;
                have_in = true;
                // the last tile of a full group publishes the group's total (nobody needs the total of the node's last, partial group)
                if (r == 63 && lane == 0)
                    __hip_atomic_store(&gdesc[g], make_desc(epoch, kDescPrefix, (int)in_sum + tile_left), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        bool all_g = true;
#pragma unroll
        for (int u = 0; u < kGW; u++) {
            if (gw0 + u >= ngw || ((gdone >> u) & 1u)) continue;
            const bool ok = ((dg[u] >> 34) == tag) && (((dg[u] >> 32) & 3ull) == kDescPrefix);
            if (__ballot(!ok) == 0ull) { acc += (unsigned)dg[u]; gdone |= 1u << u; }
            else all_g = false;
        }
        excl += (int)wave_sum_u32(acc);
        if (all_g && gw0 + kGW < ngw) { gw0 += kGW; gdone = 0u; all_g = false; if (have_in) continue; }
        if (have_in && all_g) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 22)) { if (lane == 0) atomicExch(error, 3); break; }      // never hang the GPU
    }
    return excl;
}

// (Measured and dropped, round 5: group totals ACCUMULATED by the tiles -- one agent-scope atomic add of (1 << 32 | count) per tile on its group's word,
// valid at 64 arrivals -- so that the two windows no longer depend on each other: 64 same-address atomics per word serialise at the memory side,
// c2 414 -> 364 rounds/s.)
// LOOKBACK (one GPU: the size of the left child is known from the count histogram): single pass.
// !LOOKBACK (sharded: local sizes unknown): second pass after k_part_count.
// Samples are read and written row-wise (thread t takes samples t, t+256, ..): every load is coalesced and each
// wavefront writes one contiguous run to the left list and one to the right list per row.  The fixed-point lambda of the
// built child's members is written in list order next to their ids (ql): its histogram pass reads it contiguously.
#ifndef RL_PART_WAVES
#define RL_PART_WAVES 0
#endif
template <bool LOOKBACK>
__global__ __launch_bounds__(kThreads)
#if RL_PART_WAVES
__attribute__((amdgpu_waves_per_eu(RL_PART_WAVES)))
#endif
void k_part_scatter(const Ctx c)
{
    TreeState *st = c.st;
    RL_TR_BEGIN();
    const int j = slot_of_tile(st, blockIdx.x);
    if (j < 0) return;
    const SlotRec sl = st->slot[j];                                 // (copied whole: one batch of loads)
    const int epoch = st->epoch;
    const int cnt = sl.pcount, t = sl.t, pstart = sl.pstart, pbuf = sl.pbuf;
    const bool root = (sl.node == 0);
    const bool bl = sl.build_left != 0;         // the child whose histogram is accumulated from its documents (the smaller one)
    RL_TR_MARK(1);
    const int *src = root ? nullptr : c.idx[pbuf] + pstart;
    const int ltile = blockIdx.x - sl.tile0;
    const int base = ltile * kPartTile;
    constexpr int PER = kPartTile / kThreads, NW = kThreads / 64;
    const uint16_t *b = c.bins + (size_t)sl.f * c.Npad;
    __shared__ int wl[PER * NW + 1];
    __shared__ int sh_tileoff, sh_total;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int ks[PER]; unsigned long long bal[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int pos = base + i * kThreads + threadIdx.x;
        ks[i] = (pos < cnt) ? (root ? pos : src[pos]) : -1;
    }
    // (every gather below is UNCONDITIONAL, from a clamped index: a load inside `if (member)` sits in its own exec region and the compiler completes it
    // -- s_waitcnt vmcnt(0) -- before it issues the next one: the eight bin gathers and the eight lambda gathers of a thread were sixteen serial memory
    // round trips.  Lanes that do not need a value read element 0: one broadcast line)
    bool isl[PER];
    {
        unsigned short bv[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) bv[i] = b[max(ks[i], 0)];
#pragma unroll
        for (int i = 0; i < PER; i++) isl[i] = (ks[i] >= 0) && ((int)bv[i] <= t);
    }
    RL_TR_MARK(2);
#pragma unroll
    for (int i = 0; i < PER; i++) {
        bal[i] = __ballot(isl[i]);
        if (lane == 0) wl[i * NW + wave] = __builtin_popcountll(bal[i]);
    }
    __syncthreads();
    RL_TR_MARK(3);
    if (wave == 0) {       // exclusive prefix over the (row, wave) runs of the tile
        static_assert(PER * NW <= 64, "one wave scan over the tile's (row, wave) runs");
        const int v = (lane < PER * NW) ? wl[lane] : 0;
        const int inc = (int)wave_scan_u32((unsigned)v);
        const int tile_left = (int)readlane_u32((unsigned)inc, PER * NW - 1);
        if (lane < PER * NW) wl[lane] = inc - v;
        int tileoff, nleft;
        if (LOOKBACK) {
#if RL_LOOKBACK2
            tileoff = lookback2_exclusive(c.tile_desc + sl.tile0, c.tile_gdesc + (sl.tile0 >> 6) + j, ltile, epoch, tile_left, &st->error);
#else
            tileoff = lookback_exclusive(c.tile_desc + sl.tile0, ltile, epoch, tile_left, &st->error);
#endif
            nleft = sl.nleft;
        } else {           // left members in earlier tiles, and in all tiles (= local size of the left child)
            const int *tc = c.tile_cnt + sl.tile0;
            int pre = 0, tot = 0;
            for (int i = lane; i < sl.ntiles; i += 64) { const int x = tc[i]; tot += x; if (i < ltile) pre += x; }
            for (int o = 32; o > 0; o >>= 1) { pre += __shfl_xor(pre, o); tot += __shfl_xor(tot, o); }
            tileoff = pre; nleft = tot;
        }
        if (lane == 0) { sh_tileoff = tileoff; sh_total = nleft; }
    }
    // Only the BUILT child's histogram pass reads lambda in list order, and lambda^2 is needed as one sum per child: both are fetched by document id
    // for the members of the built child alone.  The lists themselves carry document ids only: a partition moves 8 bytes per document of the parent
    // instead of 40.  The gathers are requested HERE -- after the tile's count has been published, by wavefronts 1.. while wavefront 0 waits in the
    // look-back (and by wavefront 0 after it): requested before the barrier above (round 4) they sat between a tile and the publication of its
    // count, and every later tile's look-back waits for the slowest publication before it.
    long long qv[PER], rv[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const bool mine = (ks[i] >= 0) && (isl[i] == bl);
        const int ka = mine ? ks[i] : 0;
        qv[i] = c.q[ka]; rv[i] = c.r[ka];
    }
#pragma unroll
    for (int i = 0; i < PER; i++) if (!((ks[i] >= 0) && (isl[i] == bl))) { qv[i] = 0ll; rv[i] = 0ll; }
    __syncthreads();
    const int tileoff = sh_tileoff, nleft = sh_total;
    RL_TR_MARK(4);
    int *dstL = c.idx[1 - pbuf] + pstart;
    long long *qL = c.ql[1 - pbuf] + pstart;
    if (ltile == 0 && threadIdx.x == 0) {       // local list ranges of the two children
        NodeRec &Lw = c.nodes[sl.left]; NodeRec &Rw = c.nodes[sl.right];
        Lw.start = pstart; Lw.count = nleft;
        Rw.start = pstart + nleft; Rw.count = cnt - nleft;
    }
    long long sq = 0;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int i = 0; i < PER; i++) {
        if (ks[i] < 0) continue;
        const int pos = base + i * kThreads + threadIdx.x;
        const int lbefore = tileoff + wl[i * NW + wave] + __builtin_popcountll(bal[i] & below);   // left members before pos
        const int d = isl[i] ? lbefore : nleft + (pos - lbefore);       // stable: left run, then right run
        dstL[d] = ks[i];
        if (isl[i] == bl) { qL[d] = qv[i]; sq += rv[i]; }
    }
    // fixed-point sum of lambda^2 over the tile's members of the BUILT child: one partial per tile (summed by slot_sq_left / k_hist_finish block
    // (0, slot)); thousands of atomics on one address would serialise in L2.  The sibling's sum is parent - built, exactly (integers).
    RL_TR_MARK(5);
    sq = (long long)wave_sum_u64((unsigned long long)sq);
    __shared__ long long sh_sq[NW];
    if (lane == 0) sh_sq[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) { long long v = 0; for (int w = 0; w < NW; w++) v += sh_sq[w]; c.tile_sq[blockIdx.x] = v; }
    RL_TR_END(0, blockIdx.x);
}

}  // namespace rl
