// rl_eval_sort.inc -- rl_eval_lists' long lists: ranked by a sort on integer keys (rl_rank_sort_dev.h) instead of the O(n^2) count.
// DESIGN.md 19.5.  Included by rl_ca.hip's unit before rl_eval.inc, whose rl_eval_lists launches these; the scorers (ev_metric) are used unchanged.
//
//   in-LDS class, kEvSort < n <= kEvSortLds: one block per list.
//     k_eval_sort_lds<NT, CAP>  keys and indices of the list go into LDS (12 B a record), rs_block_sort ranks them, then ranked label p
//                               = labels[idx[p]] is written over idx[p] (one thread reads and writes slot p), pos[idx[p]] = p when
//                               asked, and after a barrier the first lane runs ev_metric on the ranked labels.
//                                 n <= kEvSortSmall (2 048)  NT = 256,  24 KiB of LDS: six blocks per CU, a file of many such lists fills the chip
//                                 n <= kEvSortLds (13 312)   NT = 1024, 13 312 x 12 B = 156 KiB of a CU's 160 KiB: one block per CU, sixteen
//                                                            wavefronts on the one list
//   multi-block class, longer, any length: all its lists share every launch, dependencies are launch boundaries only.
//     k_eval_sort_tiles         grid over (list x tile of kEvSortTile = 8 192 records): a block of 1 024 threads sorts its tile in 96 KiB of
//                               LDS (one block per CU; the class's shortest list has two tiles, so the first merge is tested at its
//                               smallest) and writes it to scratch 0.
//     k_eval_sort_merge         ceil(log2(most tiles of a list)) launches, scratch 0 -> 1 -> 0 ..: grid over (list x piece of kEvSortPiece =
//                               2 048 output records).  A piece lies inside one pair of runs; two lanes find its ends on the pair's merge
//                               path (binary search on the diagonal, in global memory), the block loads the two slices (2 048 records
//                               together, 24 KiB of LDS, six blocks per CU) and every record finds its output slot as its place in its own
//                               slice plus the count of the other slice's records before it (binary search in LDS).  A run without a
//                               partner is copied.
//     k_eval_sort_finish        one block per list: ranked labels into a.glab, positions, a barrier, ev_metric by the first lane on the
//                               ranked labels in global memory -- the serial chain the global counting class had.
//     Scratch: two (key, index) buffers over the class's documents, 24 B a document, from the call's DevPool.
#include "rl_eval_host.h"
#include "rl_rank_sort_dev.h"

namespace rl {

constexpr int kEvSortSmall = 2048, kEvSortThreads = 1024, kEvSortTile = 8192, kEvSortPiece = 2048;
static_assert(kEvSort >= kEvWave && kEvSort <= kEvBlock && kEvSortLds > kEvSort, "class edges in order, the counting class inside its LDS");
static_assert(kEvSortLds * 12 <= 160 * 1024, "the in-LDS class fits a CU's LDS");
static_assert(kEvSortTile % kEvSortPiece == 0, "a piece never straddles two pairs of runs");

struct EvSortArgs {
    EvArgs ev;                                   // qlist / nq: the lists of the multi-block class
    const int32_t *moff, *toff, *poff;           // [nq + 1] (EvSplit)
    unsigned long long *key[2]; unsigned *idx[2];    // the two scratch buffers, [moff[nq]] each
};

template <int NT, int CAP>
__global__ __launch_bounds__(NT) void k_eval_sort_lds(const EvArgs a)
{
    __shared__ unsigned long long s_key[CAP];
    __shared__ unsigned s_idx[CAP];
    const int q = a.qlist[blockIdx.x];
    const int cur = a.qoff[q], n = a.qoff[q + 1] - cur;
    for (int i = threadIdx.x; i < n; i += NT) { s_key[i] = rs_key(a.sc[cur + i]); s_idx[i] = (unsigned)i; }
    __syncthreads();
    rs_block_sort<NT>(s_key, s_idx, n);
    float *lab = reinterpret_cast<float *>(s_idx);
    for (int p = threadIdx.x; p < n; p += NT) {
        const int i = (int)s_idx[p];
        lab[p] = a.labels[cur + i];
        if (a.pos) a.pos[cur + i] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) a.out[q] = ev_metric(a, q, n, lab);
}

// the last s in [0, nq) with tab[s] <= b (tab[0] = 0, tab increases strictly, b < tab[nq])
__device__ __forceinline__ int es_slot(const int32_t *tab, int nq, int b)
{
    int lo = 0, hi = nq - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kEvSortThreads) void k_eval_sort_tiles(const EvSortArgs a)
{
    __shared__ unsigned long long s_key[kEvSortTile];
    __shared__ unsigned s_idx[kEvSortTile];
    const int slot = es_slot(a.toff, a.ev.nq, (int)blockIdx.x);
    const int q = a.ev.qlist[slot];
    const int cur = a.ev.qoff[q], n = a.ev.qoff[q + 1] - cur;
    const int t0 = ((int)blockIdx.x - a.toff[slot]) * kEvSortTile;
    const int m = n - t0 < kEvSortTile ? n - t0 : kEvSortTile;
    for (int i = threadIdx.x; i < m; i += kEvSortThreads) { s_key[i] = rs_key(a.ev.sc[cur + t0 + i]); s_idx[i] = (unsigned)(t0 + i); }
    __syncthreads();
    rs_block_sort<kEvSortThreads>(s_key, s_idx, m);
    const size_t at = (size_t)a.moff[slot] + (size_t)t0;
    for (int i = threadIdx.x; i < m; i += kEvSortThreads) { a.key[0][at + i] = s_key[i]; a.idx[0][at + i] = s_idx[i]; }
}

// runs of `run` records in scratch `src` merged pairwise into scratch 1 - src
__global__ __launch_bounds__(kThreads) void k_eval_sort_merge(const EvSortArgs a, const int64_t run, const int src)
{
    __shared__ unsigned long long s_key[kEvSortPiece];
    __shared__ unsigned s_idx[kEvSortPiece];
    __shared__ int s_cut[2];
    const int slot = es_slot(a.poff, a.ev.nq, (int)blockIdx.x);
    const int q = a.ev.qlist[slot];
    const int64_t n = a.ev.qoff[q + 1] - a.ev.qoff[q];
    const int64_t o0 = (int64_t)((int)blockIdx.x - a.poff[slot]) * kEvSortPiece;          // < n
    const int64_t base = o0 / (2 * run) * (2 * run);                                      // the pair's first record: <= o0
    const int na = (int)(n - base < run ? n - base : run);                                // >= 1
    const int nb = (int)(n - base - na < run ? n - base - na : run);                      // 0: a run without a partner
    const size_t mb = (size_t)a.moff[slot];
    const unsigned long long *ka = a.key[src] + mb + base, *kb = ka + na;
    const unsigned *ia = a.idx[src] + mb + base, *ib = ia + na;
    const int64_t d0 = o0 - base, both = (int64_t)na + nb;
    const int64_t d1 = d0 + kEvSortPiece < both ? d0 + kEvSortPiece : both;               // > d0
    if (threadIdx.x == 0) s_cut[0] = rs_merge_path(ka, ia, na, kb, ib, nb, (int)d0);
    if (threadIdx.x == kWave) s_cut[1] = rs_merge_path(ka, ia, na, kb, ib, nb, (int)d1);
    __syncthreads();
    const int a0 = s_cut[0], b0 = (int)d0 - a0;
    const int ca = s_cut[1] - a0, cb = (int)(d1 - d0) - ca;                               // ca + cb <= kEvSortPiece
    for (int x = threadIdx.x; x < ca + cb; x += kThreads) {
        s_key[x] = x < ca ? ka[a0 + x] : kb[b0 + x - ca];
        s_idx[x] = x < ca ? ia[a0 + x] : ib[b0 + x - ca];
    }
    __syncthreads();
    unsigned long long *kd = a.key[1 - src] + mb + o0;
    unsigned *id = a.idx[1 - src] + mb + o0;
    for (int x = threadIdx.x; x < ca + cb; x += kThreads) {
        const unsigned long long k = s_key[x];
        const unsigned i = s_idx[x];
        const int o = x < ca ? x + rs_count_before(s_key + ca, s_idx + ca, cb, k, i) : x - ca + rs_count_before(s_key, s_idx, ca, k, i);
        kd[o] = k; id[o] = i;
    }
}

__global__ __launch_bounds__(kEvSortThreads) void k_eval_sort_finish(const EvSortArgs a, const int src)
{
    const int slot = (int)blockIdx.x;
    const int q = a.ev.qlist[slot];
    const int cur = a.ev.qoff[q], n = a.ev.qoff[q + 1] - cur;
    const unsigned *idx = a.idx[src] + (size_t)a.moff[slot];
    float *lab = a.ev.glab + cur;
    for (int p = threadIdx.x; p < n; p += kEvSortThreads) {
        const int i = (int)idx[p];
        lab[p] = a.ev.labels[cur + i];
        if (a.ev.pos) a.ev.pos[cur + i] = p;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) a.ev.out[q] = ev_metric(a.ev, q, n, lab);
}

constexpr EvEdges kEvEdges = {kEvTiny, kEvWave, kEvSort, kEvSortLds, kEvSortTile, kEvSortPiece};

// the in-LDS class
static int ev_sort_lds(EvArgs a, const EvSplit &s, const int32_t *qoff, DevPool &buf)
{
    // the lists up to kEvSortSmall first, then the others: one table, two launches
    std::vector<int32_t> order;
    int32_t n_small = 0;
    for (int big = 0; big < 2; big++)
        for (int32_t q : s.lists[kEvClsSortLds])
            if ((qoff[q + 1] - qoff[q] > kEvSortSmall) == (big == 1)) { order.push_back(q); n_small += 1 - big; }
    int32_t *d_list = nullptr;
    RL_HIP(buf.upload(&d_list, (const int32_t *)order.data(), order.size()));
    if (n_small) {
        a.qlist = d_list; a.nq = n_small;
        hipLaunchKernelGGL((k_eval_sort_lds<kThreads, kEvSortSmall>), dim3((unsigned)n_small), dim3(kThreads), 0, 0, a);
        RL_HIP(hipGetLastError());
    }
    if ((size_t)n_small < order.size()) {
        a.qlist = d_list + n_small; a.nq = (int32_t)order.size() - n_small;
        hipLaunchKernelGGL((k_eval_sort_lds<kEvSortThreads, kEvSortLds>), dim3((unsigned)a.nq), dim3(kEvSortThreads), 0, 0, a);
        RL_HIP(hipGetLastError());
    }
    return RL_OK;
}

// the multi-block class: a.glab holds [n_docs] floats
static int ev_sort_multi(const EvArgs &ev, const EvSplit &s, DevPool &buf)
{
    EvSortArgs a;
    memset(&a, 0, sizeof(a));
    a.ev = ev;
    const std::vector<int32_t> &lists = s.lists[kEvClsSortMulti];
    const size_t nq = lists.size(), docs = (size_t)s.moff.back();
    int32_t *d_list = nullptr, *d_moff = nullptr, *d_toff = nullptr, *d_poff = nullptr;
    RL_HIP(buf.upload(&d_list, lists.data(), nq));
    RL_HIP(buf.upload(&d_moff, s.moff.data(), nq + 1));
    RL_HIP(buf.upload(&d_toff, s.toff.data(), nq + 1));
    RL_HIP(buf.upload(&d_poff, s.poff.data(), nq + 1));
    for (int b = 0; b < 2; b++) { RL_HIP(buf.alloc(&a.key[b], docs)); RL_HIP(buf.alloc(&a.idx[b], docs)); }
    a.ev.qlist = d_list; a.ev.nq = (int32_t)nq; a.moff = d_moff; a.toff = d_toff; a.poff = d_poff;
    hipLaunchKernelGGL(k_eval_sort_tiles, dim3((unsigned)s.toff.back()), dim3(kEvSortThreads), 0, 0, a);
    RL_HIP(hipGetLastError());
    int src = 0;
    for (int32_t pass = 0; pass < s.passes; pass++, src = 1 - src) {
        hipLaunchKernelGGL(k_eval_sort_merge, dim3((unsigned)s.poff.back()), dim3(kThreads), 0, 0, a, (int64_t)kEvSortTile << pass, src);
        RL_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_eval_sort_finish, dim3((unsigned)nq), dim3(kEvSortThreads), 0, 0, a, src);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
