// rl_rank_sort_dev.h -- ranking a list by a sort instead of a count: the device functions, in a header of their own so that any kernel that
// ranks (k_stage_eval, k_rank_*, k_ca_trials: all counting today) can call them later.  rl_eval_sort.inc holds the kernels.  DESIGN.md 19.5.
//
//   record     one per document: a 64-bit key and the document's 32-bit index within its list, kept in two arrays (keys as ds_read_b64
//              at consecutive addresses, indices as ds_read_b32: both free of bank conflicts at unit stride).
//   rs_key     the f64 score as an unsigned integer whose DESCENDING order is the score's descending order: -0.0 folded onto +0.0 (they
//              tie), then the sign bit set on non-negative values and every bit flipped on negative ones.  +-Infinity are ordinary
//              values; NaN never arrives.  No score maps to key 0 (only the all-ones pattern would, a NaN).  st_key (rl_stage.inc) is
//              the f32 form.
//   rs_before  (key descending, index ascending): a total order, so the sort need not be stable and the result is
//              MergeSorter.sort(double[], false) exactly.
//   rs_block_sort<NT>
//              a block of NT threads sorts n records in LDS with a bitonic network in its same-direction form: stage k merges sorted
//              runs of k / 2 by one mirrored step (i against its run pair's mirror image) and then half-cleaner steps of stride
//              k / 4 .. 1, and every compare-exchange puts the earlier record at the lower address.  Because of that, n need not be a
//              power of two: slots n .. 2^m - 1 behave as records that come last and never move, so a pair whose upper slot is past n
//              is skipped, and no padding is stored.  The network has no data-dependent branch but the swap and no second buffer (a
//              merge sort in LDS would halve the longest list that fits).  Steps of stride <= 64 touch one aligned chunk of 128 records
//              only, so a wavefront takes a chunk through all of them with a wavefront fence between steps, not a block barrier: of
//              the m (m + 1) / 2 steps of 2^m records, 28 + 7 (m - 7) are wavefront-local and (m - 7) (m - 6) / 2 cross the block
//              (m = 14: 77 and 28).
//   rs_merge_path
//              how many records of run A are among the first d of the merge of A and B (binary search on the diagonal).
//   rs_count_before
//              how many records of a sorted run come before a given record (binary search): with the order total, a record's place in
//              the merge of two runs is its place in its own run plus this count in the other.
#pragma once
#include "rl_eval_dev.h"

namespace rl {

constexpr int kRsChunk = 2 * kWave;          // records a wavefront's local steps cover
constexpr unsigned kRsLog2Chunk = 7;

__device__ __forceinline__ unsigned long long rs_key(double s)
{
    unsigned long long u = (unsigned long long)__double_as_longlong(s);
    const unsigned long long sign = 0x8000000000000000ull;
    if (u == sign) u = 0ull;                                                // -0.0 == 0.0: a tie, the given order decides
    return (u & sign) ? ~u : (u | sign);
}

__device__ __forceinline__ bool rs_before(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib)
{
    return ka > kb || (ka == kb && ia < ib);
}

// compare-exchange of slots i < p: the earlier record to i
__device__ __forceinline__ void rs_cex(unsigned long long *key, unsigned *idx, int i, int p)
{
    const unsigned long long ku = key[i], kv = key[p];
    const unsigned iu = idx[i], iv = idx[p];
    if (rs_before(kv, iv, ku, iu)) { key[i] = kv; key[p] = ku; idx[i] = iv; idx[p] = iu; }
}

// the half-cleaner steps of stride j, j / 2, .. 1 (j <= kWave) on the chunk at base, by one wavefront
__device__ __forceinline__ void rs_wave_tail(unsigned long long *key, unsigned *idx, int base, int n, int j, int lane)
{
    for (; j >= 1; j >>= 1) {
        const int i = base + (lane / j) * 2 * j + (lane % j), p = i + j;
        if (p < n) rs_cex(key, idx, i, p);
        ca_sync<kWave>();
    }
}

template <int NT>
__device__ void rs_block_sort(unsigned long long *key, unsigned *idx, int n)
{
    static_assert(NT % kWave == 0, "whole wavefronts");
    constexpr int NW = NT / kWave;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int chunks = (n + kRsChunk - 1) >> kRsLog2Chunk;
    // stages 2 .. 128: every chunk on its own
    for (int c = wave; c < chunks; c += NW) {
        const int base = c << kRsLog2Chunk;
#pragma unroll 1
        for (int k = 2; k <= kRsChunk; k <<= 1) {
            const int half = k >> 1, run = lane / half, o = lane % half;
            const int i = base + run * k + o, p = base + run * k + k - 1 - o;
            if (p < n) rs_cex(key, idx, i, p);
            ca_sync<kWave>();
            rs_wave_tail(key, idx, base, n, k >> 2, lane);
        }
    }
    __syncthreads();
    // stages 256 .. : the steps of stride >= 128 across the block, the rest by chunk
    for (int k = 2 * kRsChunk; (k >> 1) < n; k <<= 1) {
        const int half = k >> 1;
        for (int t = threadIdx.x;; t += NT) {
            const int run = t / half, o = t % half;
            const int i = run * k + o, p = run * k + k - 1 - o;
            if (i >= n) break;                                              // i grows with t
            if (p < n) rs_cex(key, idx, i, p);
        }
        __syncthreads();
        for (int j = k >> 2; j >= kRsChunk; j >>= 1) {
            for (int t = threadIdx.x;; t += NT) {
                const int i = (t / j) * 2 * j + (t % j), p = i + j;
                if (i >= n) break;
                if (p < n) rs_cex(key, idx, i, p);
            }
            __syncthreads();
        }
        for (int c = wave; c < chunks; c += NW) rs_wave_tail(key, idx, c << kRsLog2Chunk, n, kWave, lane);
        __syncthreads();
    }
}

// a + b = d, a records of A [0, na) and b of B [0, nb) make the first d records of their merge: a
__device__ __forceinline__ int rs_merge_path(const unsigned long long *ka, const unsigned *ia, int na, const unsigned long long *kb,
                                             const unsigned *ib, int nb, int d)
{
    int lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rs_before(ka[mid], ia[mid], kb[d - 1 - mid], ib[d - 1 - mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// #{x in the sorted run [0, n) : x before (k, i)}
__device__ __forceinline__ int rs_count_before(const unsigned long long *key, const unsigned *idx, int n, unsigned long long k, unsigned i)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rs_before(key[mid], idx[mid], k, i)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace rl
