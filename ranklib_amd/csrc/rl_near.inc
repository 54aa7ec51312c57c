// rl_near.inc -- nearest neighbours in leaf space (rl_model_predict_neighbours, DESIGN.md 41): for every query row the k reference rows
// that reach the same leaf in the most trees of a window -- the proximity of random-forest practice.  Included at the end of
// rl_trainer.hip, after rl_leaves.inc: both sets are walked by its kernels (LeavesWalk) into device buffers of leaf numbers, uint16 BY ROW,
// [rows][ld], ld = the window rounded up to 4 trees.  By row because the match reads TWO TREES OF ONE DOCUMENT AS ONE 32-BIT WORD: a staged
// row is a run of words, a lane's operands are 128-bit LDS reads of 8 trees each, and no transpose happens anywhere.  Two kernels:
//   k_near_match  block (x, y): queries [64 x, 64 x + 64) against the reference tiles of split y, 128 references a step.  Per step the
//                 window goes through LDS 64 trees at a time; lane (a, b) of the 16 x 16 grid holds the 4 x 8 counters of queries a + 16 i and
//                 references b + 16 j, as a GEMM micro-kernel holds its accumulators.  A word of two trees costs xor, packed 16-bit min
//                 against 1, packed 16-bit add: MISMATCHES are counted, so the zeroed tail of a window (an odd last tree, the words to the
//                 end of the chunk) adds nothing, and shared = trees - mismatches.  After the window the counters go to LDS (where the staged
//                 words were) and lane q < 64 is query q's OWNER: it runs along its row and inserts what beats its k-th key into its sorted
//                 list in LDS.  No atomic: a list has one writer.  The lists leave as 64-bit keys, [split][query][k].
//   k_near_merge  a wavefront per query merges the splits' sorted lists and the running list of earlier bands by k rounds of a wave-wide
//                 maximum; the keys are distinct, so the lane whose head won steps on.
// The order (shared descending, index ascending) is total, so tiles, splits, bands and chunks cannot show in the result.
#include "rl_near_host.h"

namespace rl {

// acc += (a != b) per 16-bit half, three instructions a word of two trees.  Stated as instructions: from `min(x, 1)` on a vector of two
// u16 the compiler makes two compares, two selects and a v_perm_b32, twice the work.
__device__ __forceinline__ unsigned near_count(unsigned acc, unsigned a, unsigned b, unsigned ones)
{
    unsigned d;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(d) : "v"(a ^ b), "v"(ones));
    asm("v_pk_add_u16 %0, %1, %2" : "=v"(acc) : "v"(acc), "v"(d));
    return acc;
}

// a word of a row of leaf numbers with the trees at and after nt zeroed; w: the word's index in the row
__device__ __forceinline__ unsigned near_mask_word(unsigned v, int w, int nt)
{
    return 2 * w + 1 < nt ? v : (2 * w < nt ? (v & 0xffffu) : 0u);
}

// rows [r0, r0 + nrows) of L [n][ld] (zeros past n), words [w0, w0 + kNearCW) -> s [nrows][kNearRowW]; a thread moves 4 trees, 16 threads a row's 128 bytes
__device__ __forceinline__ void near_stage(unsigned *s, const uint16_t *L, int64_t n, int64_t ld, int64_t r0, int nrows, int w0, int nt, int tid)
{
    for (int e = tid; e < nrows * (kNearCW / 2); e += kNearThreads) {
        const int row = e / (kNearCW / 2), w = w0 + 2 * (e % (kNearCW / 2));
        uint2 v = make_uint2(0u, 0u);
        if (r0 + row < n && 2 * w < nt) v = *(const uint2 *)(L + (size_t)(r0 + row) * (size_t)ld + (size_t)(2 * w));      // (ld % 4 == 0: inside the row, on 8 bytes)
        v.x = near_mask_word(v.x, w, nt);
        v.y = near_mask_word(v.y, w + 1, nt);
        *(uint2 *)(s + row * kNearRowW + (w - w0)) = v;
    }
}

// Lq [nq][ld], Lr [nr][ld]: this query chunk's and this reference band's leaf numbers; q_base, r_base: the call's index of their first
// rows.  parts [gridDim.y][nq][k].  matrix (may be null) [nq][nr] of this chunk and band.
__global__ __launch_bounds__(kNearThreads) void k_near_match(const uint16_t *Lq, int64_t nq, const uint16_t *Lr, int64_t nr, int64_t ld, int nt, int k,
                                                             int skip_same, int64_t q_base, int64_t r_base, int64_t tiles_per_split,
                                                             unsigned long long *parts, uint16_t *matrix)
{
    extern __shared__ unsigned char near_raw[];
    unsigned *sQ = (unsigned *)near_raw;                                       // [kNearQT][kNearRowW]
    unsigned *sR = sQ + kNearQT * kNearRowW;                                   // [kNearRT][kNearRowW]
    uint16_t *sC = (uint16_t *)near_raw;                                       // [kNearQT][kNearCntRow] the tile's shared counts, once the window is through
    unsigned long long *sK = (unsigned long long *)(sQ + (kNearQT + kNearRT) * kNearRowW);      // [k][kNearQT] the lists, position-major: the owners' lanes side by side
    const int tid = threadIdx.x, a = tid >> 4, b = tid & 15;
    const unsigned ones = 0x00010001u;
    const int64_t q0 = (int64_t)blockIdx.x * kNearQT;
    const int64_t r_tiles = (nr + kNearRT - 1) / kNearRT;
    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_split, tile1 = min(r_tiles, tile0 + tiles_per_split);
    for (int e = tid; e < k * kNearQT; e += kNearThreads) sK[e] = 0ull;
    for (int64_t tile = tile0; tile < tile1; tile++) {
        const int64_t r0 = tile * kNearRT;
        unsigned acc[kNearMQ][kNearMR];                                        // two u16 counters each: the mismatches at the even and at the odd trees
#pragma unroll
        for (int i = 0; i < kNearMQ; i++)
#pragma unroll
            for (int j = 0; j < kNearMR; j++) acc[i][j] = 0u;
        for (int t0 = 0; t0 < nt; t0 += kNearTC) {
            __syncthreads();                                                   // the chunk before is counted; the tile before is scanned
            near_stage(sQ, Lq, nq, ld, q0, kNearQT, t0 / 2, nt, tid);
            near_stage(sR, Lr, nr, ld, r0, kNearRT, t0 / 2, nt, tid);
            __syncthreads();
            const int n4 = (min(kNearTC, nt - t0) + 7) / 8;                    // 128-bit reads that hold a tree of the window
            for (int c = 0; c < n4; c++) {
                uint4 q[kNearMQ], r[kNearMR];
#pragma unroll
                for (int i = 0; i < kNearMQ; i++) q[i] = *(const uint4 *)(sQ + (a + 16 * i) * kNearRowW + 4 * c);
#pragma unroll
                for (int j = 0; j < kNearMR; j++) r[j] = *(const uint4 *)(sR + (b + 16 * j) * kNearRowW + 4 * c);
#pragma unroll
                for (int i = 0; i < kNearMQ; i++)
#pragma unroll
                    for (int j = 0; j < kNearMR; j++) {
                        acc[i][j] = near_count(acc[i][j], q[i].x, r[j].x, ones);
                        acc[i][j] = near_count(acc[i][j], q[i].y, r[j].y, ones);
                        acc[i][j] = near_count(acc[i][j], q[i].z, r[j].z, ones);
                        acc[i][j] = near_count(acc[i][j], q[i].w, r[j].w, ones);
                    }
            }
        }
        __syncthreads();                                                       // the staged words are read: their place takes the counts
#pragma unroll
        for (int i = 0; i < kNearMQ; i++)
#pragma unroll
            for (int j = 0; j < kNearMR; j++)
                sC[(a + 16 * i) * kNearCntRow + b + 16 * j] = (uint16_t)(nt - (int)((acc[i][j] & 0xffffu) + (acc[i][j] >> 16)));
        __syncthreads();
        const int nrt = (int)min((int64_t)kNearRT, nr - r0);
        if (tid < kNearQT && q0 + tid < nq) {                                  // the owner of query tid
            const int64_t same = skip_same ? q_base + q0 + tid - (r_base + r0) : -1;      // the column of the reference with the query's own index
            unsigned long long kth = sK[(k - 1) * kNearQT + tid];
            for (int col = 0; col < nrt; col++) {
                const unsigned cnt = sC[tid * kNearCntRow + col];
                if (cnt < (unsigned)(kth >> 32) || col == same) continue;
                const unsigned long long key = ((unsigned long long)cnt << 32) | (unsigned)~(unsigned)(r_base + r0 + col);
                if (key <= kth) continue;
                int p = k - 1;
                for (; p > 0; p--) {
                    const unsigned long long up = sK[(p - 1) * kNearQT + tid];
                    if (up >= key) break;
                    sK[p * kNearQT + tid] = up;
                }
                sK[p * kNearQT + tid] = key;
                kth = sK[(k - 1) * kNearQT + tid];
            }
        }
        if (matrix)
            for (int e = tid; e < kNearQT * kNearRT; e += kNearThreads) {
                const int row = e / kNearRT, col = e % kNearRT;
                if (q0 + row < nq && col < nrt) matrix[(size_t)(q0 + row) * (size_t)nr + (size_t)(r0 + col)] = sC[row * kNearCntRow + col];
            }
    }
    __syncthreads();
    for (int e = tid; e < k * kNearQT; e += kNearThreads) {
        const int p = e / kNearQT, row = e % kNearQT;
        if (q0 + row < nq) parts[((size_t)blockIdx.y * (size_t)nq + (size_t)(q0 + row)) * (size_t)k + p] = sK[e];
    }
}

// A wavefront per query: lane l < splits holds the head of parts[l][query], lane `splits` the head of prev[query] (the earlier bands), all
// sorted descending; k rounds of a wave-wide maximum.  next [nq][k] the merged keys; index, shared [nq][k] what they say.
__global__ __launch_bounds__(kNearThreads) void k_near_merge(const unsigned long long *parts, int splits, const unsigned long long *prev, int64_t nq, int k,
                                                             unsigned long long *next, int32_t *index, int32_t *shared)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t q = (int64_t)blockIdx.x * (kNearThreads / kWave) + threadIdx.x / kWave;
    if (q >= nq) return;                                                       // (the whole wavefront)
    const unsigned long long *list = lane < splits ? parts + ((size_t)lane * (size_t)nq + (size_t)q) * (size_t)k
                                                   : (lane == splits ? prev + (size_t)q * (size_t)k : nullptr);
    int head = 0;
    unsigned long long cur = list ? list[0] : 0ull;
    for (int i = 0; i < k; i++) {
        unsigned long long best = cur;
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d, kWave);
            best = o > best ? o : best;
        }
        if (lane == 0) {
            next[(size_t)q * k + i] = best;
            index[(size_t)q * k + i] = best ? (int32_t)~(unsigned)best : -1;
            shared[(size_t)q * k + i] = (int32_t)(best >> 32);
        }
        if (best != 0ull && cur == best) { head++; cur = head < k ? list[head] : 0ull; }
    }
}

static thread_local double g_near_walk_ms = 0.0, g_near_match_ms = 0.0;        // this thread's last rl_model_predict_neighbours call, device events

}  // namespace rl

extern "C" {

int rl_model_predict_neighbours(rl_model *m, const float *Xq, int64_t nq, const float *Xr, int64_t nr, int32_t row_stride, int32_t first_tree,
                                int32_t n_trees, int32_t k, int32_t flags, int64_t scratch_bytes, int32_t *out_index, int32_t *out_shared,
                                uint16_t *out_matrix)
{
    static const std::string w = "rl_model_predict_neighbours: ";
    static_assert(RL_NEAR_MAX_K == kNearMaxK && RL_NEAR_SKIP_SAME_INDEX == 1, "rl_near_host.h restates these");
    std::string err;
    int rc = near_check(w, m ? (int64_t)m->trees.size() : -1, Xq, nq, Xr, nr, row_stride, first_tree, &n_trees, k, flags, scratch_bytes, out_index,
                        out_shared, err);
    if (rc) return fail(rc, err);
    for (int32_t t = first_tree; t < first_tree + n_trees; t++)
        if (leaves_count(m->trees[t]) > kLeavesMax)
            return fail(RL_ERR_UNSUPPORTED, w + "tree " + std::to_string(t) + " has " + std::to_string(leaves_count(m->trees[t])) +
                                                " leaves: a leaf number is 16 bits, 65536 leaves at most");
    g_near_walk_ms = g_near_match_ms = 0.0;
    RL_HIP(hipSetDevice(m->device));
    const int64_t ld = near_ld(n_trees);
    const NearPlan plan = near_plan(nq, nr, (int64_t)row_stride * 4 + ld * 2, scratch_bytes);
    DevPool pool;
    LeavesWalk lw;
    if ((rc = lw.open(m, pool, w, row_stride, first_tree, n_trees))) return rc;
    float *dXq = nullptr, *dXr = nullptr;
    uint16_t *dLq = nullptr, *dLr = nullptr, *dM = nullptr;
    unsigned long long *d_parts = nullptr, *d_run[2] = {nullptr, nullptr};
    int32_t *d_index = nullptr, *d_shared = nullptr;
    RL_HIP(pool.alloc(&dXq, (size_t)plan.q_chunk * row_stride));
    RL_HIP(pool.alloc(&dXr, (size_t)plan.r_band * row_stride));
    RL_HIP(pool.alloc(&dLq, (size_t)plan.q_chunk * ld));
    RL_HIP(pool.alloc(&dLr, (size_t)plan.r_band * ld));
    RL_HIP(pool.alloc(&d_parts, (size_t)plan.part_rows * k));
    RL_HIP(pool.alloc(&d_run[0], (size_t)plan.q_chunk * k));
    RL_HIP(pool.alloc(&d_run[1], (size_t)plan.q_chunk * k));
    RL_HIP(pool.alloc(&d_index, (size_t)plan.q_chunk * k));
    RL_HIP(pool.alloc(&d_shared, (size_t)plan.q_chunk * k));
    if (out_matrix) RL_HIP(pool.alloc(&dM, (size_t)plan.q_chunk * plan.r_band));
    const size_t lds = near_lds(k);
    RL_HIP(hipFuncSetAttribute((const void *)k_near_match, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    StageEvents ev;
    RL_HIP(ev.create());
    auto elapsed = [&](int from, double *ms) -> int {
        float t = 0.f;
        RL_HIP(hipEventElapsedTime(&t, ev.e[from], ev.e[from + 1]));
        *ms += (double)t;
        return RL_OK;
    };
    for (int64_t q0 = 0; q0 < nq; q0 += plan.q_chunk) {
        const int64_t nqc = std::min(plan.q_chunk, nq - q0), q_tiles = (nqc + kNearQT - 1) / kNearQT;
        RL_HIP(hipMemcpy(dXq, Xq + (size_t)q0 * row_stride, (size_t)nqc * row_stride * sizeof(float), hipMemcpyHostToDevice));
        RL_HIP(hipMemset(d_run[0], 0, (size_t)nqc * k * sizeof(unsigned long long)));      // every slot empty
        RL_HIP(hipEventRecord(ev.e[0], 0));
        if ((rc = lw.launch(false, dXq, nqc, dLq, ld))) return rc;
        RL_HIP(hipEventRecord(ev.e[1], 0));
        RL_HIP(hipEventSynchronize(ev.e[1]));
        if ((rc = elapsed(0, &g_near_walk_ms))) return rc;
        int cur = 0;
        for (int64_t r0 = 0; r0 < nr; r0 += plan.r_band) {
            const int64_t nrb = std::min(plan.r_band, nr - r0);
            int64_t per = 0, splits = 0;
            near_splits(q_tiles, (nrb + kNearRT - 1) / kNearRT, &per, &splits);
            RL_HIP(hipMemcpy(dXr, Xr + (size_t)r0 * row_stride, (size_t)nrb * row_stride * sizeof(float), hipMemcpyHostToDevice));
            RL_HIP(hipEventRecord(ev.e[0], 0));
            if ((rc = lw.launch(false, dXr, nrb, dLr, ld))) return rc;
            RL_HIP(hipEventRecord(ev.e[1], 0));
            hipLaunchKernelGGL(k_near_match, dim3((unsigned)q_tiles, (unsigned)splits), dim3(kNearThreads), lds, 0, (const uint16_t *)dLq, nqc,
                               (const uint16_t *)dLr, nrb, ld, (int)n_trees, (int)k, (int)(flags & RL_NEAR_SKIP_SAME_INDEX), q0, r0, per, d_parts, dM);
            RL_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_near_merge, dim3((unsigned)((nqc + kNearThreads / kWave - 1) / (kNearThreads / kWave))), dim3(kNearThreads), 0, 0,
                               (const unsigned long long *)d_parts, (int)splits, (const unsigned long long *)d_run[cur], nqc, (int)k, d_run[cur ^ 1],
                               d_index, d_shared);
            RL_HIP(hipGetLastError());
            RL_HIP(hipEventRecord(ev.e[2], 0));
            RL_HIP(hipEventSynchronize(ev.e[2]));                              // the next band overwrites dXr and dLr
            if ((rc = elapsed(0, &g_near_walk_ms)) || (rc = elapsed(1, &g_near_match_ms))) return rc;
            if (out_matrix)
                RL_HIP(hipMemcpy2D(out_matrix + (size_t)q0 * (size_t)nr + (size_t)r0, (size_t)nr * 2, dM, (size_t)nrb * 2, (size_t)nrb * 2, (size_t)nqc,
                                   hipMemcpyDeviceToHost));
            cur ^= 1;
        }
        RL_HIP(hipMemcpy(out_index + (size_t)q0 * k, d_index, (size_t)nqc * k * sizeof(int32_t), hipMemcpyDeviceToHost));
        RL_HIP(hipMemcpy(out_shared + (size_t)q0 * k, d_shared, (size_t)nqc * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    m->last_path = RL_MODEL_PATH_NEIGHBOURS;
    return RL_OK;
}

int rl_debug_neighbours_times(double *walk_ms, double *match_ms)
{
    if (!walk_ms || !match_ms) return fail(RL_ERR_INVALID, "rl_debug_neighbours_times: null argument");
    *walk_ms = g_near_walk_ms;
    *match_ms = g_near_match_ms;
    return RL_OK;
}

}  // extern "C"
