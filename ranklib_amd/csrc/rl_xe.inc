// rl_xe.inc -- the XE-NDCG listwise objective (rl_set_objective, DESIGN.md 37; Bruch, "An Alternative Cross Entropy Loss for Learning-to-Rank"):
// k_lambda_xe, the third arm of enqueue_lambdas (rl_round.inc), and the trainer's state.  The tile size and the block table are rl_xe_host.h.
// Included by rl_trainer.hip behind rl_kernels_round.inc (block_store_max, kThreads) and rl_device.h (exp_fdlibm_bf, root_hash, feature_key).
//
// Per list, every operation an f64 rounding of its own (-ffp-contract=off), every sum a serial chain from 0.0 in file order (include/rlhip.h):
//     phi_j = 2^(int)l_j - gamma_j,  inv = 1 / sum phi;   rho_j = exp(s_j - max s) / sum exp;   d_j = max(1 - rho_j, 2^-52)
//     a_j = rho_j - phi_j inv,  b_j = a_j / d_j,  B = sum b;   c_j = rho_j (B - b_j),  g_j = c_j / d_j,  G = sum g;   h_j = rho_j (G - g_j)
//     lambda_j = -((a_j + c_j) + h_j),  w_j = rho_j (1 - rho_j);   a list of one document: 0, 0
// O(n) a list, no ranked order.  exp is exp_fdlibm_bf: exp_fdlibm's bits on one instruction stream (rl_device.h; tests/test_gpu_parity.py).
//
// Work split.  The lists never change, so rl_init packs them once (xe_pack): consecutive whole lists into tiles of at most `tile` documents, one
// block of 256 lanes a tile; a list longer than a tile has a block of its own.
//
// Tile path.  The tile's documents live in LDS for the block's lifetime, 44 bytes each: four f64 arrays r (s, then e, then rho), a (phi, then
// phi inv, then a), c (b, then c), g (inv by list, then g), one f64 a list x (max s, then S, B, G), the list of every document (2 bytes) and the
// lists' starts (4 bytes).  Phases alternate between all lanes over the documents (exp, the three divisions: the expensive part, coalesced) and
// one owner lane a list, which adds its list's values in order out of LDS, eight loads in flight ahead of the chain:
//     load s, phi | owners: max, P, list ids | e, phi inv | owners: S | rho, a, b | owners: B | c, g | owners: G | lambda, w -> lw, block max
// A barrier between two phases, eight in all.  No atomics, nothing crosses a block.
//
// Long path.  The block walks its list in chunks of `tile` documents through the same phases, five passes; lane 0 owns the list and carries each
// sum across the chunks in a register, so the chunk size cannot change a bit.  What a later pass needs of a document is KEPT, in the output
// array itself: lw[j] holds (e_j, -) after the second pass and (rho_j, b_j) after the third; a, c, g are one or two operations away from those
// and are computed again (the same instructions on the same values).  Every lane reads back only what it wrote.  One exp a document, as in
// the tile path, and no scratch buffer.
//
//   -Rpass-analysis=kernel-resource-usage, gfx950:
//     k_lambda_xe    TotalSGPRs: 83  VGPRs: 84  AGPRs: 0  ScratchSize: 0  Occupancy [waves/SIMD]: 5  spills: 0  LDS Size [bytes/block]: 23696
//   (the registers, not the LDS, bound a CU at five blocks; what a round waits for is the owners' chains, DESIGN.md 37.4)

namespace rl {

constexpr int kXeLanes = 256;

struct XeArgs {
    const double *scores; const float *labels; const int32_t *qoff; const XeBlock *blocks;
    double2 *lw; double *blockmax;       // blockmax: [blocks of the launch]
    unsigned long long h;                // root_hash(seed ^ kXeSeedTag, round)
    int32_t tile;
};

__device__ __forceinline__ double xe_phi(unsigned long long h, int doc, float label)
{
    const double gamma = (double)(feature_key(h, doc) >> 11) * 0x1.0p-53;
    return bits2d((uint64_t)(1023 + (int)label) << 52) - gamma;       // (0 <= label <= kXeMaxLabel: rl_init)
}
__device__ __forceinline__ double xe_guard(double rho) { return fmax(1.0 - rho, 0x1.0p-52); }

// acc + v[0] + v[1] + ... in that order; the loads of eight values are issued ahead of the dependent additions
__device__ __forceinline__ double xe_chain(const double *v, int n, double acc)
{
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = v[j + u];
#pragma unroll
        for (int u = 0; u < 8; u++) acc = acc + x[u];
    }
    for (; j < n; j++) acc = acc + v[j];
    return acc;
}

// max(m, v[0], v[1], ...), the loads issued ahead in the same way
__device__ __forceinline__ double xe_max(const double *v, int n, double m)
{
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = v[j + u];
#pragma unroll
        for (int u = 0; u < 8; u++) m = x[u] > m ? x[u] : m;
    }
    for (; j < n; j++) m = v[j] > m ? v[j] : m;
    return m;
}

// lane 0's value to every lane of the block, through one LDS word that is free again on return
__device__ __forceinline__ double xe_bcast(double v, double *slot)
{
    if (threadIdx.x == 0) *slot = v;
    __syncthreads();
    v = *slot;
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(kXeLanes) void k_lambda_xe(const XeArgs a)
{
    __shared__ double s_r[kXeTile], s_a[kXeTile], s_c[kXeTile], s_g[kXeTile], s_x[kXeTile];
    __shared__ int32_t s_st[kXeTile + 1];
    __shared__ uint16_t s_lid[kXeTile];
    const int tid = (int)threadIdx.x;
    const int tile = min(a.tile, kXeTile);
    const XeBlock b = a.blocks[blockIdx.x];
    const int base = a.qoff[b.q0], cnt = a.qoff[b.q0 + b.nq] - base;
    double wmax = 0.0;
    if (cnt <= tile) {
        // ---- tile path: b.nq whole lists, cnt documents ----
        for (int l = tid; l <= b.nq; l += kXeLanes) s_st[l] = a.qoff[b.q0 + l] - base;
        for (int j = tid; j < cnt; j += kXeLanes) { s_r[j] = a.scores[base + j]; s_a[j] = xe_phi(a.h, base + j, a.labels[base + j]); }
        __syncthreads();
        for (int l = tid; l < b.nq; l += kXeLanes) {      // owners: max s, P; every document learns its list
            const int j0 = s_st[l], j1 = s_st[l + 1];
            for (int j = j0; j < j1; j++) s_lid[j] = (uint16_t)l;
            s_x[l] = xe_max(s_r + j0, j1 - j0, s_r[j0]);
            s_g[l] = 1.0 / xe_chain(s_a + j0, j1 - j0, 0.0);
        }
        __syncthreads();
        for (int j = tid; j < cnt; j += kXeLanes) {
            const int l = s_lid[j];
            s_r[j] = exp_fdlibm_bf(s_r[j] - s_x[l]);
            s_a[j] = s_a[j] * s_g[l];
        }
        __syncthreads();
        for (int l = tid; l < b.nq; l += kXeLanes) s_x[l] = xe_chain(s_r + s_st[l], s_st[l + 1] - s_st[l], 0.0);       // owners: S
        __syncthreads();
        for (int j = tid; j < cnt; j += kXeLanes) {
            const double rho = s_r[j] / s_x[s_lid[j]];
            const double aj = rho - s_a[j];
            s_r[j] = rho; s_a[j] = aj; s_c[j] = aj / xe_guard(rho);
        }
        __syncthreads();
        for (int l = tid; l < b.nq; l += kXeLanes) s_x[l] = xe_chain(s_c + s_st[l], s_st[l + 1] - s_st[l], 0.0);       // owners: B
        __syncthreads();
        for (int j = tid; j < cnt; j += kXeLanes) {
            const double rho = s_r[j];
            const double cj = rho * (s_x[s_lid[j]] - s_c[j]);
            s_c[j] = cj; s_g[j] = cj / xe_guard(rho);
        }
        __syncthreads();
        for (int l = tid; l < b.nq; l += kXeLanes) s_x[l] = xe_chain(s_g + s_st[l], s_st[l + 1] - s_st[l], 0.0);       // owners: G
        __syncthreads();
        for (int j = tid; j < cnt; j += kXeLanes) {
            const int l = s_lid[j];
            const double rho = s_r[j];
            const double hj = rho * (s_x[l] - s_g[j]);
            const bool one = s_st[l + 1] - s_st[l] <= 1;
            const double lam = one ? 0.0 : -((s_a[j] + s_c[j]) + hj);
            a.lw[base + j] = make_double2(lam, one ? 0.0 : rho * (1.0 - rho));
            wmax = fmax(wmax, fabs(lam));
        }
    } else {
        // ---- long path: one list of cnt > tile documents, lane 0 its owner ----
        double M = 0.0, P = 0.0, S = 0.0, B = 0.0, G = 0.0;
        for (int c0 = 0; c0 < cnt; c0 += tile) {
            const int cn = min(tile, cnt - c0);
            for (int j = tid; j < cn; j += kXeLanes) { s_r[j] = a.scores[base + c0 + j]; s_a[j] = xe_phi(a.h, base + c0 + j, a.labels[base + c0 + j]); }
            __syncthreads();
            if (tid == 0) {
                M = xe_max(s_r, cn, c0 == 0 ? s_r[0] : M);
                P = xe_chain(s_a, cn, P);
            }
            __syncthreads();
        }
        M = xe_bcast(M, s_x);
        const double inv = xe_bcast(1.0 / P, s_x);
        for (int c0 = 0; c0 < cnt; c0 += tile) {
            const int cn = min(tile, cnt - c0);
            for (int j = tid; j < cn; j += kXeLanes) {
                const double e = exp_fdlibm_bf(a.scores[base + c0 + j] - M);
                s_r[j] = e; a.lw[base + c0 + j] = make_double2(e, 0.0);
            }
            __syncthreads();
            if (tid == 0) S = xe_chain(s_r, cn, S);
            __syncthreads();
        }
        S = xe_bcast(S, s_x);
        for (int c0 = 0; c0 < cnt; c0 += tile) {
            const int cn = min(tile, cnt - c0);
            for (int j = tid; j < cn; j += kXeLanes) {
                const int d = base + c0 + j;
                const double rho = a.lw[d].x / S;
                const double bj = (rho - xe_phi(a.h, d, a.labels[d]) * inv) / xe_guard(rho);
                s_c[j] = bj; a.lw[d] = make_double2(rho, bj);
            }
            __syncthreads();
            if (tid == 0) B = xe_chain(s_c, cn, B);
            __syncthreads();
        }
        B = xe_bcast(B, s_x);
        for (int c0 = 0; c0 < cnt; c0 += tile) {
            const int cn = min(tile, cnt - c0);
            for (int j = tid; j < cn; j += kXeLanes) {
                const double2 rb = a.lw[base + c0 + j];
                s_g[j] = (rb.x * (B - rb.y)) / xe_guard(rb.x);
            }
            __syncthreads();
            if (tid == 0) G = xe_chain(s_g, cn, G);
            __syncthreads();
        }
        G = xe_bcast(G, s_x);
        for (int c0 = 0; c0 < cnt; c0 += tile) for (int j = tid; j < min(tile, cnt - c0); j += kXeLanes) {       // (chunked like the passes above: a lane meets its own documents)
            const int d = base + c0 + j;
            const double2 rb = a.lw[d];
            const double rho = rb.x;
            const double aj = rho - xe_phi(a.h, d, a.labels[d]) * inv;
            const double cj = rho * (B - rb.y);
            const double hj = rho * (G - cj / xe_guard(rho));
            const double lam = -((aj + cj) + hj);
            a.lw[d] = make_double2(lam, rho * (1.0 - rho));
            wmax = fmax(wmax, fabs(lam));
        }
    }
    block_store_max(wmax, a.blockmax);
}

// the trainer's XE-NDCG state (rl_trainer::xe); `on` and the seed are rl_set_objective's, the block table init_xe's (rl_init.inc)
struct XeState {
    bool on = false;
    uint64_t seed = 0;
    int32_t tile = kXeTile, n_blocks = 0;
    XeBlock *d_blocks = nullptr;
};

// one launch: the lambdas and weights of round `round` for the lists behind `blocks`
static void launch_lambda_xe(hipStream_t s, const double *scores, const float *labels, const int32_t *qoff, const XeBlock *blocks, int n_blocks, int tile,
                             uint64_t seed, int round, double2 *lw, double *blockmax)
{
    const XeArgs a{scores, labels, qoff, blocks, lw, blockmax, root_hash(seed ^ kXeSeedTag, round), tile};
    hipLaunchKernelGGL(k_lambda_xe, dim3((unsigned)n_blocks), dim3(kXeLanes), 0, s, a);
}

}  // namespace rl
