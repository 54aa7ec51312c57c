// rl_perm.inc -- the Fisher randomisation test of the Analyzer (stats/RandomPermutationTest.java:23-53) on gfx950.  DESIGN.md 18.
//
// The Java draws nPermutation sign vectors and, for each, sums two length-n double arrays serially (BasicStats.mean: += from 0.0 in
// array order, one division by the length).  Work is nPermutation x n x targets f64 adds in dependent chains; the chains of different
// permutations are independent, so one lane owns one permutation:
//
//   k_perm_test   gridDim.y = target.  Lane i handles permutation perm_begin + i.  Its bits come from ONE java.util.Random(seed) per
//                 target: permutation p takes the nextDouble draws [p D, (p + 1) D), D = n / 10 + 1 (randomBitVector :60-73), each draw
//                 two LCG steps, so the lane composes x -> a x + c (mod 2^48) with itself k = 2 D p times by square-and-multiply and
//                 starts there.  (int)(1024 * nextDouble()) == next(26) >> 16 == bits 47..38 of the state after the draw's first
//                 step (tests/test_analyzer_cpu.py holds the two forms equal); bit q of the chunk, most significant first, swaps
//                 b[j] and t[j].  Two running sums from 0.0, plain adds, then a correctly rounded division by (double)n each, fabs
//                 of the difference, >= trueDiff.  One ballot + popcount per wavefront and one integer atomic per wavefront: the
//                 count is exact and order-free.
//
// Every lane reads the same b[j], t[j] at the same step: the index is wave-uniform and nothing in the kernel writes the inputs before
// the loop ends, so the loads are scalar loads (ten elements of each array per chunk, fetched ahead of the adds that use them); no LDS
// tile, no barrier, no tile-size edge.  Built with -ffp-contract=off like the rest.  There is no CPU fallback: the host loop at the end
// of this file is tools/perm_bench.py's yardstick and a debug entry, nothing the Analyzer calls.
#include <chrono>
#include <cstdint>
#include <string>

namespace rl {

constexpr uint64_t kLcgA = 0x5DEECE66DULL, kLcgC = 0xBULL, kLcgMask = (1ULL << 48) - 1;

// k steps of the LCG as one affine map x -> A x + C (mod 2^48): square-and-multiply over the bits of k (64-bit wrap keeps the low 48 bits)
__host__ __device__ __forceinline__ void lcg_jump(uint64_t k, uint64_t &A, uint64_t &C)
{
    uint64_t ra = 1, rc = 0, ba = kLcgA, bc = kLcgC;
    while (k) {
        if (k & 1) { ra = ba * ra; rc = ba * rc + bc; }
        bc = ba * bc + bc; ba = ba * ba;
        k >>= 1;
    }
    A = ra & kLcgMask; C = rc & kLcgMask;
}

__device__ __forceinline__ uint64_t lcg_step(uint64_t s) { return (s * kLcgA + kLcgC) & kLcgMask; }

// state0: the scrambled seed ((seed ^ 0x5DEECE66D) & mask), the state before the first step
__global__ __launch_bounds__(kThreads) void k_perm_test(const double *__restrict__ base, const double *__restrict__ targets,
                                                        const double *__restrict__ true_diff, unsigned long long *count, double *pdiff,
                                                        int n, uint64_t state0, int64_t perm_begin, int64_t perm_count)
{
    const int tgt = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < perm_count;
    if (!__ballot(live)) return;                            // a wavefront past the end (uniform)
    const double *__restrict__ t = targets + (size_t)tgt * n;
    const int full = n / 10, rem = n - full * 10;
    const uint64_t D2 = 2 * ((uint64_t)full + 1);           // LCG steps per permutation
    uint64_t A, C;
    lcg_jump((uint64_t)(perm_begin + (live ? i : 0)) * D2, A, C);      // lanes past the end walk along, unread
    uint64_t s = (A * state0 + C) & kLcgMask;
    double sb = 0.0, st = 0.0;
    for (int c = 0; c < full; c++) {
        s = lcg_step(s);
        const uint32_t x = (uint32_t)(s >> 38);             // (int)(1024 * nextDouble())
        s = lcg_step(s);                                    // the draw's next(27)
        const int j0 = c * 10;
#pragma unroll
        for (int q = 0; q < 10; q++) {
            const double bv = base[j0 + q], tv = t[j0 + q];
            const bool swap = (x >> (9 - q)) & 1u;
            sb += swap ? tv : bv;
            st += swap ? bv : tv;
        }
    }
    if (rem) {                                              // n % 10 == 0: the Java's last draw is taken and never used, nothing to do
        s = lcg_step(s);
        const uint32_t x = (uint32_t)(s >> 38);
        const int j0 = full * 10;
        for (int q = 0; q < rem; q++) {
            const double bv = base[j0 + q], tv = t[j0 + q];
            const bool swap = (x >> (9 - q)) & 1u;
            sb += swap ? tv : bv;
            st += swap ? bv : tv;
        }
    }
    const double pd = fabs(sb / (double)n - st / (double)n);
    if (live && pdiff) pdiff[(size_t)tgt * perm_count + i] = pd;
    const bool hit = live && pd >= true_diff[tgt];          // a NaN on either side does not count
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(count + tgt, (unsigned long long)__popcll(m));
}

// calibration (tools/perm_bench.py): one wavefront, one dependent chain of 64 * rounds f64 adds per lane (64 adds between two branches,
// so the loop's own instructions do not set the figure)
__global__ void k_perm_calib(double *io, int64_t rounds)
{
    double s = io[threadIdx.x];
    const double x = io[kWave + threadIdx.x];
    for (int64_t a = 0; a < rounds; a++) {
#pragma unroll
        for (int u = 0; u < 64; u++) s += x;
    }
    io[threadIdx.x] = s;
}

static double perm_mean(const double *v, int n)
{   // BasicStats.mean :7-16
    double mean = 0.0;
    for (int i = 0; i < n; i++) mean += v[i];
    return mean / n;
}

static double perm_next_double(JavaRandom &r)
{   // Random.nextDouble: (((long) next(26) << 27) + next(27)) * 0x1.0p-53
    const int64_t hi = (int64_t)r.next(26) << 27;
    return (double)(hi + r.next(27)) * 0x1.0p-53;
}

// RandomPermutationTest.test :33-52 as written, on the host, one Random(seed) for the call: digit strings, copies into pb / pt, two means
static int64_t perm_host_literal(const double *b, const double *t, int n, int64_t seed, int64_t np, double trueDiff)
{
    JavaRandom r(seed);
    std::vector<double> pb((size_t)n), pt((size_t)n);
    std::string bits;
    int64_t count = 0;
    for (int64_t i = 0; i < np; i++) {
        bits.clear();
        for (int c = 0; c < n / 10 + 1; c++) {
            const int x = (int)((1 << 10) * perm_next_double(r));
            for (int q = 9; q >= 0; q--) bits.push_back(((x >> q) & 1) ? '1' : '0');
        }
        for (int j = 0; j < n; j++) {
            if (bits[(size_t)j] == '0') { pb[j] = b[j]; pt[j] = t[j]; }
            else { pb[j] = t[j]; pt[j] = b[j]; }
        }
        const double pDiff = std::fabs(perm_mean(pb.data(), n) - perm_mean(pt.data(), n));
        if (pDiff >= trueDiff) count++;
    }
    return count;
}

}  // namespace rl

extern "C" {

int rl_perm_test(int device, const double *base, const double *targets, int n, int n_targets, int64_t seed, int64_t perm_begin,
                 int64_t perm_count, int64_t *out_count, double *out_true_diff, double *out_pdiff)
{
    if (!base || !targets || !out_count || !out_true_diff) return fail(RL_ERR_INVALID, "rl_perm_test: null argument");
    if (n < 1) return fail(RL_ERR_INVALID, "rl_perm_test: n must be >= 1 (BasicStats.mean refuses an empty array)");
    if (n_targets < 1) return fail(RL_ERR_INVALID, "rl_perm_test: n_targets must be >= 1");
    if (n_targets > 65535) return fail(RL_ERR_INVALID, "rl_perm_test: at most 65535 targets per call");
    if (perm_count < 1) return fail(RL_ERR_INVALID, "rl_perm_test: perm_count must be >= 1");
    if (perm_count > INT32_MAX) return fail(RL_ERR_INVALID, "rl_perm_test: perm_count above 2^31 - 1: split the run with perm_begin");
    if (perm_begin < 0) return fail(RL_ERR_INVALID, "rl_perm_test: perm_begin must be >= 0");
    const int64_t D2 = 2 * ((int64_t)(n / 10) + 1);
    if (perm_begin > INT64_MAX - perm_count || perm_begin + perm_count > INT64_MAX / D2)
        return fail(RL_ERR_INVALID, "rl_perm_test: (perm_begin + perm_count) * 2 * (n / 10 + 1) LCG steps overflow 63 bits");
    int rc = open_device(device, true);
    if (rc) return rc;
    std::vector<double> td((size_t)n_targets);
    const double mb = perm_mean(base, n);
    for (int k = 0; k < n_targets; k++) td[k] = std::fabs(mb - perm_mean(targets + (size_t)k * n, n));
    DevPool buf;
    double *d_b = nullptr, *d_t = nullptr, *d_td = nullptr, *d_pd = nullptr; unsigned long long *d_cnt = nullptr;
    RL_HIP(buf.alloc(&d_b, (size_t)n));
    RL_HIP(buf.alloc(&d_t, (size_t)n * n_targets));
    RL_HIP(buf.alloc(&d_td, (size_t)n_targets));
    RL_HIP(buf.alloc(&d_cnt, (size_t)n_targets));
    if (out_pdiff) RL_HIP(buf.alloc(&d_pd, (size_t)n_targets * (size_t)perm_count));
    RL_HIP(hipMemcpy(d_b, base, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_t, targets, (size_t)n * n_targets * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_td, td.data(), (size_t)n_targets * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemset(d_cnt, 0, (size_t)n_targets * sizeof(unsigned long long)));
    const uint64_t state0 = JavaRandom(seed).seed;
    const unsigned gx = (unsigned)((perm_count + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_perm_test, dim3(gx, (unsigned)n_targets), dim3(kThreads), 0, 0, d_b, d_t, d_td, d_cnt, d_pd, n, state0, perm_begin,
                       perm_count);
    RL_HIP(hipGetLastError());
    std::vector<unsigned long long> cnt((size_t)n_targets);
    RL_HIP(hipMemcpy(cnt.data(), d_cnt, (size_t)n_targets * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (out_pdiff) RL_HIP(hipMemcpy(out_pdiff, d_pd, (size_t)n_targets * (size_t)perm_count * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < n_targets; k++) { out_count[k] = (int64_t)cnt[k]; out_true_diff[k] = td[k]; }
    return RL_OK;
}

int rl_debug_perm_calib(int device, const double *base, const double *target, int n, int64_t seed, int64_t perm_count, int64_t chain_adds,
                        double *add_ns, double *host_ms, int64_t *host_count)
{
    if (!add_ns || !host_ms || !host_count) return fail(RL_ERR_INVALID, "rl_debug_perm_calib: null argument");
    if (chain_adds < 1) return fail(RL_ERR_INVALID, "rl_debug_perm_calib: chain_adds must be >= 1");
    *add_ns = 0.0; *host_ms = 0.0; *host_count = 0;
    if (base && target) {
        if (n < 1 || perm_count < 1) return fail(RL_ERR_INVALID, "rl_debug_perm_calib: n and perm_count must be >= 1");
        const double trueDiff = std::fabs(perm_mean(base, n) - perm_mean(target, n));
        const auto t0 = std::chrono::steady_clock::now();
        *host_count = perm_host_literal(base, target, n, seed, perm_count, trueDiff);
        *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    int rc = open_device(device, true);
    if (rc) return rc;
    DevPool buf;
    double *d_io = nullptr;
    RL_HIP(buf.alloc(&d_io, (size_t)2 * kWave));
    std::vector<double> io((size_t)2 * kWave, 1.0);
    RL_HIP(hipMemcpy(d_io, io.data(), io.size() * sizeof(double), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    RL_HIP(hipEventCreate(&e0));
    RL_HIP(hipEventCreate(&e1));
    float ms[3] = {0.f, 0.f, 0.f};
    for (int pass = 0; pass < 3; pass++) {                 // a warm-up, then the chain at one and two lengths: the difference has no launch in it
        const int64_t rounds = (pass == 2 ? 2 : 1) * ((chain_adds + 63) / 64);
        (void)hipEventRecord(e0, 0);
        hipLaunchKernelGGL(k_perm_calib, dim3(1), dim3(kWave), 0, 0, d_io, rounds);
        (void)hipEventRecord(e1, 0);
        hipError_t e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[pass], e0, e1);
        if (e != hipSuccess) {
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
            return fail(RL_ERR_HIP, std::string("rl_debug_perm_calib: ") + hipGetErrorString(e));
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *add_ns = ((double)ms[2] - (double)ms[1]) * 1e6 / (double)(64 * ((chain_adds + 63) / 64));
    return RL_OK;
}

}  // extern "C"
