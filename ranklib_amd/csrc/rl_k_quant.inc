// rl_k_quant.inc -- K1b: lambda -> order-independent fixed point (DESIGN.md 3 "exact sums"; the reference has no such step, it sums doubles in
// sample order).  quant_exponents, rint_ll_small and k_quantize; the root pass of k_hist that quantises on the fly uses the first two.
// Included by rl_kernels_round.inc; needs nothing of that file and none of the other pieces.

namespace rl {

// ------------------------------------------------------------------------------------------------
// K1b: fixed-point quantisation.  q = rint(lambda * 2^E) with E chosen from max|lambda| so that one LDS
// accumulator (<= 2^kLog2Chunk addends) cannot overflow int64.  Integer sums are associative: every
// histogram value below is independent of accumulation order, thread count and GPU count.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void quant_exponents(unsigned long long maxbits, int N, int &E, int &E2)
{
    if (maxbits == 0) { E = 0; E2 = 0; return; }
    const double m = bits2d(maxbits);
    const int M = ilogb(m) + 1;                      // m < 2^M
    int lgN = 0;
    while ((1LL << lgN) < (long long)N + 1) lgN++;
    E = 62 - kLog2Chunk - M;
    E2 = 61 - lgN - 2 * M;
}

// (long long)rint(x) for |x| < 2^51 by one addition: x + 1.5 * 2^52 is rounded to an integer (nearest, ties to even -- the rounding of
// __double2ll_rn) and the integer sits in the low mantissa bits.  The library conversion is a dozen instructions (there is no f64 -> i64
// convert on gfx950); the root pass that quantises on the fly runs it once per document and feature group.  |q| < 2^48 by the choice of E
// (quant_exponents); r is NOT small on small data (r < 2^(61 - lg N)) and keeps the library conversion.
__device__ __forceinline__ long long rint_ll_small(double x)
{
    const double magic = 6755399441055744.0;        // 1.5 * 2^52
    return (long long)(d2bits(x + magic) - d2bits(magic));
}

__global__ __launch_bounds__(kThreads) void k_quantize(const Ctx c)
{
    int E, E2;
    quant_exponents(c.st->maxabs_bits, c.Nglobal, E, E2);      // the GLOBAL document count: lambda^2 sums are all-reduced as raw integers
    long long acc = 0;
    for (int k = blockIdx.x * kThreads + threadIdx.x; k < c.N; k += gridDim.x * kThreads) {
        const double l = c.lw[k].x;
        c.q[k] = __double2ll_rn(ldexp(l, E));
        const long long r = __double2ll_rn(ldexp(l * l, E2));
        c.r[k] = r;
        acc += r;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    __shared__ long long part[4];
    if (lane_id() == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd((unsigned long long *)&c.st->root_sq, (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
        if (blockIdx.x == 0) { c.st->E = E; c.st->E2 = E2; }
    }
}

}  // namespace rl
