// rl_rn.inc -- RankNet and LambdaRank training (-ranker 1 / 5, learning/neuralnet/RankNet.java learn :290-334, LambdaRank.java, Neuron.java
// computeDelta / updateDelta / updateWeight :97-167) on gfx950; included at the end of rl_ca.hip.  The handle holds a ranking context (LinCtx, rl_linear.inc) and ranks
// with k_ca_trials (T = 1 on the cache as it is).
//
// The network is rl_net.inc's: layer 0 = F inputs and a bias neuron, layers 1 .. L - 1 hidden, layer L one output neuron; the weights
// in rl_net_create's layout (per layer a row-major [n_l][n_{l-1} + 1], the bias last).  learn() walks the lists in order; per list of n
// documents (DESIGN.md 16):
//     batchFeedForward      the outputs of every neuron for every document with the weights as they are, kept; beside each output o the
//                           value d(o) = s * (1.0 - s), s = 1 / (1 + exp(-o)) (LogiFunction.computeDerivative of an output: a second
//                           logistic, as written), which depends on o alone
//     batchBackPropagate    one step per document i = 0 .. n - 1, in order; the pairs of i are the j with label_i > label_j, ascending
//         output neuron     pij_j = 1 / (1 + exp(o_i - o_j));  delta_i = 0.0, += pij_j in order, *= d(o_i);  deltas_j = pij_j * d(o_j)
//         hidden, last to first, neuron h:  errorSum_j = 0.0, += target.deltas_j * w over the next layer;  deltas_j = errorSum_j * d(h_j);
//                           delta_i = 0.0, += target.delta_i * w, *= d(h_i)   (only with at least one pair: else it stays 0)
//         every weight      sum_j = 0.0, += deltas_j * source.out(j) in order;  w += lr * (delta_i * source.out(i) - sum_j)
// every operation its own f64 rounding (-ffp-contract=off), the logistic = rho_fdlibm of rl_device.h.  The float pair weight of the Java
// (1.0f) multiplies exactly and is left out.
//
//   k_rn_epoch       one launch per epoch and ONE workgroup of kRnThreads that walks all lists and, inside a list, the documents in order:
//                    step i + 1 reads the weights step i wrote, and that dependency is the algorithm.  The pairs of a step are a bit mask
//                    over the list's documents (one __ballot per wavefront); the serial sums walk its set bits in ascending order.
//   k_lrk_epoch      k_rn_epoch's sibling for LambdaRank (rl_rn_set_lambdarank, DESIGN.md 17): described where it stands
//   k_rn_score       the forward pass over a whole set at full width, for the per-epoch metric: net_layer over the context's column-major
//                    set, rl_net_predict's bits on the same rows.
//   k_rn_misordered  estimateLoss's count (:230-252) over a set's score cache, a block per list; an integer, so any order is exact.

#include <chrono>

#include "rl_knobs.h"

namespace rl {

constexpr int kRnThreads = 1024;       // the workgroup of k_rn_epoch (DESIGN.md 16)
constexpr int kRnMaxL = 9;             // layers past the input: at most 8 hidden layers and the output neuron
constexpr int kRnMaxW = 2048;          // weights kept in LDS (16 KB); more: k_rn_epoch<false> works on the global copy
constexpr int kRnPool = 9216;          // doubles of LDS (72 KB) for a list's kept values: 3 n H + n + H of them; more: the handle's global pool
constexpr int kRnXCap = 8192;          // floats of LDS (32 KB) for a list's X tile [F][n | 1]; larger: X is read from the set
constexpr int kRnMaskWords = 512;      // 64-bit words of the pair mask (4 KB): lists of up to kRnMaxList documents
constexpr int kRnMaxList = kRnMaskWords * 64;

struct RnNet {
    int32_t F, L, nw, H, maxw;         // inputs, layers past the input, weights, neurons past the input, widest hidden layer
    int32_t dims[kRnMaxL + 1];         // F, the hidden sizes, 1
    int32_t woff[kRnMaxL + 1];         // [l]: where layer l's matrix starts among the weights, l = 1 .. L
    int32_t ooff[kRnMaxL + 1];         // [l]: the neurons of layers 1 .. l - 1
};

struct RnArgs {
    const float *xc; const float *labels; const int32_t *qoff;
    double *w;                 // [nw], read at the start and written at the end of an epoch
    double *pool;              // [3 maxq H + maxq + H]
    int64_t N; int32_t Q;
    double lr;
    RnNet net;
};

__device__ __forceinline__ uint64_t rn_uniform(uint64_t m)
{   // a value every lane holds: into scalar registers
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)m), hi = __builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// SKIP (a measuring aid, rl_rn::skip): 1 leaves out the forward pass, 2 the deltas, 4 the update; the results are then meaningless
template <bool WLDS, int SKIP>
__global__ __launch_bounds__(kRnThreads) void k_rn_epoch(const RnArgs a)
{
    __shared__ double s_w[WLDS ? kRnMaxW : 1];
    __shared__ double s_pool[kRnPool];
    __shared__ float s_x[kRnXCap];
    __shared__ uint64_t s_mask[kRnMaskWords];
    __shared__ int s_P;
    const int tid = threadIdx.x, F = a.net.F, L = a.net.L, H = a.net.H, nw = a.net.nw;
    double *w = WLDS ? s_w : a.w;
    if (WLDS) {
        for (int k = tid; k < nw; k += kRnThreads) s_w[k] = a.w[k];
        __syncthreads();
    }
    for (int q = 0; q < a.Q; q++) {
        const int cur = a.qoff[q], n = a.qoff[q + 1] - cur, np = n | 1, nwords = (n + 63) >> 6;
        const int64_t nH = (int64_t)n * H;
        double *pool = 3 * nH + n + H <= kRnPool ? s_pool : a.pool;
        double *out = pool, *dd = out + nH, *dj = dd + nH, *pp = dj + nH, *di = pp + n;      // [H][n] three times, [n], [H]
        const bool xt = (int64_t)np * F <= kRnXCap;
        const float *xg = a.xc + cur;                                   // document j's input k: xg[k * N + j]
        if (xt) {
            for (int e = tid; e < n * F; e += kRnThreads) {
                const int k = e / n, i = e - k * n;
                s_x[k * np + i] = xg[(int64_t)k * a.N + i];
            }
            __syncthreads();
        }
        // batchFeedForward: a document per lane, every layer in the lane's own columns
        for (int i = tid; i < n; i += kRnThreads) {
            const double *W = w;
            for (int l = 1; l <= L; l++) {
                const int ns = a.net.dims[l - 1], nl = a.net.dims[l];
                double *ol = out + (int64_t)a.net.ooff[l] * n + i, *dl = dd + (int64_t)a.net.ooff[l] * n + i;
                auto put = [&](int j, double v) {
                    ol[(int64_t)j * n] = v;
                    const double s = rho_fdlibm(-v);
                    dl[(int64_t)j * n] = s * (1.0 - s);
                };
                if (SKIP & 1) {
                    for (int j = 0; j < nl; j++) { ol[(int64_t)j * n] = 0.5; dl[(int64_t)j * n] = 0.25; }
                } else if (l == 1) {
                    if (xt) net_layer(W, ns, nl, [&](int k) { return (double)s_x[k * np + i]; }, put);
                    else net_layer(W, ns, nl, [&](int k) { return (double)xg[(int64_t)k * a.N + i]; }, put);
                } else {
                    const double *il = out + (int64_t)a.net.ooff[l - 1] * n + i;
                    net_layer(W, ns, nl, [&](int k) { return il[(int64_t)k * n]; }, put);
                }
                W += (size_t)nl * (ns + 1);
            }
        }
        __syncthreads();
        double *po = out + (int64_t)a.net.ooff[L] * n, *ddo = dd + (int64_t)a.net.ooff[L] * n, *djo = dj + (int64_t)a.net.ooff[L] * n;
        // batchBackPropagate
        for (int i = 0; i < n; i++) {
            const float li = a.labels[cur + i];
            const double oi = po[i];
            // the pairs of i and the output neuron's pij, deltas_j: a document per lane
            for (int j0 = 0; j0 < n; j0 += kRnThreads) {
                const int j = j0 + tid;
                const bool f = j < n && li > a.labels[cur + (j < n ? j : 0)];
                const uint64_t b = __ballot(f);
                if ((tid & (kWave - 1)) == 0 && j < n) s_mask[j >> 6] = b;
                if (f) {
                    const double p = (SKIP & 2) ? 0.5 : rho_fdlibm(oi - po[j]);
                    pp[j] = p;
                    djo[j] = p * ddo[j];
                }
            }
            __syncthreads();
            // the output neuron's delta_i: one serial chain over the pairs in ascending order, every lane of wavefront 0 carries it
            if (tid < kWave) {
                double s = 0.0;
                int P = 0;
                for (int wd = 0; wd < nwords; wd++) {
                    uint64_t m = rn_uniform(s_mask[wd]);
                    P += __popcll(m);
                    if (SKIP & 2) continue;
                    const double val = ((m >> tid) & 1) ? pp[wd * 64 + tid] : 0.0;
                    while (m) {
                        const int bit = __builtin_ctzll(m);
                        m &= m - 1;
                        s += ln_readlane(val, bit);
                    }
                }
                s *= ddo[i];
                if (tid == 0) { di[a.net.ooff[L]] = s; s_P = P; }
            }
            __syncthreads();
            const int P = s_P;
            // updateDelta of the hidden layers, last to first: a (neuron, pair) per lane, then a neuron's delta_i per lane
            for (int l = L - 1; l >= 1 && !(SKIP & 2); l--) {
                const int nl = a.net.dims[l], nt = a.net.dims[l + 1];
                const double *Wt = w + a.net.woff[l + 1];                               // [nt][nl + 1]
                const double *djt = dj + (int64_t)a.net.ooff[l + 1] * n, *dit = di + a.net.ooff[l + 1];
                double *djl = dj + (int64_t)a.net.ooff[l] * n;
                const double *ddl = dd + (int64_t)a.net.ooff[l] * n;
                for (int64_t e = tid; e < (int64_t)nl * n; e += kRnThreads) {
                    const int h = (int)(e / n), j = (int)(e - (int64_t)h * n);
                    if (!((s_mask[j >> 6] >> (j & 63)) & 1)) continue;
                    double es = 0.0;
                    for (int t = 0; t < nt; t++) es += djt[(int64_t)t * n + j] * Wt[(size_t)t * (nl + 1) + h];
                    djl[(int64_t)h * n + j] = es * ddl[(int64_t)h * n + j];
                }
                for (int h = tid; h < nl; h += kRnThreads) {
                    double d = 0.0;
                    if (P > 0) {
                        for (int t = 0; t < nt; t++) d += dit[t] * Wt[(size_t)t * (nl + 1) + h];
                        d *= ddl[(int64_t)h * n + i];
                    }
                    di[a.net.ooff[l] + h] = d;
                }
                __syncthreads();
            }
            // updateWeight: a weight per lane, its sum_j a serial chain over the pairs in ascending order
            for (int e = tid; e < nw && !(SKIP & 4); e += kRnThreads) {
                int l = 1;
                while (l < L && e >= a.net.woff[l + 1]) l++;
                const int ns = a.net.dims[l - 1], r = e - a.net.woff[l], t = r / (ns + 1), s = r - t * (ns + 1);
                const double *djn = dj + (int64_t)(a.net.ooff[l] + t) * n;
                const double delta = di[a.net.ooff[l] + t];
                auto update = [&](auto src) {
                    double sum = 0.0;
                    for (int wd = 0; wd < nwords; wd++) {
                        uint64_t m = rn_uniform(s_mask[wd]);
                        while (m) {
                            const int j = wd * 64 + __builtin_ctzll(m);
                            m &= m - 1;
                            sum += djn[j] * src(j);
                        }
                    }
                    const double dw = a.lr * (delta * src(i) - sum);
                    w[e] += dw;
                };
                if (s == ns) update([&](int) { return 1.0; });
                else if (l > 1) { const double *sl = out + (int64_t)(a.net.ooff[l - 1] + s) * n; update([&](int j) { return sl[j]; }); }
                else if (xt) { const float *xs = s_x + s * np; update([&](int j) { return (double)xs[j]; }); }
                else { const float *xs = xg + (int64_t)s * a.N; update([&](int j) { return (double)xs[j]; }); }
            }
            __syncthreads();                                 // the next step reads these weights and reuses the mask, pp, dj and di
        }
    }
    if (WLDS)
        for (int k = tid; k < nw; k += kRnThreads) a.w[k] = s_w[k];
}

// ---- LambdaRank (-ranker 5, learning/neuralnet/LambdaRank.java, the pairWeight != null arms of Neuron.java :111-120, :136-148) -------------
// k_lrk_epoch is k_rn_epoch's walk with LambdaRank's four overrides (DESIGN.md 17); a sibling, not a third template argument, so that the
// RankNet instances keep their device code.  Per list, after the forward pass: the rank of every document by its output (stable,
// descending) as perm[position] = document; the scorer's tables on the ranked labels; then per step i -- a ranked POSITION -- the pairs
// are the positions j whose label differs, the target bit label_i > label_j, the float pair weight |swapChange[i][j]| * sign.  The kept
// outputs, d() and X stay in the given order and are read through perm; lambda, deltas_j, the weight row and the pair mask are by position.
// The target value is consumed where it is formed (the lane that owns the pair computes lambda at once), so it needs no mask of its own.

constexpr int kLrkList = 1024;                     // documents of a list whose LambdaRank arrays stay in LDS; longer: the handle's global pool
constexpr int kLrkChainList = 4096;                // documents of a list under MAP, or ERR@k with k beyond it: a lane walks a chain of up to n per pair
constexpr int kLrkPool = (7 * kLrkList + 1) / 2;   // doubles (28 KB): two tables [n] of doubles, then perm, the ranked labels, the weight row

struct LrkArgs {
    RnArgs r;
    const double *ideal;       // [Q] the lists' ideal DCG as the context scores with (NDCG)
    const int32_t *rd;         // [Q] external relevant-document counts (MAP under -qrel) or null
    const double *disc;        // [maxq + 2] DCGScorer's discounts
    double *lpool;             // [(7 maxq + 1) / 2]
    int32_t metric, mk;
    double err_max;
};

__device__ __forceinline__ double lrk_gain(int rel) { return (double)(int)(((unsigned)1 << (rel & 31)) - 1u); }     // (1 << rel) - 1, a Java int

struct LrkTab {
    const double *A, *B;       // NDCG / DCG: gain, discount.  ERR: R, np (0 from `size` on).  MAP: A holds relCount as int32
    const float *lab;          // the ranked labels
    int32_t size, metric, rd, cnt;
    double ideal;
};

// |changes[a][b]| of scorer.swapChange for ranked positions a < b: NDCGScorer.java:132-160, DCGScorer.java:74-90, APScorer.java:108-162,
// ERRScorer.java:76-115, every operation in the Java's order
__device__ double lrk_swap_abs(const LrkTab &t, int a, int b)
{
    if (t.metric == RL_METRIC_NDCG) {
        if (a >= t.size || !(t.ideal > 0)) return 0.0;
        return fabs((t.B[a] - t.B[b]) * (t.A[a] - t.A[b]) / t.ideal);
    }
    if (t.metric == RL_METRIC_DCG) {
        if (a >= t.size) return 0.0;
        return fabs((t.B[a] - t.B[b]) * (t.A[a] - t.A[b]));
    }
    if (t.metric == RL_METRIC_MAP) {                       // K ignored; divided by rdCount, the external count under -qrel
        if (t.rd == 0 || t.cnt == 0) return 0.0;
        const int32_t *rc = (const int32_t *)t.A;
        const int la = t.lab[a] > 0.f ? 1 : 0, lb = t.lab[b] > 0.f ? 1 : 0;
        double change = 0;
        if (la != lb) {
            const int diff = lb - la, ra = rc[a], rb = rc[b];
            change += ((double)((ra + diff) * lb - ra * la)) / (a + 1);
            for (int k = a + 1; k <= b - 1; k++)
                if (t.lab[k] > 0.f) change += ((double)diff) / (k + 1);
            change += ((double)(-rb * diff)) / (b + 1);
        }
        return fabs(change / t.rd);
    }
    // ERR: labels / R / np from `size` on are 0 in the Java, so its k-loop past `size` adds p * 0 / (1 + k) and multiplies p by 1
    if (a >= t.size) return 0.0;
    const int la = (int)t.lab[a], lb = (b < t.size) ? (int)t.lab[b] : 0;
    if (la == lb) return 0.0;
    const double Ra = t.A[a], Rb = t.A[b];
    const double base = (a == 0) ? 1.0 : t.B[a - 1];
    const double v1 = 1.0 / (a + 1) * base;
    double change = v1 * (Rb - Ra);
    double p = base * (Ra - Rb);
    const int kend = min(b, t.size);
    for (int k = a + 1; k < kend; k++) { const double Rk = t.A[k]; change += p * Rk / (1 + k); p *= 1.0 - Rk; }
    if (b > kend) change += p * 0.0;                       // +-0, or NaN once p is not finite
    const double npb = t.B[b - 1];
    change += (npb * (1.0 - Rb) * Ra / (1.0 - Ra) - npb * Rb) / (b + 1);
    return fabs(change);
}

// SKIP: 1 leaves out the forward pass, 4 the update, as k_rn_epoch's.  There is no variant without the deltas: the update would read
// hidden deltas_j that nobody wrote, so RLHIP_RN_SKIP=2 runs the whole kernel on a LambdaRank handle
template <bool WLDS, int SKIP>
__global__ __launch_bounds__(kRnThreads) void k_lrk_epoch(const LrkArgs g)
{
    __shared__ double s_w[WLDS ? kRnMaxW : 1];
    __shared__ double s_pool[kRnPool];
    __shared__ double s_lrk[kLrkPool];
    __shared__ float s_x[kRnXCap];
    __shared__ uint64_t s_mask[kRnMaskWords];
    __shared__ double s_w0;
    __shared__ int s_P;
    const RnArgs &a = g.r;
    const int tid = threadIdx.x, F = a.net.F, L = a.net.L, H = a.net.H, nw = a.net.nw;
    double *w = WLDS ? s_w : a.w;
    if (WLDS) {
        for (int k = tid; k < nw; k += kRnThreads) s_w[k] = a.w[k];
        __syncthreads();
    }
    for (int q = 0; q < a.Q; q++) {
        const int cur = a.qoff[q], n = a.qoff[q + 1] - cur, np = n | 1, nwords = (n + 63) >> 6;
        const int64_t nH = (int64_t)n * H;
        double *pool = 3 * nH + n + H <= kRnPool ? s_pool : a.pool;
        double *out = pool, *dd = out + nH, *dj = dd + nH, *pp = dj + nH, *di = pp + n;      // [H][n] three times, [n], [H]
        double *lp = n <= kLrkList ? s_lrk : g.lpool;
        double *tabA = lp, *tabB = lp + n;                                                   // [n] twice, then three [n] of 4 bytes
        int32_t *perm = (int32_t *)(lp + 2 * (int64_t)n);
        float *rlab = (float *)(perm + n), *wrow = rlab + n;
        const bool xt = (int64_t)np * F <= kRnXCap;
        const float *xg = a.xc + cur;                                   // document j's input k: xg[k * N + j]
        if (xt) {
            for (int e = tid; e < n * F; e += kRnThreads) {
                const int k = e / n, i = e - k * n;
                s_x[k * np + i] = xg[(int64_t)k * a.N + i];
            }
            __syncthreads();
        }
        // the forward pass, in the given order: eval(doc) of rank() and batchFeedForward's propagate are the same chain
        for (int i = tid; i < n; i += kRnThreads) {
            const double *W = w;
            for (int l = 1; l <= L; l++) {
                const int ns = a.net.dims[l - 1], nl = a.net.dims[l];
                double *ol = out + (int64_t)a.net.ooff[l] * n + i, *dl = dd + (int64_t)a.net.ooff[l] * n + i;
                auto put = [&](int j, double v) {
                    ol[(int64_t)j * n] = v;
                    const double s = rho_fdlibm(-v);
                    dl[(int64_t)j * n] = s * (1.0 - s);
                };
                if (SKIP & 1) {
                    for (int j = 0; j < nl; j++) { ol[(int64_t)j * n] = 0.5; dl[(int64_t)j * n] = 0.25; }
                } else if (l == 1) {
                    if (xt) net_layer(W, ns, nl, [&](int k) { return (double)s_x[k * np + i]; }, put);
                    else net_layer(W, ns, nl, [&](int k) { return (double)xg[(int64_t)k * a.N + i]; }, put);
                } else {
                    const double *il = out + (int64_t)a.net.ooff[l - 1] * n + i;
                    net_layer(W, ns, nl, [&](int k) { return il[(int64_t)k * n]; }, put);
                }
                W += (size_t)nl * (ns + 1);
            }
        }
        __syncthreads();
        double *po = out + (int64_t)a.net.ooff[L] * n, *ddo = dd + (int64_t)a.net.ooff[L] * n, *djo = dj + (int64_t)a.net.ooff[L] * n;
        // internalReorder = rank(rl): MergeSorter's stable descending order; position = the outputs above, and the equal ones before
        // (a NaN output -- the weights went NaN earlier in this epoch, which the host refuses after it -- ranks below every number and
        // ties with other NaNs, so that perm stays a permutation and every index read through it stays inside the list)
        for (int j = tid; j < n; j += kRnThreads) {
            const double oj = po[j];
            const bool nj = oj != oj;
            int pos = 0;
            for (int m = 0; m < n; m++) {
                const double om = po[m];
                const bool nm = om != om;
                const bool above = om > oj || (nj && !nm), same = om == oj || (nj && nm);
                pos += (above || (same && m < j)) ? 1 : 0;
            }
            perm[pos] = j;
            rlab[pos] = a.labels[cur + j];
        }
        __syncthreads();
        // the scorer's tables on the ranked labels
        const int size = n > g.mk ? g.mk : n;                           // swapChange's cut-off (<= 0 with k <= 0: no position below it)
        if (g.metric == RL_METRIC_NDCG || g.metric == RL_METRIC_DCG) {
            for (int p = tid; p < n; p += kRnThreads) { tabA[p] = lrk_gain((int)rlab[p]); tabB[p] = g.disc[p]; }
        } else if (g.metric == RL_METRIC_MAP) {                         // relCount: integers, any order is exact
            int32_t *rc = (int32_t *)tabA;
            for (int p = tid; p < n; p += kRnThreads) {
                int c = 0;
                for (int m = 0; m <= p; m++) c += rlab[m] > 0.f ? 1 : 0;
                rc[p] = c;
            }
        } else {                                                        // ERR: R and np of the first `size` positions, one serial chain
            if (tid == 0) {
                double p = 1.0;
                for (int i = 0; i < size; i++) {
                    const double R = lrk_gain((int)rlab[i]) / g.err_max, v = p * (1.0 - R);
                    p *= v;
                    tabA[i] = R; tabB[i] = v;
                }
            }
            for (int p = (size > 0 ? size : 0) + tid; p < n; p += kRnThreads) { tabA[p] = 0.0; tabB[p] = 0.0; }
        }
        __syncthreads();
        LrkTab tab;
        tab.A = tabA; tab.B = tabB; tab.lab = rlab; tab.size = size; tab.metric = g.metric; tab.ideal = g.ideal[q];
        tab.cnt = g.metric == RL_METRIC_MAP ? ((const int32_t *)tabA)[n - 1] : 0;          // n >= 1: rl_rn_set_train refuses an empty list (ca_check_set)
        tab.rd = g.rd ? g.rd[q] : tab.cnt;
        // batchBackPropagate over the ranked positions
        for (int i = 0; i < n; i++) {
            const float li = rlab[i];
            const int doci = perm[i];
            const double oi = po[doci];
            // the pairs of i, their targets and weights, the output neuron's lambda and deltas_j: a position per lane
            for (int j0 = 0; j0 < n; j0 += kRnThreads) {
                const int j = j0 + tid;
                const float lj = rlab[j < n ? j : 0];
                const bool tg = j < n && li > lj, f = tg || (j < n && li < lj);
                const uint64_t b = __ballot(f);
                if ((tid & (kWave - 1)) == 0 && j < n) s_mask[j >> 6] = b;
                if (f) {
                    const double ch = lrk_swap_abs(tab, i < j ? i : j, i < j ? j : i);
                    const float wf = (float)ch * (float)(tg ? 1 : -1);
                    wrow[j] = wf;
                    const int docj = perm[j];
                    const double pij = (double)(tg ? 1.0f : 0.0f) - rho_fdlibm(-(oi - po[docj]));
                    const double lambda = (double)wf * pij;
                    pp[j] = lambda;
                    djo[j] = lambda * ddo[docj];
                }
            }
            __syncthreads();
            // the output neuron's delta_i: one serial chain over the pairs in ascending order; weight_0 = the first pair's weight
            if (tid < kWave) {
                double s = 0.0;
                int P = 0, first = -1;
                for (int wd = 0; wd < nwords; wd++) {
                    uint64_t m = rn_uniform(s_mask[wd]);
                    if (first < 0 && m) first = wd * 64 + __builtin_ctzll(m);
                    P += __popcll(m);
                    const double val = ((m >> tid) & 1) ? pp[wd * 64 + tid] : 0.0;
                    while (m) {
                        const int bit = __builtin_ctzll(m);
                        m &= m - 1;
                        s += ln_readlane(val, bit);
                    }
                }
                s *= ddo[doci];
                if (tid == 0) { di[a.net.ooff[L]] = s; s_P = P; s_w0 = first >= 0 ? (double)wrow[first] : 0.0; }
            }
            __syncthreads();
            const int P = s_P;
            const double w0 = s_w0;
            // updateDelta of the hidden layers, last to first: deltas_j take the pair's weight, delta_i takes weight_0
            for (int l = L - 1; l >= 1; l--) {
                const int nl = a.net.dims[l], nt = a.net.dims[l + 1];
                const double *Wt = w + a.net.woff[l + 1];                               // [nt][nl + 1]
                const double *djt = dj + (int64_t)a.net.ooff[l + 1] * n, *dit = di + a.net.ooff[l + 1];
                double *djl = dj + (int64_t)a.net.ooff[l] * n;
                const double *ddl = dd + (int64_t)a.net.ooff[l] * n;
                for (int64_t e = tid; e < (int64_t)nl * n; e += kRnThreads) {
                    const int h = (int)(e / n), j = (int)(e - (int64_t)h * n);
                    if (!((s_mask[j >> 6] >> (j & 63)) & 1)) continue;
                    double es = 0.0;
                    for (int t = 0; t < nt; t++) es += djt[(int64_t)t * n + j] * Wt[(size_t)t * (nl + 1) + h];
                    djl[(int64_t)h * n + j] = (es * (double)wrow[j]) * ddl[(int64_t)h * n + perm[j]];
                }
                for (int h = tid; h < nl; h += kRnThreads) {
                    double d = 0.0;
                    if (P > 0) {
                        for (int t = 0; t < nt; t++) d += dit[t] * Wt[(size_t)t * (nl + 1) + h];
                        d *= (w0 * ddl[(int64_t)h * n + doci]);
                    }
                    di[a.net.ooff[l] + h] = d;
                }
                __syncthreads();
            }
            // updateWeight: a weight per lane, its sum_j a serial chain over the pairs in ascending order
            for (int e = tid; e < nw && !(SKIP & 4); e += kRnThreads) {
                int l = 1;
                while (l < L && e >= a.net.woff[l + 1]) l++;
                const int ns = a.net.dims[l - 1], r = e - a.net.woff[l], t = r / (ns + 1), s = r - t * (ns + 1);
                const double *djn = dj + (int64_t)(a.net.ooff[l] + t) * n;
                const double delta = di[a.net.ooff[l] + t];
                auto update = [&](auto src) {                                           // src(document)
                    double sum = 0.0;
                    for (int wd = 0; wd < nwords; wd++) {
                        uint64_t m = rn_uniform(s_mask[wd]);
                        while (m) {
                            const int j = wd * 64 + __builtin_ctzll(m);
                            m &= m - 1;
                            sum += djn[j] * src(perm[j]);
                        }
                    }
                    const double dw = a.lr * (delta * src(doci) - sum);
                    w[e] += dw;
                };
                if (s == ns) update([&](int) { return 1.0; });
                else if (l > 1) { const double *sl = out + (int64_t)(a.net.ooff[l - 1] + s) * n; update([&](int j) { return sl[j]; }); }
                else if (xt) { const float *xs = s_x + s * np; update([&](int j) { return (double)xs[j]; }); }
                else { const float *xs = xg + (int64_t)s * a.N; update([&](int j) { return (double)xs[j]; }); }
            }
            __syncthreads();                                 // the next step reads these weights and reuses the mask, the weight row, pp, dj and di
        }
    }
    if (WLDS)
        for (int k = tid; k < nw; k += kRnThreads) a.w[k] = s_w[k];
}

// a document per lane over a bounded grid, the hidden outputs in a global scratch [2][maxw][lanes]: k_net_forward_global on the column-major set
__global__ __launch_bounds__(kThreads) void k_rn_score(double *out, const float *xc, int64_t n, const RnNet net, const double *w, double *scratch)
{
    const int64_t lanes = (int64_t)gridDim.x * kThreads, lane = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double *act_a = scratch + lane, *act_b = act_a + (size_t)net.maxw * lanes;
    for (int64_t doc = lane; doc < n; doc += lanes) {
        const double *W = w;
        double *in = act_b, *ob = act_a;
        for (int l = 1; l <= net.L; l++) {
            const int ns = net.dims[l - 1], nl = net.dims[l];
            auto put = [&](int j, double val) {
                if (l < net.L) ob[(size_t)j * lanes] = val;
                else out[doc] = val;
            };
            if (l == 1) net_layer(W, ns, nl, [&](int k) { return (double)xc[(int64_t)k * n + doc]; }, put);
            else net_layer(W, ns, nl, [&](int i) { return in[(size_t)i * lanes]; }, put);
            W += (size_t)nl * (ns + 1);
            double *t = in; in = ob; ob = t;
        }
    }
}

// misorderedPairs of every list: pairs k < l in the given order with label_k > label_l and score_k < score_l
__global__ __launch_bounds__(kThreads) void k_rn_misordered(const float *labels, const double *score, const int32_t *qoff, int32_t Q,
                                                            unsigned long long *cnt)
{
    __shared__ unsigned long long s_c[kThreads];
    const int tid = threadIdx.x;
    for (int q = blockIdx.x; q < Q; q += gridDim.x) {
        const int a = qoff[q], b = qoff[q + 1];
        unsigned long long c = 0;
        for (int k = a + tid; k < b - 1; k += kThreads) {
            const float lk = labels[k];
            const double sk = score[k];
            for (int l = k + 1; l < b; l++) c += (lk > labels[l] && sk < score[l]) ? 1 : 0;
        }
        s_c[tid] = c;
        __syncthreads();
        for (int st = kThreads / 2; st > 0; st >>= 1) {
            if (tid < st) s_c[tid] += s_c[tid + st];
            __syncthreads();
        }
        if (tid == 0) cnt[q] = s_c[0];
        __syncthreads();
    }
}

}  // namespace rl

struct rl_rn {
    rl_rn_params p;
    std::vector<int32_t> hidden;
    rl::RnNet net;                         // filled by rl_rn_set_train (it needs the feature count)
    LinCtx ctx;
    std::vector<double> start, weight;     // the weights rl_rn_set_weights gave; after learn: the restored best or the last epoch's
    std::vector<rl_rn_trace_rec> trace;
    int64_t total_pairs = 0;               // RankNet.init()'s totalPairs, counted by rl_rn_set_train
    double epoch_ms = 0, score_ms = 0;
    int32_t skip = 0;                      // RLHIP_RN_SKIP (rl_knobs.h): the phase k_rn_epoch leaves out, for tools/rn_bench.py
    bool lambdarank = false;               // rl_rn_set_lambdarank: k_lrk_epoch in place of k_rn_epoch
    const char *name() const { return lambdarank ? "LambdaRank" : "RankNet"; }
};

namespace rl {

static void rn_plan(rl_rn *h, int32_t F)
{
    RnNet &n = h->net;
    n = RnNet();
    n.F = F; n.L = (int32_t)h->hidden.size() + 1;
    n.dims[0] = F;
    for (int l = 1; l < n.L; l++) { n.dims[l] = h->hidden[l - 1]; n.maxw = std::max(n.maxw, n.dims[l]); }
    n.dims[n.L] = 1;
    int64_t nw = 0, H = 0;
    for (int l = 1; l <= n.L; l++) {
        n.woff[l] = (int32_t)nw; n.ooff[l] = (int32_t)H;
        nw += (int64_t)n.dims[l] * (n.dims[l - 1] + 1);
        H += n.dims[l];
    }
    n.nw = (int32_t)nw; n.H = (int32_t)H;
}

// RankNet.init() :268-278 over getCorrectRanking(): the pairs of a list whose labels differ
static int64_t rn_total_pairs(const CaSet &d)
{
    int64_t total = 0;
    std::vector<float> lab;
    for (int32_t q = 0; q < d.Q; q++) {
        lab.assign(d.labels.begin() + d.qoff[q], d.labels.begin() + d.qoff[q + 1]);
        std::sort(lab.begin(), lab.end());
        const int64_t n = (int64_t)lab.size();
        int64_t same = 0;
        for (int64_t i = 0; i < n;) {
            int64_t j = i;
            while (j < n && lab[j] == lab[i]) j++;
            same += (j - i) * (j - i - 1) / 2;
            i = j;
        }
        total += n * (n - 1) / 2 - same;
    }
    return total;
}

struct RnDev { double *w, *scratch; unsigned long long *cnt; std::vector<unsigned long long> h_cnt; };

static int rn_score_set(rl_rn *h, CaSet &d, RnDev &v, double *score, int64_t *misordered)
{
    LinCtx *c = &h->ctx;
    const int64_t blocks = (d.N + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_rn_score, dim3((unsigned)std::min<int64_t>(blocks, kNetGlobalBlocks)), dim3(kThreads), 0, c->stream, d.d_cache,
                       (const float *)d.d_xc, d.N, h->net, (const double *)v.w, v.scratch);
    RL_HIP(hipGetLastError());
    if (misordered) {
        hipLaunchKernelGGL(k_rn_misordered, dim3((unsigned)std::min<int32_t>(d.Q, 4096)), dim3(kThreads), 0, c->stream,
                           (const float *)d.d_labels, (const double *)d.d_cache, (const int32_t *)d.d_qoff, d.Q, v.cnt);
        RL_HIP(hipGetLastError());
        RL_HIP(hipMemcpyAsync(v.h_cnt.data(), v.cnt, (size_t)d.Q * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    int rc = ca_trials(c, d, nullptr, nullptr, 1, 0, score);       // synchronises the stream
    if (rc) return rc;
    if (misordered) {
        *misordered = 0;
        for (int32_t q = 0; q < d.Q; q++) *misordered += (int64_t)v.h_cnt[q];
    }
    return RL_OK;
}

template <bool WLDS, int SKIP> static void rn_launch(hipStream_t s, const RnArgs &a)
{
    hipLaunchKernelGGL((k_rn_epoch<WLDS, SKIP>), dim3(1), dim3(kRnThreads), 0, s, a);
}

template <bool WLDS, int SKIP> static void lrk_launch(hipStream_t s, const LrkArgs &g)
{
    hipLaunchKernelGGL((k_lrk_epoch<WLDS, SKIP>), dim3(1), dim3(kRnThreads), 0, s, g);
}

static bool lrk_metric(int32_t metric)
{   // the scorers whose swapChange is built: the tree trainer's four
    return metric == RL_METRIC_NDCG || metric == RL_METRIC_DCG || metric == RL_METRIC_MAP || metric == RL_METRIC_ERR;
}

// RankNet.learn() :290-334, which LambdaRank inherits unchanged
static int rn_learn(rl_rn *h)
{
    LinCtx *c = &h->ctx;
    CaSet &d = c->tr;
    const RnNet &net = h->net;
    const int nw = net.nw;
    int rc = ca_prepare(c);                                   // uploads the sets (and drops the host rows)
    if (rc) return rc;
    RnArgs a;
    RnDev v;
    double *dpool = nullptr;
    RL_HIP(c->buf.alloc(&v.w, (size_t)nw));
    RL_HIP(c->buf.alloc(&dpool, (size_t)3 * d.maxq * net.H + d.maxq + net.H));
    RL_HIP(c->buf.alloc(&v.scratch, (size_t)2 * net.maxw * kNetGlobalBlocks * kThreads));
    RL_HIP(c->buf.alloc(&v.cnt, (size_t)d.Q));
    v.h_cnt.resize((size_t)d.Q);
    a.xc = d.d_xc; a.labels = d.d_labels; a.qoff = d.d_qoff; a.w = v.w; a.pool = dpool; a.N = d.N; a.Q = d.Q; a.lr = h->p.learning_rate;
    a.net = net;
    LrkArgs g;
    g.r = a; g.ideal = d.d_ideal; g.rd = d.d_rd; g.disc = c->d_disc; g.lpool = nullptr; g.metric = c->metric; g.mk = c->metric_k;
    g.err_max = c->err_max;
    if (h->lambdarank) RL_HIP(c->buf.alloc(&g.lpool, ((size_t)7 * d.maxq + 1) / 2));
    h->weight = h->start;
    RL_HIP(hipMemcpyAsync(v.w, h->weight.data(), nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipEvent_t e0, e1;
    RL_HIP(hipEventCreate(&e0)); RL_HIP(hipEventCreate(&e1));
    struct Events { hipEvent_t a, b; ~Events() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    h->trace.clear(); h->epoch_ms = h->score_ms = 0;
    std::vector<double> best;
    double bestScore = 0.0;                                   // Ranker.bestScoreOnValidationData
    for (int epoch = 1; epoch <= h->p.n_epochs; epoch++) {
        RL_HIP(hipEventRecord(e0, c->stream));
        if (h->lambdarank) {
            if (nw > kRnMaxW) lrk_launch<false, 0>(c->stream, g);
            else if (h->skip == 1) lrk_launch<true, 1>(c->stream, g);
            else if (h->skip == 4) lrk_launch<true, 4>(c->stream, g);
            else lrk_launch<true, 0>(c->stream, g);
        }
        else if (nw > kRnMaxW) rn_launch<false, 0>(c->stream, a);
        else if (h->skip == 1) rn_launch<true, 1>(c->stream, a);
        else if (h->skip == 2) rn_launch<true, 2>(c->stream, a);
        else if (h->skip == 4) rn_launch<true, 4>(c->stream, a);
        else rn_launch<true, 0>(c->stream, a);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(e1, c->stream));
        RL_HIP(hipMemcpyAsync(h->weight.data(), v.w, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        RL_HIP(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, e0, e1));
        h->epoch_ms += ms;
        for (int k = 0; k < nw; k++)
            if (!std::isfinite(h->weight[k])) {
                char msg[300];
                snprintf(msg, sizeof(msg), "%s: weight %d is %.17g after epoch %d (a learning rate too large for the data%s); the Java goes "
                         "on with it, not reproduced (DESIGN.md %s)", h->name(), k, h->weight[k], epoch,
                         h->lambdarank ? ", or a swap change that is not finite" : "", h->lambdarank ? "17" : "16");
                return fail(RL_ERR_UNSUPPORTED, msg);
            }
        const auto t0 = std::chrono::steady_clock::now();
        rl_rn_trace_rec r; r.epoch = epoch; r.saved = 0; r.misordered = 0; r.total_pairs = h->total_pairs; r.train = 0; r.valid = 0;
        if ((rc = rn_score_set(h, d, v, &r.train, &r.misordered))) return rc;          // :304-305
        if (c->has_valid) {
            if ((rc = rn_score_set(h, c->va, v, &r.valid, nullptr))) return rc;
            if (r.valid > bestScore) { bestScore = r.valid; best = h->weight; r.saved = 1; }      // :311-314, strict
        }
        h->score_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        h->trace.push_back(r);
    }
    if (c->has_valid) {                                       // restoreBestModelOnValidation :206-223
        if (best.empty())
            return fail(RL_ERR_NO_BEST, std::string(h->name()) + ": no epoch scored above 0.0 on the validation set, so no model was saved; "
                                        "the Java's restoreBestModelOnValidation throws here");
        h->weight = best;
        RL_HIP(hipMemcpyAsync(v.w, h->weight.data(), nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = rn_score_set(h, d, v, &c->train_score, nullptr))) return rc;
    c->valid_score = 0;
    if (c->has_valid && (rc = rn_score_set(h, c->va, v, &c->valid_score, nullptr))) return rc;
    c->learned = true;
    return RL_OK;
}

}  // namespace rl

extern "C" {

void rl_rn_params_default(rl_rn_params *p)
{   // learning/neuralnet/RankNet.java:37-40
    if (!p) return;
    p->n_epochs = 100; p->learning_rate = 0.00005; p->n_hidden = 1; p->hidden_sizes = nullptr;
    p->metric = RL_METRIC_NDCG; p->metric_k = 10; p->device = 0; p->err_max = 16.0;
}

int rl_rn_create(const rl_rn_params *p, rl_rn **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    if (p->n_epochs < 0) return fail(RL_ERR_INVALID, "n_epochs (-epoch) must not be negative");
    if (!std::isfinite(p->learning_rate)) return fail(RL_ERR_INVALID, "learning_rate must be finite");
    if (p->n_hidden < 0) return fail(RL_ERR_INVALID, "n_hidden (-layer) must not be negative");
    for (int32_t l = 0; l < p->n_hidden && p->hidden_sizes; l++)
        if (p->hidden_sizes[l] < 1) return fail(RL_ERR_INVALID, "hidden layer " + std::to_string(l + 1) + " has no neuron (-node)");
    if (p->n_hidden > kRnMaxL - 1)
        return fail(RL_ERR_UNSUPPORTED, "RankNet training is built for at most " + std::to_string(kRnMaxL - 1) + " hidden layers (DESIGN.md 16)");
    std::unique_ptr<rl_rn> h(new rl_rn());
    h->p = *p;
    for (int32_t l = 0; l < p->n_hidden; l++) h->hidden.push_back(p->hidden_sizes ? p->hidden_sizes[l] : 10);
    h->p.hidden_sizes = nullptr;                             // the caller's array is not kept
    h->skip = read_rn_skip_knob();
    int rc = lin_create(&h->ctx, "RankNet", p->metric, p->metric_k, p->device, p->err_max);
    if (rc) return rc;
    *out = h.release();
    return RL_OK;
}

void rl_rn_destroy(rl_rn *h) { lin_destroy(h); }

int rl_rn_set_train(rl_rn *h, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                    int32_t n_queries, const int32_t *qkey)
{
    if (h && n_features > 0) {
        int64_t nw = 0, prev = n_features;
        for (int32_t sz : h->hidden) { nw += (int64_t)sz * (prev + 1); prev = sz; }
        nw += prev + 1;
        if (nw > (int64_t)1 << 28) return fail(RL_ERR_UNSUPPORTED, "RankNet: a network of more than 2^28 weights");
    }
    int rc = lin_set_train(lin_ctx(h), "rl_rn_", X, n_docs, n_features, labels, qoff, n_queries, qkey);
    if (rc) return rc;
    h->start.clear();                                        // the weights belong to a feature count
    rn_plan(h, n_features);
    h->total_pairs = rn_total_pairs(h->ctx.tr);
    return RL_OK;
}

int rl_rn_set_validation(rl_rn *h, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                         const int32_t *qkey)
{
    return lin_set_validation(lin_ctx(h), "rl_rn_", X, n_docs, labels, qoff, n_queries, qkey);
}

int rl_rn_set_external_judgments(rl_rn *h, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    return lin_set_external_judgments(lin_ctx(h), "rl_rn_", validation, ideal_dcg, rel_doc_count);
}

int rl_rn_set_weights(rl_rn *h, const double *w, int32_t n)
{
    if (!h || !w) return fail(RL_ERR_INVALID, "null argument");
    if (!h->ctx.has_train) return fail(RL_ERR_INVALID, "rl_rn_set_weights: set the training data first (the weight count depends on n_features)");
    if (h->ctx.uploaded) return fail(RL_ERR_STATE, "rl_rn_set_weights after rl_rn_learn");
    if (n != h->net.nw)
        return fail(RL_ERR_INVALID, "rl_rn_set_weights: n is " + std::to_string(n) + ", the network has " + std::to_string(h->net.nw) +
                                    " weights (for every layer n_l * (n_{l-1} + 1))");
    h->start.assign(w, w + n);
    return RL_OK;
}

int rl_rn_set_lambdarank(rl_rn *h, int32_t on)
{
    if (!h) return fail(RL_ERR_INVALID, "null handle");
    if (h->ctx.uploaded) return fail(RL_ERR_STATE, "rl_rn_set_lambdarank after rl_rn_learn");
    if (on && !lrk_metric(h->ctx.metric))
        return fail(RL_ERR_UNSUPPORTED, "LambdaRank: the train metric must be one of NDCG, DCG, MAP, ERR: the swap changes of P@k, RR@k and "
                                        "BEST are not built (DESIGN.md 17)");
    h->lambdarank = on != 0;
    return RL_OK;
}

int rl_rn_learn(rl_rn *h)
{
    if (!h) return fail(RL_ERR_INVALID, "null handle");
    if (!h->ctx.has_train) return fail(RL_ERR_INVALID, "rl_rn_learn: set the training data first");
    if (h->start.empty()) return fail(RL_ERR_INVALID, "rl_rn_learn: set the start weights first (rl_rn_set_weights)");
    if (h->ctx.tr.maxq > kRnMaxList)
        return fail(RL_ERR_UNSUPPORTED, std::string(h->name()) + ": a ranked list of more than " + std::to_string(kRnMaxList) +
                                        " documents (DESIGN.md 16)");
    if (h->lambdarank && h->ctx.tr.maxq > kLrkChainList &&
        (h->ctx.metric == RL_METRIC_MAP || (h->ctx.metric == RL_METRIC_ERR && h->ctx.metric_k > kLrkChainList)))
        return fail(RL_ERR_UNSUPPORTED, "LambdaRank: a ranked list of more than " + std::to_string(kLrkChainList) + " documents under MAP (or ERR@k "
                                        "with a larger k): every pair's swap change walks a serial chain over the list, n^3 / 1024 steps a list "
                                        "(DESIGN.md 17)");
    int rc = lin_begin_learn(lin_ctx(h), "rl_rn_");
    if (rc) return rc;
    return rn_learn(h);
}

int rl_rn_get_weights(const rl_rn *h, double *w, int32_t cap, int32_t *n)
{
    if (!h || !n) return fail(RL_ERR_INVALID, "null argument");
    if (!h->ctx.learned) return fail(RL_ERR_STATE, "rl_rn_learn has not run");
    *n = (int32_t)h->weight.size();
    if (w) std::copy(h->weight.begin(), h->weight.begin() + std::min<size_t>(h->weight.size(), (size_t)std::max(0, cap)), w);
    return RL_OK;
}

int rl_rn_scores(const rl_rn *h, double *train, double *valid) { return lin_scores(lin_ctx(h), "rl_rn_", train, valid); }

int rl_rn_trace(const rl_rn *h, rl_rn_trace_rec *out, int64_t cap, int64_t *n) { return lin_trace(h ? &h->trace : nullptr, out, cap, n); }

int rl_rn_debug_doc_scores(const rl_rn *h, int32_t validation, double *out, int64_t cap)
{
    if (!h || !out) return fail(RL_ERR_INVALID, "null argument");
    if (!h->ctx.learned) return fail(RL_ERR_STATE, "rl_rn_learn has not run");
    if (validation && !h->ctx.has_valid) return fail(RL_ERR_STATE, "no validation set");
    const CaSet &d = validation ? h->ctx.va : h->ctx.tr;
    if (cap < d.N) return fail(RL_ERR_INVALID, "score buffer too small");
    RL_HIP(hipSetDevice(h->ctx.device));
    RL_HIP(hipMemcpy(out, d.d_cache, (size_t)d.N * sizeof(double), hipMemcpyDeviceToHost));
    return RL_OK;
}

int rl_rn_debug_times(const rl_rn *h, double *epoch_ms, double *score_ms)
{
    if (!h) return fail(RL_ERR_INVALID, "null handle");
    if (!h->ctx.uploaded) return fail(RL_ERR_STATE, "rl_rn_learn has not run");
    if (epoch_ms) *epoch_ms = h->epoch_ms;
    if (score_ms) *score_ms = h->score_ms;
    return RL_OK;
}

}  // extern "C"
