// rl_rb.inc -- RankBoost (-ranker 2, learning/boosting/RankBoost.java) on gfx950; included at the end of rl_ca.hip.  The handle holds a
// ranking context (LinCtx, rl_linear.inc: the device sets, the stream, the common entry-point bodies) and ranks with rl_ca.hip's scorer
// (ca_metric) and ranking kernel (k_ca_trials with T = 1 on the cache as it is).
//
// The Java keeps sweight[list][j][k] for every pair of a list.  Only crucial pairs (label_j > label_k) ever hold anything but +0.0, and
// adding or subtracting +0.0 changes neither a potential nor Z_t, so the device stores the crucial pairs alone, in (list, j, k) order:
// the order of the Java's Z_t chain.  The training lists are in getCorrectRanking()'s order (labels descending), so the crucial k of a
// document j are the tail of its list that starts where the next lower label starts: row j is w[rowoff[j] .. rowoff[j + 1]),
// k = kfirst[j] + t.  Offsets into w are 64-bit.
//
//   k_rb_potential   thread j: p = 0.0, += row j (k ascending), -= column j (the rows of the documents with a higher label, ascending)
//   k_rb_cand        block f: the serial chain r += potential[order[f][i]] of feature f (learnWeakRanker :96-141).  The documents a
//                    feature's chain visits and the positions where a threshold is compared are fixed per learn() (rb_build_feature):
//                    order[f] holds the documents, bit 31 set where a comparison follows.  All threads gather tiles of potentials into
//                    LDS (two buffers, the next tile's loads in flight) ahead of thread 0, which adds them and writes every partial sum
//                    back; the comparisons (`r > maxR`, strict: the greatest r at the lowest position) are then the whole block's.
//   k_rb_weak        h_t(x) = [x[f] > threshold] per document and cache += alpha_t * h_t (RankBoost.eval's next term)
//   k_rb_update      16 lanes per row: w = w * exp(alpha_t * (h(k) - h(j))), the factor one of exp(alpha_t), exp(-alpha_t), 1.0 (the host's)
//   k_rb_zsum        ONE block: Z_t, the serial f64 sum over all pairs; tiles staged in LDS as in k_rb_cand
//   k_rb_normalize   w = w / Z_t, an IEEE division
//
// A model's scores from scratch, 0.0 + w[0] h_0(x) + w[1] h_1(x) + ... (RankBoost.eval :348-355), are k_lin_score's with thresholds.
// log / exp are the host C library's, as in rl_ada.inc.

#include <thread>

namespace rl {

constexpr int kRbTile = 2048;          // elements of a staged tile (8 per thread); two tiles of doubles = 32 KB of LDS
constexpr uint32_t kRbCmp = 0x80000000u;

__global__ void k_rb_potential(const double *w, const int64_t *rowoff, const int32_t *kfirst, const int32_t *cbeg, const int32_t *cend,
                               double *pot, int64_t N)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    double p = 0.0;
    const int64_t r1 = rowoff[j + 1];
    for (int64_t a = rowoff[j]; a < r1; a++) p += w[a];                          // updatePotential :80-82
    const int32_t c1 = cend[j];
    for (int32_t k = cbeg[j]; k < c1; k++) p -= w[rowoff[k] + (j - kfirst[k])];  // :83-85
    pot[j] = p;
}

__global__ __launch_bounds__(kThreads) void k_rb_cand(const double *pot, const uint32_t *order, const int64_t *ooff, const uint8_t *cmp0,
                                                      double *best, int32_t *bpos)
{
    __shared__ double s_v[2][kRbTile];
    __shared__ uint32_t s_o[2][kRbTile];
    constexpr int PER = kRbTile / kThreads;
    const int f = blockIdx.x, tid = threadIdx.x;
    const uint32_t *o = order + ooff[f];
    const int64_t n = ooff[f + 1] - ooff[f];
    double v[PER]; uint32_t e[PER];
    auto load = [&](int64_t base) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int64_t i = base + u * kThreads + tid;
            e[u] = i < n ? o[i] : 0u;
            v[u] = i < n ? pot[e[u] & ~kRbCmp] : 0.0;
        }
    };
    double r = 0.0, bst = -10.0;                            // learnWeakRanker: maxR = -10 (carried across features by the host)
    int32_t bp = -1;
    if (tid == 0 && cmp0[f]) { bst = r; bp = 0; }          // thresholds no document exceeds: r = 0.0 is compared first
    load(0);
    int buf = 0;
    for (int64_t base = 0; base < n; base += kRbTile, buf ^= 1) {
#pragma unroll
        for (int u = 0; u < PER; u++) { s_v[buf][u * kThreads + tid] = v[u]; s_o[buf][u * kThreads + tid] = e[u]; }
        __syncthreads();
        if (base + kRbTile < n) load(base + kRbTile);
        if (tid == 0) {
            // the chain: 16 adds a step, the next 16 values already on their way from LDS, every partial sum written back in place.  The
            // tile's tail beyond n holds +0.0: r is never -0.0 (it starts at +0.0), so adding +0.0 leaves it as it is
            const int m = (int)min((int64_t)kRbTile, n - base);
            double vv[16], vn[16];
#pragma unroll
            for (int u = 0; u < 16; u++) vv[u] = s_v[buf][u];
            for (int i0 = 0; i0 < m; i0 += 16) {
                const int nx = min(i0 + 16, kRbTile - 16);
#pragma unroll
                for (int u = 0; u < 16; u++) vn[u] = s_v[buf][nx + u];
#pragma unroll
                for (int u = 0; u < 16; u++) { r += vv[u]; vv[u] = r; }
#pragma unroll
                for (int u = 0; u < 16; u++) s_v[buf][i0 + u] = vv[u];
#pragma unroll
                for (int u = 0; u < 16; u++) vv[u] = vn[u];
            }
        }
        __syncthreads();
        // the comparisons, off the chain: `if (r > maxR)` keeps the first strict maximum, which is the greatest r at the lowest position --
        // every thread scans its share of the tile in position order, the block combines at the end
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int i = u * kThreads + tid;
            const double c = s_v[buf][i];
            if ((s_o[buf][i] & kRbCmp) && c > bst) { bst = c; bp = (int32_t)(base + i + 1); }
        }
    }
    __syncthreads();
    double *s_b = &s_v[0][0];
    int32_t *s_p = (int32_t *)&s_o[0][0];
    s_b[tid] = bst; s_p[tid] = bp;
    __syncthreads();
    if (tid == 0) {
        for (int t = 1; t < kThreads; t++) {
            const double c = s_b[t]; const int32_t q = s_p[t];
            if (q >= 0 && (bp < 0 || c > bst || (c == bst && q < bp))) { bst = c; bp = q; }
        }
        best[f] = bst; bpos[f] = bp;
    }
}

__global__ void k_rb_weak(const float *x, int64_t n, double thr, double alpha, double *cache, uint8_t *h)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = ((double)x[i] > thr) ? 1 : 0;             // RBWeakRanker.score
    if (h) h[i] = (uint8_t)s;
    cache[i] = cache[i] + alpha * (double)s;
}

__global__ void k_rb_update(double *w, const int64_t *rowoff, const int32_t *kfirst, const uint8_t *h, double e_pos, double e_neg, int64_t N)
{
    const int lane = threadIdx.x & 15;
    const int64_t groups = (int64_t)gridDim.x * (blockDim.x >> 4);
    for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4); j < N; j += groups) {
        const int64_t r0 = rowoff[j], r1 = rowoff[j + 1];
        if (r0 == r1) continue;
        const int hj = h[j];
        const uint8_t *hk = h + kfirst[j];
        for (int64_t a = r0 + lane; a < r1; a += 16) {
            const int d = (int)hk[a - r0] - hj;              // alpha_t * d is alpha_t, -alpha_t or +-0.0, and exp(+-0.0) = 1.0
            w[a] = w[a] * (d > 0 ? e_pos : d < 0 ? e_neg : 1.0);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_rb_zsum(const double *w, int64_t P, double *out)
{
    __shared__ double s_v[2][kRbTile];
    constexpr int PER = kRbTile / kThreads;
    const int tid = threadIdx.x;
    double v[PER];
    auto load = [&](int64_t base) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int64_t i = base + u * kThreads + tid;
            v[u] = i < P ? w[i] : 0.0;
        }
    };
    double z = 0.0;
    load(0);
    int buf = 0;
    for (int64_t base = 0; base < P; base += kRbTile, buf ^= 1) {
#pragma unroll
        for (int u = 0; u < PER; u++) s_v[buf][u * kThreads + tid] = v[u];
        __syncthreads();
        if (base + kRbTile < P) load(base + kRbTile);
        if (tid == 0) {
            // as in k_rb_cand: 16 adds a step, the next 16 values already on their way from LDS; the tail beyond P holds +0.0
            const int m = (int)min((int64_t)kRbTile, P - base);
            double vv[16], vn[16];
#pragma unroll
            for (int u = 0; u < 16; u++) vv[u] = s_v[buf][u];
            for (int i0 = 0; i0 < m; i0 += 16) {
                const int nx = min(i0 + 16, kRbTile - 16);
#pragma unroll
                for (int u = 0; u < 16; u++) vn[u] = s_v[buf][nx + u];
#pragma unroll
                for (int u = 0; u < 16; u++) z += vv[u];
#pragma unroll
                for (int u = 0; u < 16; u++) vv[u] = vn[u];
            }
        }
    }
    if (tid == 0) out[0] = z;
}

__global__ void k_rb_normalize(double *w, int64_t P, double z)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += stride) w[i] = w[i] / z;
}

}  // namespace rl

struct rl_rb {
    rl_rb_params p;
    LinCtx ctx;
    std::vector<int32_t> fid; std::vector<double> thr, weight;
    std::vector<rl_rb_trace_rec> trace;
    std::vector<std::vector<double>> pots;       // keep_potentials
};

namespace rl {

// utilities/Sorter.sort(double[], false): the unstable selection sort (the FIRST position >= i holding the maximum is swapped into slot i)
static void rb_sorter(const float *lab, int n, std::vector<int32_t> &idx)
{
    idx.resize(n);
    for (int i = 0; i < n; i++) idx[i] = i;
    for (int i = 0; i < n - 1; i++) {
        int mx = i;
        for (int j = i + 1; j < n; j++)
            if ((double)lab[idx[mx]] < (double)lab[idx[j]]) mx = j;
        std::swap(idx[i], idx[mx]);
    }
}

struct RbFeature {                     // what learnWeakRanker needs of one feature, fixed for the whole of learn()
    std::vector<uint32_t> order;       // the documents in the order the r chain takes them; kRbCmp: a threshold is compared after this one
    std::vector<int64_t> end; std::vector<double> tval;     // the comparisons: documents taken so far (strictly increasing), threshold
    uint8_t cmp0 = 0;                  // a comparison before the first document (end[0] == 0)
};

// init() :188-263 for feature f, restructured: a document is taken at the first threshold (in tSortedIdx order) below its value, the
// documents of one threshold in (list, position in the list's MergeSorter order) order
static void rb_build_feature(const CaSet &d, int F, int f, int nThreshold, RbFeature &out)
{
    const int64_t N = d.N;
    const float *X = d.X.data();
    std::vector<double> th;
    if (nThreshold <= 0) {
        th.resize((size_t)N);
        for (int64_t i = 0; i < N; i++) th[(size_t)i] = (double)X[i * F + f];
    } else {
        double fmax = -1E6, fmin = 1E6;
        for (int64_t i = 0; i < N; i++) {
            const double v = (double)X[i * F + f];
            if (v > fmax) fmax = v;
            if (v < fmin) fmin = v;
        }
        const double step = std::fabs(fmax - fmin) / nThreshold;
        th.resize((size_t)nThreshold + 1);
        th[0] = fmax;
        for (int j = 1; j < nThreshold; j++) th[j] = th[j - 1] - step;
        th[nThreshold] = fmin - 1.0E8;
    }
    const size_t T = th.size();
    std::vector<int32_t> tidx(T);
    for (size_t e = 0; e < T; e++) tidx[e] = (int32_t)e;
    std::stable_sort(tidx.begin(), tidx.end(), [&](int32_t a, int32_t b) { return th[a] > th[b]; });     // MergeSorter.sort(, false)
    std::vector<double> ts(T);
    for (size_t e = 0; e < T; e++) ts[e] = th[tidx[e]];
    std::vector<int32_t> seq((size_t)N), te((size_t)N);
    std::vector<int64_t> cnt(T + 1, 0);
    for (int q = 0; q < d.Q; q++) {
        const int a = d.qoff[q], b = d.qoff[q + 1];
        for (int i = a; i < b; i++) seq[i] = i;
        std::stable_sort(seq.begin() + a, seq.begin() + b, [&](int32_t u, int32_t v) { return X[(int64_t)u * F + f] > X[(int64_t)v * F + f]; });
    }
    for (int64_t s = 0; s < N; s++) {
        const double x = (double)X[(int64_t)seq[s] * F + f];
        const size_t e = std::partition_point(ts.begin(), ts.end(), [&](double t) { return !(x > t); }) - ts.begin();
        te[s] = (int32_t)e;
        cnt[e]++;
    }
    std::vector<int64_t> start(T + 1);
    int64_t acc = 0;
    for (size_t e = 0; e <= T; e++) { start[e] = acc; acc += cnt[e]; }
    const int64_t taken = start[T];
    out.order.assign((size_t)taken, 0u);
    {
        std::vector<int64_t> pos(start.begin(), start.end());
        for (int64_t s = 0; s < N; s++)
            if ((size_t)te[s] < T) out.order[(size_t)pos[te[s]]++] = (uint32_t)seq[s];
    }
    out.end.clear(); out.tval.clear(); out.cmp0 = 0;
    for (size_t e = 0; e < T; e++) {
        const int64_t end = start[e + 1];
        if (!out.end.empty() && out.end.back() == end) continue;      // r unchanged since the last comparison: a strict > cannot hold
        out.end.push_back(end); out.tval.push_back(ts[e]);
        if (end == 0) out.cmp0 = 1; else out.order[(size_t)end - 1] |= kRbCmp;
    }
}

struct RbDev {
    double *w = nullptr, *pot = nullptr, *best = nullptr, *z = nullptr;
    int64_t *rowoff = nullptr, *ooff = nullptr;
    int32_t *kfirst = nullptr, *cbeg = nullptr, *cend = nullptr, *bpos = nullptr;
    uint32_t *order = nullptr; uint8_t *cmp0 = nullptr, *h = nullptr;
    int64_t P = 0;
};

static std::string rb_gb(double bytes)
{
    char b[64];
    snprintf(b, sizeof(b), "%.1f", bytes / 1e9);
    return b;
}

// the crucial-pair layout of the training set (labels descending within a list) and RankBoost.init()'s tables, then the upload
static int rb_init(rl_rb *R, RbDev &D, std::vector<RbFeature> &feat)
{
    LinCtx *c = &R->ctx;
    CaSet &d = c->tr;
    const int64_t N = d.N; const int F = c->F;
    std::vector<int64_t> rowoff((size_t)N + 1);
    std::vector<int32_t> kfirst((size_t)N), cbeg((size_t)N), cend((size_t)N);
    int64_t P = 0;
    for (int q = 0; q < d.Q; q++) {
        const int a = d.qoff[q], b = d.qoff[q + 1];
        for (int g0 = a; g0 < b;) {                          // a group of equal labels [g0, g1): its crucial k start at g1
            int g1 = g0 + 1;
            while (g1 < b && d.labels[g1] == d.labels[g0]) g1++;
            for (int j = g0; j < g1; j++) { rowoff[j] = P; P += b - g1; kfirst[j] = g1; cbeg[j] = a; cend[j] = g0; }
            g0 = g1;
        }
    }
    rowoff[(size_t)N] = P;
    if (P == 0)
        return fail(RL_ERR_UNSUPPORTED, "RankBoost: the training data has no crucial pair (no list holds two different labels); the Java divides by "
                                        "totalCorrectPairs = 0 and stops on round 2 with NaN weights, not reproduced (DESIGN.md 10)");
    if (P > (int64_t)2147483647)
        return fail(RL_ERR_UNSUPPORTED, "RankBoost: " + std::to_string((long long)P) + " crucial pairs; the Java counts them in an int (totalCorrectPairs), "
                                        "which wraps beyond 2^31 - 1, not reproduced (DESIGN.md 10)");
    {
        const double need = 8.0 * (double)P + 4.0 * (double)N * F + 4.0 * (double)N * F * (c->has_valid ? 2 : 1) + 64.0 * (double)N;
        size_t mem_free = 0, mem_total = 0;
        RL_HIP(hipMemGetInfo(&mem_free, &mem_total));
        if (need > 0.8 * (double)mem_free)
            return fail(RL_ERR_UNSUPPORTED, "RankBoost: " + std::to_string((long long)P) + " crucial pairs would need " + rb_gb(need) +
                                            " GB for the pair weights, the take orders and the data; " + rb_gb((double)mem_free) + " GB are free");
    }
    feat.resize((size_t)F);
    {
        const int nt = (int)std::max(1u, std::min(std::min(16u, std::thread::hardware_concurrency()), (unsigned)F));
        std::vector<std::thread> pool;
        for (int w = 0; w < nt; w++)
            pool.emplace_back([&, w]() { for (int f = w; f < F; f += nt) rb_build_feature(d, F, f, R->p.n_threshold, feat[(size_t)f]); });
        for (auto &t : pool) t.join();
    }
    int rc = ca_prepare(c);                                   // uploads the sets (and drops the host rows)
    if (rc) return rc;
    D.P = P;
    std::vector<int64_t> ooff((size_t)F + 1, 0);
    std::vector<uint8_t> cmp0((size_t)F);
    for (int f = 0; f < F; f++) { ooff[(size_t)f + 1] = ooff[f] + (int64_t)feat[f].order.size(); cmp0[f] = feat[f].cmp0; }
    RL_HIP(c->buf.alloc(&D.w, (size_t)P));
    RL_HIP(c->buf.alloc(&D.pot, (size_t)N));
    RL_HIP(c->buf.alloc(&D.best, (size_t)F));
    RL_HIP(c->buf.alloc(&D.bpos, (size_t)F));
    RL_HIP(c->buf.alloc(&D.z, 1));
    RL_HIP(c->buf.alloc(&D.rowoff, (size_t)N + 1));
    RL_HIP(c->buf.alloc(&D.kfirst, (size_t)N));
    RL_HIP(c->buf.alloc(&D.cbeg, (size_t)N));
    RL_HIP(c->buf.alloc(&D.cend, (size_t)N));
    RL_HIP(c->buf.alloc(&D.ooff, (size_t)F + 1));
    RL_HIP(c->buf.alloc(&D.cmp0, (size_t)F));
    RL_HIP(c->buf.alloc(&D.h, (size_t)N));
    RL_HIP(c->buf.alloc(&D.order, (size_t)ooff[(size_t)F]));
    RL_HIP(hipMemcpy(D.rowoff, rowoff.data(), rowoff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(D.kfirst, kfirst.data(), kfirst.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(D.cbeg, cbeg.data(), cbeg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(D.cend, cend.data(), cend.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(D.ooff, ooff.data(), ooff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(D.cmp0, cmp0.data(), cmp0.size(), hipMemcpyHostToDevice));
    for (int f = 0; f < F; f++) {
        if (!feat[f].order.empty())
            RL_HIP(hipMemcpy(D.order + ooff[f], feat[f].order.data(), feat[f].order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        std::vector<uint32_t>().swap(feat[f].order);
    }
    {   // sweight = 1.0 / totalCorrectPairs on every crucial pair (:163-177)
        std::vector<double> w0((size_t)std::min<int64_t>(P, (int64_t)1 << 22), 1.0 / (double)(int32_t)P);
        for (int64_t o = 0; o < P; o += (int64_t)w0.size())
            RL_HIP(hipMemcpy(D.w + o, w0.data(), (size_t)std::min<int64_t>((int64_t)w0.size(), P - o) * sizeof(double), hipMemcpyHostToDevice));
    }
    return RL_OK;
}

// RankBoost.learn() :265-346
static int rb_learn(rl_rb *R)
{
    LinCtx *c = &R->ctx;
    const int F = c->F;
    RbDev D;
    std::vector<RbFeature> feat;
    R->trace.clear(); R->pots.clear();
    R->fid.clear(); R->thr.clear(); R->weight.clear();
    int rc = rb_init(R, D, feat);
    if (rc) return rc;
    CaSet &tr = c->tr, &va = c->va;
    const int64_t N = tr.N, P = D.P;
    RL_HIP(hipMemsetAsync(tr.d_cache, 0, N * sizeof(double), c->stream));                 // the empty ensemble scores 0.0
    if (c->has_valid) RL_HIP(hipMemsetAsync(va.d_cache, 0, va.N * sizeof(double), c->stream));
    const unsigned gridN = (unsigned)((N + 255) / 256);
    const unsigned gridP = (unsigned)std::min<int64_t>((P + 255) / 256, 8192);
    const unsigned gridU = (unsigned)std::min<int64_t>((N + 15) / 16, 8192);
    std::vector<double> best((size_t)F); std::vector<int32_t> bpos((size_t)F);
    double Z_t = 1.0, bestValid = 0.0;                        // Ranker.java:43 bestScoreOnValidationData = 0.0
    int bestLen = 0;
    char msg[400];
    for (int t = 1; t <= R->p.n_iteration; t++) {
        hipLaunchKernelGGL(k_rb_potential, dim3(gridN), dim3(256), 0, c->stream, (const double *)D.w, (const int64_t *)D.rowoff,
                           (const int32_t *)D.kfirst, (const int32_t *)D.cbeg, (const int32_t *)D.cend, D.pot, N);
        RL_HIP(hipGetLastError());
        if (t <= R->p.keep_potentials) {
            R->pots.emplace_back((size_t)N);
            RL_HIP(hipMemcpyAsync(R->pots.back().data(), D.pot, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        hipLaunchKernelGGL(k_rb_cand, dim3((unsigned)F), dim3(kThreads), 0, c->stream, (const double *)D.pot, (const uint32_t *)D.order,
                           (const int64_t *)D.ooff, (const uint8_t *)D.cmp0, D.best, D.bpos);
        RL_HIP(hipGetLastError());
        RL_HIP(hipMemcpyAsync(best.data(), D.best, F * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        RL_HIP(hipMemcpyAsync(bpos.data(), D.bpos, F * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        RL_HIP(hipStreamSynchronize(c->stream));
        int bf = -1; double maxR = -10; int32_t bp = -1;       // the first strict maximum in (feature, threshold) order
        for (int f = 0; f < F; f++)
            if (bpos[f] >= 0 && best[f] > maxR) { maxR = best[f]; bf = f; bp = bpos[f]; }
        if (bf < 0) break;                                     // learnWeakRanker returned null
        const RbFeature &bfeat = feat[(size_t)bf];
        const double thr = bfeat.tval[(size_t)(std::lower_bound(bfeat.end.begin(), bfeat.end.end(), (int64_t)bp) - bfeat.end.begin())];
        const double R_t = Z_t * maxR;
        const double alpha = 0.5 * ada_ln((Z_t + R_t) / (Z_t - R_t));
        const double e_pos = std::exp(alpha), e_neg = std::exp(-alpha);
        if (!std::isfinite(alpha) || !std::isfinite(e_pos)) {
            snprintf(msg, sizeof(msg), "RankBoost round %d: feature index %d at threshold %.17g gives alpha_t = 0.5 ln((Z + R) / (Z - R)) = %.17g "
                     "(exp(alpha_t) = %.17g) with maxR = %.17g, Z = %.17g, R = %.17g; the Java goes on with non-finite weights, not reproduced "
                     "(DESIGN.md 10)", t, bf, thr, alpha, e_pos, maxR, Z_t, R_t);
            return fail(RL_ERR_UNSUPPORTED, msg);
        }
        R->fid.push_back(bf); R->thr.push_back(thr); R->weight.push_back(alpha);
        const float *x = tr.d_xc + (size_t)bf * N;
        hipLaunchKernelGGL(k_rb_weak, dim3(gridN), dim3(256), 0, c->stream, x, N, thr, alpha, tr.d_cache, D.h);
        RL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rb_update, dim3(gridU), dim3(256), 0, c->stream, D.w, (const int64_t *)D.rowoff, (const int32_t *)D.kfirst,
                           (const uint8_t *)D.h, e_pos, e_neg, N);
        RL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rb_zsum, dim3(1), dim3(kThreads), 0, c->stream, (const double *)D.w, P, D.z);
        RL_HIP(hipGetLastError());
        RL_HIP(hipMemcpyAsync(&Z_t, D.z, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        RL_HIP(hipStreamSynchronize(c->stream));
        if (!std::isfinite(Z_t) || Z_t == 0.0) {
            snprintf(msg, sizeof(msg), "RankBoost round %d: Z_t = %.17g after feature index %d at threshold %.17g with alpha_t = %.17g; the Java "
                     "divides every pair weight by it, not reproduced (DESIGN.md 10)", t, Z_t, bf, thr, alpha);
            return fail(RL_ERR_UNSUPPORTED, msg);
        }
        rl_rb_trace_rec rec; memset(&rec, 0, sizeof(rec));
        rec.iteration = t; rec.feature = bf; rec.threshold = thr; rec.max_r = maxR; rec.r_t = R_t; rec.alpha = alpha; rec.z_t = Z_t;
        if ((rc = ca_trials(c, tr, nullptr, nullptr, 1, 0, &rec.train_score))) return rc;
        if (c->has_valid) {
            hipLaunchKernelGGL(k_rb_weak, dim3((unsigned)((va.N + 255) / 256)), dim3(256), 0, c->stream, (const float *)(va.d_xc + (size_t)bf * va.N),
                               va.N, thr, alpha, va.d_cache, (uint8_t *)nullptr);
            RL_HIP(hipGetLastError());
            if ((rc = ca_trials(c, va, nullptr, nullptr, 1, 0, &rec.valid_score))) return rc;
            if (rec.valid_score > bestValid) { bestValid = rec.valid_score; bestLen = t; }
        }
        R->trace.push_back(rec);
        hipLaunchKernelGGL(k_rb_normalize, dim3(gridP), dim3(256), 0, c->stream, D.w, P, Z_t);
        RL_HIP(hipGetLastError());
    }
    RL_HIP(hipStreamSynchronize(c->stream));
    if (c->has_valid && bestLen > 0) { R->fid.resize(bestLen); R->thr.resize(bestLen); R->weight.resize(bestLen); }      // :333-338
    LinModel m;
    m.col = R->fid.data(); m.thr = R->thr.data(); m.w = R->weight.data(); m.nt = m.nw = (int32_t)R->fid.size();
    return lin_finish(c, m);
}

}  // namespace rl

extern "C" {

void rl_rb_params_default(rl_rb_params *p)
{   // learning/boosting/RankBoost.java:38-39
    if (!p) return;
    p->n_iteration = 300; p->n_threshold = 10; p->metric = RL_METRIC_NDCG; p->metric_k = 10; p->device = 0; p->keep_potentials = 0;
    p->err_max = 16.0;
}

int rl_rb_create(const rl_rb_params *p, rl_rb **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<rl_rb> R(new rl_rb());
    R->p = *p;
    int rc = lin_create(&R->ctx, "RankBoost", p->metric, p->metric_k, p->device, p->err_max);
    if (rc) return rc;
    *out = R.release();
    return RL_OK;
}

void rl_rb_destroy(rl_rb *r) { lin_destroy(r); }

int rl_rb_set_train(rl_rb *r, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                    int32_t n_queries, const int32_t *qkey)
{
    int rc = lin_set_train(lin_ctx(r), "rl_rb_", X, n_docs, n_features, labels, qoff, n_queries, qkey);
    if (rc) return rc;
    // init() :152: samples.set(i, samples.get(i).getCorrectRanking()) -- every list in Sorter's order of its labels from here on
    CaSet &d = r->ctx.tr;
    std::vector<int32_t> idx;
    for (int32_t q = 0; q < n_queries; q++) {
        const int a = qoff[q], n = qoff[q + 1] - a;
        rb_sorter(labels + a, n, idx);
        for (int i = 0; i < n; i++) {
            d.labels[(size_t)a + i] = labels[a + idx[i]];
            std::copy(X + (size_t)(a + idx[i]) * n_features, X + (size_t)(a + idx[i] + 1) * n_features, d.X.begin() + (size_t)(a + i) * n_features);
        }
    }
    return RL_OK;
}

int rl_rb_set_validation(rl_rb *r, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                         const int32_t *qkey)
{
    return lin_set_validation(lin_ctx(r), "rl_rb_", X, n_docs, labels, qoff, n_queries, qkey);
}

int rl_rb_set_external_judgments(rl_rb *r, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    return lin_set_external_judgments(lin_ctx(r), "rl_rb_", validation, ideal_dcg, rel_doc_count);
}

int rl_rb_learn(rl_rb *r)
{
    int rc = lin_begin_learn(lin_ctx(r), "rl_rb_");
    if (rc) return rc;
    return rb_learn(r);
}

int rl_rb_get_model(const rl_rb *r, int32_t *fid, double *threshold, double *weight, int32_t cap, int32_t *n)
{
    if (!r || !n) return fail(RL_ERR_INVALID, "null argument");
    if (!r->ctx.learned) return fail(RL_ERR_STATE, "rl_rb_learn has not run");
    *n = (int32_t)r->fid.size();
    const size_t m = std::min<size_t>(r->fid.size(), (size_t)std::max(0, cap));
    if (fid) std::copy(r->fid.begin(), r->fid.begin() + m, fid);
    if (threshold) std::copy(r->thr.begin(), r->thr.begin() + m, threshold);
    if (weight) std::copy(r->weight.begin(), r->weight.begin() + m, weight);
    return RL_OK;
}

int rl_rb_scores(const rl_rb *r, double *train, double *valid) { return lin_scores(lin_ctx(r), "rl_rb_", train, valid); }

int rl_rb_trace(const rl_rb *r, rl_rb_trace_rec *out, int64_t cap, int64_t *n) { return lin_trace(r ? &r->trace : nullptr, out, cap, n); }

int rl_rb_debug_potentials(const rl_rb *r, int32_t round, double *out, int64_t cap)
{
    if (!r || !out) return fail(RL_ERR_INVALID, "null argument");
    if (round < 1 || (size_t)round > r->pots.size())
        return fail(RL_ERR_STATE, "rl_rb_learn kept no potentials of that round (keep_potentials, and the rounds that ran)");
    const std::vector<double> &p = r->pots[(size_t)round - 1];
    if (cap < (int64_t)p.size()) return fail(RL_ERR_INVALID, "potentials buffer too small");
    std::copy(p.begin(), p.end(), out);
    return RL_OK;
}

int rl_rb_predict(int32_t device, const int32_t *feature_ids, const double *thresholds, const double *weights, int32_t n_rankers,
                  const float *X, int64_t n_docs, int32_t row_stride, double *out)
{
    if (!feature_ids || !thresholds || !weights || !out || (n_docs > 0 && !X)) return fail(RL_ERR_INVALID, "null argument");
    if (n_rankers < 0 || n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad sizes");
    LinModel m;
    m.col = feature_ids; m.thr = thresholds; m.w = weights; m.nt = m.nw = n_rankers;
    return lin_predict(device, m, X, n_docs, row_stride, out);
}

}  // extern "C"
