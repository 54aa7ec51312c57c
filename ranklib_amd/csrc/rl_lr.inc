// rl_lr.inc -- Linear Regression (-ranker 9, learning/LinearRegRank.java) on gfx950; included at the end of rl_ca.hip.  The handle holds a
// ranking context (LinCtx, rl_linear.inc: the device sets, the stream, the common entry-point bodies) and ranks with rl_ca.hip's scorer
// (ca_metric) and ranking kernel (k_ca_trials with T = 1 on the cache as it is).
//
// learn() (:44-100) is one accumulation and one solve.  With t = (x_1, ..., x_{nVar-1}, 1) per document, in (list, document) order:
//     xTx[j][k] += t_j * t_k   the product of two widened floats, exact in f64 (24 + 24 significand bits)
//     xTy[j]    += t_j * label a FLOAT product (rounded to f32, f32 subnormals kept), then widened
// Every cell is its own serial f64 chain over all N documents; the cells are independent.  Both sides of a mirrored pair of xTx receive
// the same exact addends in the same order, so the matrix is bitwise symmetric and only the upper triangle is computed.
//
//   k_lr_gram<RB>   a block owns a tile of (16 RB) x (16 RB) cells of the upper triangle (or 64 cells of xTy).  All 256 threads stage slabs
//                   of documents of the tile's row and column features into LDS, coalesced from the column-major set, widened to f64
//                   once (two buffers, the next slab's loads in flight).  Each of the four wavefronts adds one quadrant: a lane carries
//                   RB x RB accumulators, its RB^2 independent chains fill the latency of a dependent f64 add.  The LDS reads (2 RB
//                   per document and wavefront, broadcasts), not the adds, set the pace; one adding wavefront per block was slower
//                   per cell wherever the chip is full (measured: DESIGN.md 11).
//                   The add is fma(t_j, t_k, acc): the product is exact, so the one rounding of the fma IS the rounding of the Java's
//                   multiply-then-add.  It is the only explicit fma in the library (-ffp-contract=off stays); v_mul_f64 + v_add_f64
//                   would double the f64 issue slots of the chain for the same bits.
//
// Scoring is k_lin_score with the bias: score = w[last], then += w[i] * x[features[i]] (LinearRegRank.eval :103-109: bias first).
// The ridge term, solve() (:188-239: Gaussian elimination without pivoting) and the refusals are host code, built with the same flags.

#include <chrono>

#include "rl_knobs.h"

namespace rl {

constexpr int kLrSlab = 3584;          // values staged per slab: 14 per thread
constexpr int kLrLds = 3808;           // doubles per buffer, >= the largest D * (NF + 1) below (112 * 33); two buffers = 59.5 KB of LDS: two blocks per CU
constexpr int kLrYCells = 64;          // xTy cells of a y block: one chain per lane of the adding wavefront

// Value c of the staged vector of document i: Y = false: t_c (x_{c+1}, or 1 for c == C - 1); Y = true: the float product t_c * label.
// In two halves, so that a slab's loads are all in flight together: lr_fetch only loads (no branch: what is out of range reads element
// 0), lr_value turns the loaded pair into the value when the slab is written to LDS.
struct LrRaw { float x, l; };

template <bool Y>
__device__ __forceinline__ LrRaw lr_fetch(const float *xc, const float *lab, int64_t N, int C, int c, int64_t i)
{
    const bool in = i < N && c < C, isx = in && c < C - 1;
    LrRaw r;
    r.x = xc[isx ? (int64_t)c * N + i : (int64_t)0];
    r.l = Y ? lab[in ? i : (int64_t)0] : 0.f;
    return r;
}

template <bool Y>
__device__ __forceinline__ float lr_value(LrRaw r, int64_t N, int C, int c, int64_t i)
{
    const bool in = i < N && c < C, isx = in && c < C - 1;
    const float t = isx ? r.x : in ? 1.f : 0.f;               // t_c, 0 beyond the data
    return Y ? __fmul_rn(t, in ? r.l : 0.f) : t;              // f32 multiply: rounded to float, subnormals kept; 1.f * label is the label
}

// Stages NF values per document, D = kLrSlab / NF documents per slab, row stride NF + 1 doubles (ds_write_b64 of 16 consecutive documents
// then hits 32 different banks; an adding wavefront's ds_read_b64 of one document are broadcasts of <= 16 addresses).  col(f) is the
// global index of staged value f; add(s, m) consumes m documents of a slab.
template <int NF, bool Y, class Col, class Add>
__device__ __forceinline__ void lr_stream(double (*s_t)[kLrLds], const float *xc, const float *lab, int64_t N, int C, Col col, Add add)
{
    constexpr int D = kLrSlab / NF, S = NF + 1, PER = kLrSlab / kThreads;
    static_assert(D * NF == kLrSlab && D * S <= kLrLds && PER * kThreads == kLrSlab, "slab geometry");
    const int tid = threadIdx.x;
    int gc[PER], dd[PER], lo[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int e = u * kThreads + tid, f = e / D;
        dd[u] = e - f * D; gc[u] = col(f); lo[u] = dd[u] * S + f;
    }
    LrRaw v[PER];
    auto load = [&](int64_t base) {
#pragma unroll
        for (int u = 0; u < PER; u++) v[u] = lr_fetch<Y>(xc, lab, N, C, gc[u], base + dd[u]);
    };
    load(0);
    int buf = 0;
    for (int64_t base = 0; base < N; base += D, buf ^= 1) {
#pragma unroll
        for (int u = 0; u < PER; u++) s_t[buf][lo[u]] = (double)lr_value<Y>(v[u], N, C, gc[u], base + dd[u]);
        __syncthreads();
        if (base + D < N) load(base + D);
        add(s_t[buf], (int)min((int64_t)D, N - base));
    }
}

// The adding loop of one full slab: the documents in groups of kLrGroup with two register buffers, the LDS reads of the next group
// written ahead of the adds of this one, so that the compiler can keep reads in flight and wait for them by count, not group by group
constexpr int kLrGroup = 4;

template <int RB>
__device__ __forceinline__ void lr_tile(double (*s_t)[kLrLds], const float *xc, int64_t N, int C, int bj, int bk, double *xtx)
{
    // the block's tile is 16 RB x 16 RB cells: wavefront (wy, wx) owns a quadrant, lane (ty, tx) of it RB x RB cells
    constexpr int T = 16 * RB, NF = 2 * T, D = kLrSlab / NF, S = NF + 1, G = kLrGroup;
    static_assert(D % G == 0, "slab length");
    const int tid = threadIdx.x, w = tid >> 6, ty = (tid >> 3) & 7, tx = tid & 7;
    const int ro = ((w >> 1) * 8 + ty) * RB, co = T + ((w & 1) * 8 + tx) * RB;
    double acc[RB][RB];
#pragma unroll
    for (int r = 0; r < RB; r++)
#pragma unroll
        for (int c = 0; c < RB; c++) acc[r][c] = 0.0;
    auto read = [&](const double *row, double *a, double *b) {
#pragma unroll
        for (int r = 0; r < RB; r++) a[r] = row[ro + r];
#pragma unroll
        for (int c = 0; c < RB; c++) b[c] = row[co + c];
    };
    auto add = [&](const double *a, const double *b) {
#pragma unroll
        for (int r = 0; r < RB; r++)
#pragma unroll
            for (int c = 0; c < RB; c++) acc[r][c] = __builtin_fma(a[r], b[c], acc[r][c]);     // exact product: see the head of the file
    };
    lr_stream<NF, false>(s_t, xc, nullptr, N, C, [&](int f) { return (f < T ? bj : bk) * T + (f < T ? f : f - T); },
                         [&](const double *s, int m) {
                             double a[2][G][RB], b[2][G][RB];
                             if (m == D) {
#pragma unroll
                                 for (int g = 0; g < G; g++) read(s + g * S, a[0][g], b[0][g]);
#pragma unroll 2
                                 for (int d = 0; d < D; d += 2 * G) {
#pragma unroll
                                     for (int g = 0; g < G; g++) read(s + min(d + G + g, D - 1) * S, a[1][g], b[1][g]);
#pragma unroll
                                     for (int g = 0; g < G; g++) add(a[0][g], b[0][g]);
                                     if (d + G < D) {
#pragma unroll
                                         for (int g = 0; g < G; g++) read(s + min(d + 2 * G + g, D - 1) * S, a[0][g], b[0][g]);
#pragma unroll
                                         for (int g = 0; g < G; g++) add(a[1][g], b[1][g]);
                                     }
                                 }
                             } else {
                                 for (int d = 0; d < m; d++) { read(s + d * S, a[0][0], b[0][0]); add(a[0][0], b[0][0]); }
                             }
                         });
#pragma unroll
    for (int r = 0; r < RB; r++)
#pragma unroll
        for (int c = 0; c < RB; c++) {
            const int j = bj * T + ro + r, k = bk * T + (co - T) + c;
            if (j < C && k < C) {
                xtx[(size_t)j * C + k] = acc[r][c];
                if (bj != bk) xtx[(size_t)k * C + j] = acc[r][c];      // a diagonal tile computes both of its triangles itself
            }
        }
}

// 64 cells of xTy: 16 lanes of each of the four wavefronts carry one chain each (four wavefronts reading, one per SIMD, is what the LDS
// serves at its rate; the other lanes repeat a neighbour's reads and write nothing)
__device__ __forceinline__ void lr_ytile(double (*s_t)[kLrLds], const float *xc, const float *lab, int64_t N, int C, int bj, double *xty)
{
    constexpr int NF = kLrYCells, D = kLrSlab / NF, S = NF + 1, G = kLrGroup;
    static_assert(D % (2 * G) == 0, "slab length");
    const int tid = threadIdx.x, f = (tid >> 6) * 16 + (tid & 15);
    double acc = 0.0;
    lr_stream<NF, true>(s_t, xc, lab, N, C, [&](int v) { return bj * NF + v; },
                        [&](const double *s, int m) {
                            double a[2][G];
                            if (m == D) {
#pragma unroll
                                for (int g = 0; g < G; g++) a[0][g] = s[g * S + f];
#pragma unroll 2
                                for (int d = 0; d < D; d += 2 * G) {
#pragma unroll
                                    for (int g = 0; g < G; g++) a[1][g] = s[(d + G + g) * S + f];
#pragma unroll
                                    for (int g = 0; g < G; g++) acc += a[0][g];
#pragma unroll
                                    for (int g = 0; g < G; g++) a[0][g] = s[min(d + 2 * G + g, D - 1) * S + f];
#pragma unroll
                                    for (int g = 0; g < G; g++) acc += a[1][g];
                                }
                            } else {
                                for (int d = 0; d < m; d++) acc += s[d * S + f];
                            }
                        });
    const int c = bj * NF + f;
    if ((tid & 63) < 16 && c < C) xty[c] = acc;
}

// blocks [0, ntri): the tiles (bj <= bk) of the upper triangle, row by row; blocks [ntri, ...): 64 cells of xTy each
template <int RB>
__global__ __launch_bounds__(kThreads) void k_lr_gram(const float *xc, const float *lab, int64_t N, int C, int nt, int ntri, double *xtx,
                                                      double *xty)
{
    __shared__ double s_t[2][kLrLds];
    const int b = blockIdx.x;
    if (b < ntri) {
        int bj = 0, rem = b;
        while (rem >= nt - bj) { rem -= nt - bj; bj++; }
        lr_tile<RB>(s_t, xc, N, C, bj, bj + rem, xtx);
    } else {
        lr_ytile(s_t, xc, lab, N, C, b - ntri, xty);
    }
}

}  // namespace rl

struct rl_lr {
    rl_lr_params p;
    LinCtx ctx;
    bool gram_done = false;
    int32_t n_var = 0;                 // the Java's nVar (0: the training set's column count)
    bool has_cols = false;
    std::vector<int32_t> cols;         // eval's columns (features[i] - 1; -1 reads 0)
    std::vector<double> xtx, xty, weight;
    double gram_ms = 0, solve_ms = 0, score_ms = 0;
    int32_t rb = 0;
    int32_t rb_knob = 0;               // RLHIP_LR_RB when it names a register block (1 / 2 / 4), else 0: lr_pick_rb chooses
};

namespace rl {

static int lr_blocks(int C, int rb) { const int nt = (C + 16 * rb - 1) / (16 * rb); return nt * (nt + 1) / 2 + (C + kLrYCells - 1) / kLrYCells; }

// The register block, by a model: a lane's RB^2 chains cost max(13, 4 RB^2) cycles a document (the latency of one dependent f64 add against
// the issue of RB^2 wave64 f64 operations), and the chip runs about 512 blocks at a time (two 59.5 KB blocks per CU).  The measured costs
// are higher (the LDS reads set them), but the sweeps at 46, 136 and 700 columns agree with every choice it makes (DESIGN.md 11).
// rl_lr::rb_knob overrides.
static int lr_pick_rb(int C, int rb_knob)
{
    if (rb_knob) return rb_knob;
    int best = 1; int64_t bc = 0;
    for (int rb = 1; rb <= 4; rb *= 2) {
        const int64_t cost = (int64_t)((lr_blocks(C, rb) + 511) / 512) * std::max(13, 4 * rb * rb);
        if (rb == 1 || cost < bc) { best = rb; bc = cost; }
    }
    return best;
}

static std::string lr_colname(int j, int n)
{
    return j == n - 1 ? std::string("the constant's column") : "the column of feature " + std::to_string(j + 1);
}

// LinearRegRank.solve (:188-239), the Java's loop order; a zero or non-finite pivot and non-finite weights are refused
static int lr_solve(std::vector<double> &a, std::vector<double> &b, int n, std::vector<double> &x)
{
    auto bad = [&](int j, double pivot) {
        char msg[400];
        snprintf(msg, sizeof(msg), "Linear Regression: the pivot of %s is %.17g in the elimination without pivoting (an empty or dependent column "
                 "and too small a -L2); the Java goes on with NaN weights, not reproduced (DESIGN.md 11)", lr_colname(j, n).c_str(), pivot);
        return fail(RL_ERR_UNSUPPORTED, msg);
    };
    for (int j = 0; j < n - 1; j++) {
        const double pivot = a[(size_t)j * n + j];
        if (pivot == 0.0 || !std::isfinite(pivot)) return bad(j, pivot);
        for (int i = j + 1; i < n; i++) {
            const double multiplier = a[(size_t)i * n + j] / pivot;
            double *ai = &a[(size_t)i * n];
            const double *aj = &a[(size_t)j * n];
            for (int k = j + 1; k < n; k++) ai[k] -= aj[k] * multiplier;
            b[i] -= b[j] * multiplier;
        }
    }
    if (a[(size_t)(n - 1) * n + n - 1] == 0.0 || !std::isfinite(a[(size_t)(n - 1) * n + n - 1])) return bad(n - 1, a[(size_t)(n - 1) * n + n - 1]);
    x.assign((size_t)n, 0.0);
    x[n - 1] = b[n - 1] / a[(size_t)(n - 1) * n + n - 1];
    for (int i = n - 2; i >= 0; i--) {
        double val = b[i];
        for (int j = i + 1; j < n; j++) val -= a[(size_t)i * n + j] * x[j];
        x[i] = val / a[(size_t)i * n + i];
    }
    for (int i = 0; i < n; i++)
        if (!std::isfinite(x[i])) {
            char msg[300];
            snprintf(msg, sizeof(msg), "Linear Regression: the weight of %s is %.17g after the solve; the Java goes on with it, not reproduced "
                     "(DESIGN.md 11)", lr_colname(i, n).c_str(), x[i]);
            return fail(RL_ERR_UNSUPPORTED, msg);
        }
    return RL_OK;
}

static int lr_gram(rl_lr *R)
{
    LinCtx *c = &R->ctx;
    CaSet &d = c->tr;
    const int C = R->n_var;
    const int rb = R->rb = lr_pick_rb(C, R->rb_knob);
    const int nt = (C + 16 * rb - 1) / (16 * rb), ntri = nt * (nt + 1) / 2;
    const unsigned grid = (unsigned)lr_blocks(C, rb);
    double *dxtx = nullptr, *dxty = nullptr;
    RL_HIP(c->buf.alloc(&dxtx, (size_t)C * C));
    RL_HIP(c->buf.alloc(&dxty, (size_t)C));
    hipEvent_t e0, e1;
    RL_HIP(hipEventCreate(&e0)); RL_HIP(hipEventCreate(&e1));
    RL_HIP(hipEventRecord(e0, c->stream));
    if (rb == 1) hipLaunchKernelGGL(k_lr_gram<1>, dim3(grid), dim3(kThreads), 0, c->stream, (const float *)d.d_xc, (const float *)d.d_labels, d.N, C, nt, ntri, dxtx, dxty);
    else if (rb == 2) hipLaunchKernelGGL(k_lr_gram<2>, dim3(grid), dim3(kThreads), 0, c->stream, (const float *)d.d_xc, (const float *)d.d_labels, d.N, C, nt, ntri, dxtx, dxty);
    else hipLaunchKernelGGL(k_lr_gram<4>, dim3(grid), dim3(kThreads), 0, c->stream, (const float *)d.d_xc, (const float *)d.d_labels, d.N, C, nt, ntri, dxtx, dxty);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) le = hipEventRecord(e1, c->stream);
    if (le == hipSuccess) le = hipEventSynchronize(e1);
    float ms = 0.f;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    RL_HIP(le);
    R->gram_ms = ms;
    R->xtx.assign((size_t)C * C, 0.0); R->xty.assign((size_t)C, 0.0);
    RL_HIP(hipMemcpy(R->xtx.data(), dxtx, R->xtx.size() * sizeof(double), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(R->xty.data(), dxty, R->xty.size() * sizeof(double), hipMemcpyDeviceToHost));
    R->gram_done = true;
    return RL_OK;
}

// LinearRegRank.learn() :44-100
static int lr_learn(rl_lr *R)
{
    LinCtx *c = &R->ctx;
    const int W = c->F;
    if (R->n_var == 0) R->n_var = W;
    const int n = R->n_var;
    if (!R->has_cols) { R->cols.resize((size_t)W); for (int i = 0; i < W; i++) R->cols[i] = i; }
    if ((int)R->cols.size() > n)
        return fail(RL_ERR_UNSUPPORTED, "Linear Regression: " + std::to_string(R->cols.size()) + " features to score with, but only " +
                                        std::to_string(n) + " weights (nVar = the largest feature id of the training lists); the Java ends in an "
                                        "ArrayIndexOutOfBoundsException in eval (DESIGN.md 11)");
    int rc = ca_prepare(c);                                   // uploads the sets (and drops the host rows)
    if (rc) return rc;
    if ((rc = lr_gram(R))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> a = R->xtx, b = R->xty;
    if (R->p.lambda != 0.0)                                   // :84-89
        for (int i = 0; i < n; i++) a[(size_t)i * n + i] += R->p.lambda;
    if ((rc = lr_solve(a, b, n, R->weight))) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    R->solve_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    LinModel m;                                               // eval :103-109: the bias w[n - 1], then the columns
    m.col = R->cols.data(); m.nt = (int32_t)R->cols.size(); m.w = R->weight.data(); m.nw = (int32_t)R->weight.size(); m.bias = true;
    if ((rc = lin_finish(c, m))) return rc;
    R->score_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    return RL_OK;
}

}  // namespace rl

extern "C" {

void rl_lr_params_default(rl_lr_params *p)
{   // learning/LinearRegRank.java:26
    if (!p) return;
    p->lambda = 1E-10; p->metric = RL_METRIC_NDCG; p->metric_k = 10; p->device = 0; p->err_max = 16.0;
}

int rl_lr_create(const rl_lr_params *p, rl_lr **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!std::isfinite(p->lambda)) return fail(RL_ERR_INVALID, "lambda (-L2) must be finite");
    std::unique_ptr<rl_lr> R(new rl_lr());
    R->p = *p;
    R->rb_knob = read_lr_rb_knob();
    int rc = lin_create(&R->ctx, "Linear Regression", p->metric, p->metric_k, p->device, p->err_max);
    if (rc) return rc;
    *out = R.release();
    return RL_OK;
}

void rl_lr_destroy(rl_lr *r) { lin_destroy(r); }

int rl_lr_set_train(rl_lr *r, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                    int32_t n_queries, const int32_t *qkey)
{
    return lin_set_train(lin_ctx(r), "rl_lr_", X, n_docs, n_features, labels, qoff, n_queries, qkey);
}

int rl_lr_set_validation(rl_lr *r, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                         const int32_t *qkey)
{
    return lin_set_validation(lin_ctx(r), "rl_lr_", X, n_docs, labels, qoff, n_queries, qkey);
}

int rl_lr_set_external_judgments(rl_lr *r, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    return lin_set_external_judgments(lin_ctx(r), "rl_lr_", validation, ideal_dcg, rel_doc_count);
}

int rl_lr_set_features(rl_lr *r, int32_t n_var, const int32_t *eval_cols, int32_t n_eval)
{
    if (!r) return fail(RL_ERR_INVALID, "null handle");
    if (!r->ctx.has_train) return fail(RL_ERR_STATE, "set the training data first");
    if (r->ctx.uploaded) return fail(RL_ERR_STATE, "rl_lr_set_features after rl_lr_learn");
    if (n_var < 0 || n_var > r->ctx.F) return fail(RL_ERR_INVALID, "n_var must be 0 (all columns) or 1 .. n_features");
    if (n_eval < 0 || (n_eval > 0 && !eval_cols)) return fail(RL_ERR_INVALID, "bad eval columns");
    for (int32_t i = 0; i < n_eval; i++)
        if (eval_cols[i] < -1 || eval_cols[i] >= r->ctx.F) return fail(RL_ERR_INVALID, "eval column out of range (-1 .. n_features - 1)");
    r->n_var = n_var;
    r->has_cols = eval_cols != nullptr;                      // NULL: columns 0 .. n_features - 1
    r->cols.clear();
    if (eval_cols) r->cols.assign(eval_cols, eval_cols + n_eval);
    return RL_OK;
}

int rl_lr_learn(rl_lr *r)
{
    int rc = lin_begin_learn(lin_ctx(r), "rl_lr_");
    if (rc) return rc;
    return lr_learn(r);
}

int rl_lr_get_weights(const rl_lr *r, double *w, int32_t cap, int32_t *n)
{
    if (!r || !n) return fail(RL_ERR_INVALID, "null argument");
    if (!r->ctx.learned) return fail(RL_ERR_STATE, "rl_lr_learn has not run");
    *n = (int32_t)r->weight.size();
    if (w) std::copy(r->weight.begin(), r->weight.begin() + std::min<size_t>(r->weight.size(), (size_t)std::max(0, cap)), w);
    return RL_OK;
}

int rl_lr_scores(const rl_lr *r, double *train, double *valid) { return lin_scores(lin_ctx(r), "rl_lr_", train, valid); }

int rl_lr_debug_gram(const rl_lr *r, double *xtx, double *xty, int32_t cap, int32_t *n_var)
{
    if (!r || !n_var) return fail(RL_ERR_INVALID, "null argument");
    if (!r->gram_done) return fail(RL_ERR_STATE, "rl_lr_learn has not accumulated xTx yet");
    *n_var = r->n_var;
    if (!xtx && !xty) return RL_OK;
    if (cap < r->n_var) return fail(RL_ERR_INVALID, "gram buffers too small");
    if (xtx) std::copy(r->xtx.begin(), r->xtx.end(), xtx);
    if (xty) std::copy(r->xty.begin(), r->xty.end(), xty);
    return RL_OK;
}

int rl_lr_debug_times(const rl_lr *r, double *gram_ms, double *solve_ms, double *score_ms, int32_t *register_block)
{
    if (!r) return fail(RL_ERR_INVALID, "null handle");
    if (!r->gram_done) return fail(RL_ERR_STATE, "rl_lr_learn has not run");
    if (gram_ms) *gram_ms = r->gram_ms;
    if (solve_ms) *solve_ms = r->solve_ms;
    if (score_ms) *score_ms = r->score_ms;
    if (register_block) *register_block = r->rb;
    return RL_OK;
}

int rl_lr_predict(int32_t device, const int32_t *feature_ids, int32_t n_features, const double *weights, int32_t n_weights, const float *X,
                  int64_t n_docs, int32_t row_stride, double *out)
{
    if (!weights || !out || (n_features > 0 && !feature_ids) || (n_docs > 0 && !X)) return fail(RL_ERR_INVALID, "null argument");
    if (n_features < 0 || n_weights < 1 || n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad sizes");
    if (n_features > n_weights)
        return fail(RL_ERR_UNSUPPORTED, "Linear Regression: " + std::to_string(n_features) + " features to score with, but only " +
                                        std::to_string(n_weights) + " weights; the Java ends in an ArrayIndexOutOfBoundsException in eval "
                                        "(DESIGN.md 11)");
    LinModel m;
    m.col = feature_ids; m.nt = n_features; m.w = weights; m.nw = n_weights; m.bias = true;
    return lin_predict(device, m, X, n_docs, row_stride, out);
}

}  // extern "C"
