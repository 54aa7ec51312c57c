// rl_ln.inc -- ListNet training (-ranker 7, learning/neuralnet/ListNet.java learn :101-140, ListNeuron.java) on gfx950; included at the end
// of rl_ca.hip.  The handle holds a ranking context (LinCtx, rl_linear.inc) and ranks with k_ca_trials (T = 1 on the cache as it is).
//
// The network is F inputs and a bias neuron feeding ONE logistic output neuron (ListNet.init :84-98, no hidden layer): F + 1 weights in
// inLinks order, inputs 0 .. F - 1 and the bias last.  learn() updates them once per ranked list, list after list:
//     o_i  = 1 / (1 + exp(-wsum_i)),  wsum_i = 0.0, += (double)x_ik * w_k for k = 0 .. F - 1, += 1.0 * w_F           (Neuron.computeOutput :78-87)
//     d1_i = exp((double)label_i) / sum_j exp(label_j),  d2_i = exp(o_i) / sum_j exp(o_j)       both sums serial, j in order (ListNeuron :18-33)
//     w_k += lr * (sum_l (d1_l - d2_l) * x_lk)          the sum serial, l in order; then one multiply, one add                (ListNeuron :36-49)
// every operation its own f64 rounding (-ffp-contract=off), exp = exp_fdlibm, the logistic = rho_fdlibm of rl_device.h.
//
//   k_ln_label_exp   once per set, a thread per list: d1_i.  It depends on the labels alone, so no epoch computes it again.
//   k_ln_epoch       one launch per epoch and ONE workgroup that walks all lists in order: list q's forward pass reads the weights list
//                    q - 1 wrote, and that dependency is the algorithm.  The weights stay in LDS for the whole epoch (in global memory when
//                    F + 1 > kLnMaxW: k_ln_epoch<false>); the per-document values of a list in LDS (in a global scratch of maxq doubles
//                    when the list is longer than kLnDocCap).  Per list: (1) forward, a document per lane, coalesced over the column-major set, then exp(o_i);
//                    (2) the sum of exp(o_j) as one serial chain: wavefront 0 reads 64 values at a time and adds them lane after lane
//                    (v_readlane, no LDS round trip per addend); (3) d1_i - d2_i, parallel; (4) the update, a weight per lane, each a serial
//                    chain over the list's documents.  Every loop bound is block-uniform: each __syncthreads() is reached by all threads.
//   k_ln_score       the forward pass over a whole set at full width, for the per-epoch metric: rl_net_predict's bits on the same rows.
//
// The host loop (ln_learn) is ListNet.learn(): epoch kernel, scorer.score(rank(.)) of both sets, the strict `>` on the validation score,
// the save, and after the last epoch the restore.  Weights that are not all finite after an epoch are refused.

#include <chrono>

#include "rl_knobs.h"

namespace rl {

constexpr int kLnMaxW = 4096;          // weights kept in LDS (32 KB); more: k_ln_epoch<false> works on the global copy
constexpr int kLnDocCap = 2048;        // per-document values of a list kept in LDS (16 KB); longer lists: the handle's global scratch

struct LnArgs {
    const float *xc; const double *d1; const int32_t *qoff;
    double *w;                 // [F + 1], read at the start and written at the end of an epoch
    double *scratch;           // [maxq]
    int64_t N; int32_t F, Q;
    double lr;
};

__device__ __forceinline__ double ln_readlane(double v, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// wsum of document i (column-major set) and the logistic of it
__device__ __forceinline__ double ln_output(const float *xc, int64_t N, int64_t i, int F, const double *w)
{
    const float *x = xc + i;
    double wsum = 0.0;
#pragma unroll 8
    for (int k = 0; k < F; k++) wsum += (double)x[(int64_t)k * N] * w[k];
    wsum += 1.0 * w[F];
    return rho_fdlibm(-wsum);
}

// a thread per list: d1_i = exp(label_i) / sumLabelExp (ListNeuron.computeDelta :19-31, the label half)
__global__ void k_ln_label_exp(const float *labels, const int32_t *qoff, int32_t Q, double *d1)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const int a = qoff[q], b = qoff[q + 1];
    double sum = 0;
    for (int i = a; i < b; i++) { const double e = exp_fdlibm((double)labels[i]); d1[i] = e; sum += e; }
    for (int i = a; i < b; i++) d1[i] = d1[i] / sum;
}

// SKIP (a measuring aid, rl_ln::skip): 1 leaves out the forward pass, 2 the sum chain, 4 the update; the results are then meaningless
template <bool WLDS, int SKIP>
__global__ __launch_bounds__(kThreads) void k_ln_epoch(const LnArgs a)
{
    __shared__ double s_w[WLDS ? kLnMaxW : 1];
    __shared__ double s_v[kLnDocCap];
    __shared__ double s_sum;
    const int tid = threadIdx.x, F = a.F, C = F + 1;
    double *w = WLDS ? s_w : a.w;
    if (WLDS) {
        for (int k = tid; k < C; k += kThreads) s_w[k] = a.w[k];
        __syncthreads();
    }
    for (int q = 0; q < a.Q; q++) {
        const int cur = a.qoff[q], n = a.qoff[q + 1] - cur;
        double *v = n <= kLnDocCap ? s_v : a.scratch;
        for (int i = tid; i < n; i += kThreads) v[i] = (SKIP & 1) ? 1.0 : exp_fdlibm(ln_output(a.xc, a.N, (int64_t)cur + i, F, w));
        __syncthreads();
        if ((SKIP & 2) && tid == 0) s_sum = (double)n;
        if (!(SKIP & 2) && tid < kWave) {                                   // sumScoreExp: every lane of wavefront 0 carries the same chain
            double s = 0;
            for (int i0 = 0; i0 < n; i0 += kWave) {
                const double val = i0 + tid < n ? v[i0 + tid] : 0.0;
                const int m = min(kWave, n - i0);
                for (int j = 0; j < m; j++) s += ln_readlane(val, j);
            }
            if (tid == 0) s_sum = s;
        }
        __syncthreads();
        const double sum = s_sum;
        for (int i = tid; i < n; i += kThreads) v[i] = a.d1[cur + i] - v[i] / sum;
        __syncthreads();
        for (int k = tid; k < C && !(SKIP & 4); k += kThreads) {
            double dw = 0;
            if (k < F) {
                const float *x = a.xc + (int64_t)k * a.N + cur;
#pragma unroll 8
                for (int l = 0; l < n; l++) dw += v[l] * (double)x[l];
            } else {
#pragma unroll 8
                for (int l = 0; l < n; l++) dw += v[l] * 1.0;
            }
            dw *= a.lr;
            w[k] += dw;
        }
        __syncthreads();                                     // the next list reads these weights and reuses v and s_sum
    }
    if (WLDS)
        for (int k = tid; k < C; k += kThreads) a.w[k] = s_w[k];
}

__global__ __launch_bounds__(kThreads) void k_ln_score(double *out, const float *xc, int64_t n, int32_t F, const double *__restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = ln_output(xc, n, i, F, w);
}

}  // namespace rl

struct rl_ln {
    rl_ln_params p;
    LinCtx ctx;
    std::vector<double> start, weight;     // the weights rl_ln_set_weights gave; after learn: the restored best or the last epoch's
    std::vector<rl_ln_trace_rec> trace;
    double epoch_ms = 0, score_ms = 0;
    int32_t skip = 0;                      // RLHIP_LN_SKIP (rl_knobs.h): the phase k_ln_epoch leaves out, for tools/ln_bench.py
};

namespace rl {

static int ln_score_set(LinCtx *c, CaSet &d, const double *dw, double *score)
{
    hipLaunchKernelGGL(k_ln_score, dim3((unsigned)((d.N + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, d.d_cache,
                       (const float *)d.d_xc, d.N, c->F, dw);
    RL_HIP(hipGetLastError());
    return ca_trials(c, d, nullptr, nullptr, 1, 0, score);       // synchronises the stream
}

// ListNet.learn() :101-140
static int ln_learn(rl_ln *h)
{
    LinCtx *c = &h->ctx;
    CaSet &d = c->tr;
    const int C = c->F + 1;
    int rc = ca_prepare(c);                                   // uploads the sets (and drops the host rows)
    if (rc) return rc;
    LnArgs a;
    double *dw = nullptr, *dd1 = nullptr, *dscr = nullptr;
    RL_HIP(c->buf.alloc(&dw, (size_t)C));
    RL_HIP(c->buf.alloc(&dd1, (size_t)d.N));
    RL_HIP(c->buf.alloc(&dscr, (size_t)d.maxq));
    a.xc = d.d_xc; a.d1 = dd1; a.qoff = d.d_qoff; a.w = dw; a.scratch = dscr; a.N = d.N; a.F = c->F; a.Q = d.Q; a.lr = h->p.learning_rate;
    hipLaunchKernelGGL(k_ln_label_exp, dim3((unsigned)((d.Q + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                       (const float *)d.d_labels, (const int32_t *)d.d_qoff, d.Q, dd1);
    RL_HIP(hipGetLastError());
    h->weight = h->start;
    RL_HIP(hipMemcpyAsync(dw, h->weight.data(), C * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipEvent_t e0, e1;
    RL_HIP(hipEventCreate(&e0)); RL_HIP(hipEventCreate(&e1));
    struct Events { hipEvent_t a, b; ~Events() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    h->trace.clear(); h->epoch_ms = h->score_ms = 0;
    std::vector<double> best;
    double bestScore = 0.0;                                   // Ranker.bestScoreOnValidationData
    for (int epoch = 1; epoch <= h->p.n_epochs; epoch++) {
        RL_HIP(hipEventRecord(e0, c->stream));
        if (C > kLnMaxW) hipLaunchKernelGGL((k_ln_epoch<false, 0>), dim3(1), dim3(kThreads), 0, c->stream, a);
        else if (h->skip == 1) hipLaunchKernelGGL((k_ln_epoch<true, 1>), dim3(1), dim3(kThreads), 0, c->stream, a);
        else if (h->skip == 2) hipLaunchKernelGGL((k_ln_epoch<true, 2>), dim3(1), dim3(kThreads), 0, c->stream, a);
        else if (h->skip == 4) hipLaunchKernelGGL((k_ln_epoch<true, 4>), dim3(1), dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL((k_ln_epoch<true, 0>), dim3(1), dim3(kThreads), 0, c->stream, a);
        RL_HIP(hipGetLastError());
        RL_HIP(hipEventRecord(e1, c->stream));
        RL_HIP(hipMemcpyAsync(h->weight.data(), dw, C * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        RL_HIP(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        RL_HIP(hipEventElapsedTime(&ms, e0, e1));
        h->epoch_ms += ms;
        for (int k = 0; k < C; k++)
            if (!std::isfinite(h->weight[k])) {
                char msg[300];
                snprintf(msg, sizeof(msg), "ListNet: weight %d is %.17g after epoch %d (a learning rate too large for the data); the Java goes "
                         "on with it, not reproduced (DESIGN.md 15)", k, h->weight[k], epoch);
                return fail(RL_ERR_UNSUPPORTED, msg);
            }
        const auto t0 = std::chrono::steady_clock::now();
        rl_ln_trace_rec r; r.epoch = epoch; r.saved = 0; r.train = 0; r.valid = 0;
        if ((rc = ln_score_set(c, d, dw, &r.train))) return rc;
        if (c->has_valid) {
            if ((rc = ln_score_set(c, c->va, dw, &r.valid))) return rc;
            if (r.valid > bestScore) { bestScore = r.valid; best = h->weight; r.saved = 1; }      // :117-120, strict
        }
        h->score_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        h->trace.push_back(r);
    }
    if (c->has_valid) {                                       // restoreBestModelOnValidation (RankNet.java:206-223)
        if (best.empty())
            return fail(RL_ERR_NO_BEST, "ListNet: no epoch scored above 0.0 on the validation set, so no model was saved; the Java's "
                                        "restoreBestModelOnValidation throws here");
        h->weight = best;
        RL_HIP(hipMemcpyAsync(dw, h->weight.data(), C * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = ln_score_set(c, d, dw, &c->train_score))) return rc;
    c->valid_score = 0;
    if (c->has_valid && (rc = ln_score_set(c, c->va, dw, &c->valid_score))) return rc;
    c->learned = true;
    return RL_OK;
}

}  // namespace rl

extern "C" {

void rl_ln_params_default(rl_ln_params *p)
{   // learning/neuralnet/ListNet.java:29-30
    if (!p) return;
    p->n_epochs = 1500; p->learning_rate = 0.00001; p->metric = RL_METRIC_NDCG; p->metric_k = 10; p->device = 0; p->err_max = 16.0;
}

int rl_ln_create(const rl_ln_params *p, rl_ln **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    if (p->n_epochs < 0) return fail(RL_ERR_INVALID, "n_epochs (-epoch) must not be negative");
    if (!std::isfinite(p->learning_rate)) return fail(RL_ERR_INVALID, "learning_rate must be finite");
    std::unique_ptr<rl_ln> h(new rl_ln());
    h->p = *p;
    h->skip = read_ln_skip_knob();
    int rc = lin_create(&h->ctx, "ListNet", p->metric, p->metric_k, p->device, p->err_max);
    if (rc) return rc;
    *out = h.release();
    return RL_OK;
}

void rl_ln_destroy(rl_ln *h) { lin_destroy(h); }

int rl_ln_set_train(rl_ln *h, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                    int32_t n_queries, const int32_t *qkey)
{
    int rc = lin_set_train(lin_ctx(h), "rl_ln_", X, n_docs, n_features, labels, qoff, n_queries, qkey);
    if (rc == RL_OK) h->start.clear();                       // the weights belong to a feature count
    return rc;
}

int rl_ln_set_validation(rl_ln *h, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                         const int32_t *qkey)
{
    return lin_set_validation(lin_ctx(h), "rl_ln_", X, n_docs, labels, qoff, n_queries, qkey);
}

int rl_ln_set_external_judgments(rl_ln *h, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    return lin_set_external_judgments(lin_ctx(h), "rl_ln_", validation, ideal_dcg, rel_doc_count);
}

int rl_ln_set_weights(rl_ln *h, const double *w, int32_t n)
{
    if (!h || !w) return fail(RL_ERR_INVALID, "null argument");
    if (!h->ctx.has_train) return fail(RL_ERR_INVALID, "rl_ln_set_weights: set the training data first (n must be n_features + 1)");
    if (h->ctx.uploaded) return fail(RL_ERR_STATE, "rl_ln_set_weights after rl_ln_learn");
    if (n != h->ctx.F + 1)
        return fail(RL_ERR_INVALID, "rl_ln_set_weights: n is " + std::to_string(n) + ", the network has " + std::to_string(h->ctx.F + 1) +
                                    " weights (n_features inputs and the bias)");
    h->start.assign(w, w + n);
    return RL_OK;
}

int rl_ln_learn(rl_ln *h)
{
    if (!h) return fail(RL_ERR_INVALID, "null handle");
    if (!h->ctx.has_train) return fail(RL_ERR_INVALID, "rl_ln_learn: set the training data first");
    if (h->start.empty()) return fail(RL_ERR_INVALID, "rl_ln_learn: set the start weights first (rl_ln_set_weights)");
    int rc = lin_begin_learn(lin_ctx(h), "rl_ln_");
    if (rc) return rc;
    return ln_learn(h);
}

int rl_ln_get_weights(const rl_ln *h, double *w, int32_t cap, int32_t *n)
{
    if (!h || !n) return fail(RL_ERR_INVALID, "null argument");
    if (!h->ctx.learned) return fail(RL_ERR_STATE, "rl_ln_learn has not run");
    *n = (int32_t)h->weight.size();
    if (w) std::copy(h->weight.begin(), h->weight.begin() + std::min<size_t>(h->weight.size(), (size_t)std::max(0, cap)), w);
    return RL_OK;
}

int rl_ln_scores(const rl_ln *h, double *train, double *valid) { return lin_scores(lin_ctx(h), "rl_ln_", train, valid); }

int rl_ln_trace(const rl_ln *h, rl_ln_trace_rec *out, int64_t cap, int64_t *n) { return lin_trace(h ? &h->trace : nullptr, out, cap, n); }

int rl_ln_debug_doc_scores(const rl_ln *h, int32_t validation, double *out, int64_t cap)
{
    if (!h || !out) return fail(RL_ERR_INVALID, "null argument");
    if (!h->ctx.learned) return fail(RL_ERR_STATE, "rl_ln_learn has not run");
    if (validation && !h->ctx.has_valid) return fail(RL_ERR_STATE, "no validation set");
    const CaSet &d = validation ? h->ctx.va : h->ctx.tr;
    if (cap < d.N) return fail(RL_ERR_INVALID, "score buffer too small");
    RL_HIP(hipSetDevice(h->ctx.device));
    RL_HIP(hipMemcpy(out, d.d_cache, (size_t)d.N * sizeof(double), hipMemcpyDeviceToHost));
    return RL_OK;
}

int rl_ln_debug_times(const rl_ln *h, double *epoch_ms, double *score_ms)
{
    if (!h) return fail(RL_ERR_INVALID, "null handle");
    if (!h->ctx.uploaded) return fail(RL_ERR_STATE, "rl_ln_learn has not run");
    if (epoch_ms) *epoch_ms = h->epoch_ms;
    if (score_ms) *score_ms = h->score_ms;
    return RL_OK;
}

}  // extern "C"
