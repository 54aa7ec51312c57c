// rl_linear.inc -- what the four linear rankers (Coordinate Ascent, AdaRank, RankBoost, Linear Regression) share; included first by
// rl_ca.hip.  Each of their handles holds one LinCtx and its own parameters, model and trace.
//
//   LinCtx          the ranking context: the metric, the device and its stream, the training and validation sets on the device (CaSet),
//                   the scorer's tables and the buffers of the ranking kernel (k_ca_trials, rl_ca.hip), and the final scores.
//   k_lin_score     the one document-scoring kernel: s = start, then s += w[t] * term(x[col[t]]) in index order.  start is 0.0 or
//                   w[nw - 1] (LinearRegRank.eval: bias first); the term is the value or RBWeakRanker's [value > thr[t]].  Column-major
//                   sets (training: col == null is the identity) or rows (prediction).
//   lin_*           the entry points' common bodies: creation, the three set functions, the learn guards, destroy, the scores getter,
//                   "score a model on a set" and "score rows with a model" (prediction).  They take the calling API's prefix ("rl_ada_"),
//                   so a state error names the functions the caller used.

namespace rl {

constexpr int kCaSteps = 64;          // trials per launch (a direction of more trials is evaluated in pieces of 64: same chain)
constexpr int kCaTiny = 16, kCaWave = 384, kCaBlock = 5000;

// A linear model: nt terms w[t] * term(x[col[t]]) on top of 0.0 or (BIAS) w[nw - 1].  Host or device pointers, as the function says.
struct LinModel {
    const int32_t *col = nullptr; int32_t nt = 0;      // null: column t (column-major sets only)
    const double *thr = nullptr;                       // null: the term is the value; else (double)value > thr[t] ? 1 : 0
    const double *w = nullptr; int32_t nw = 0;         // nw >= nt
    bool bias = false;                                 // the sum starts at w[nw - 1]
};

// column-major X (xc[col * n + i]) or rows (rows[i * stride + col]); col < 0 or (rows) col >= stride reads 0
template <bool STEP, bool BIAS>
__global__ void k_lin_score(double *out, const float *xc, const float *rows, int64_t stride, int64_t n, const int32_t *col, int32_t nt,
                            const double *thr, const double *w, int32_t nw)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = BIAS ? w[nw - 1] : 0.0;
    for (int t = 0; t < nt; t++) {
        const int32_t c = col ? col[t] : t;
        float v = 0.f;
        if (c >= 0) {
            if (xc) v = xc[(int64_t)c * n + i];
            else if (c < stride) v = rows[i * stride + c];
        }
        if (STEP) s += w[t] * (double)(((double)v > thr[t]) ? 1 : 0);       // a multiply by 0 too: RankBoost.eval adds every term
        else s += w[t] * (double)v;
    }
    out[i] = s;
}

struct CaClass {
    int32_t nq = 0; int32_t *d_qlist = nullptr;
    int64_t nh = 0; int64_t *d_hoff = nullptr;        // longest class only
};

struct CaSet : ListSetHost {           // the host side (labels, qoff, qkey, the -qrel tables): rl_lists_host.h
    std::vector<float> X;              // [N][F] as given
    float *d_xc = nullptr, *d_labels = nullptr; int32_t *d_qoff = nullptr, *d_rd = nullptr;
    double *d_ideal = nullptr, *d_cache = nullptr, *d_cache2 = nullptr;
    CaClass cls[4];
    double *d_hsc = nullptr; int32_t *d_hrel = nullptr; int32_t hchunks = 0;
};

struct LinCtx {
    int32_t metric = RL_METRIC_NDCG, metric_k = 10, device = 0;
    double err_max = 16.0;
    int32_t F = 0;
    bool has_train = false, has_valid = false, uploaded = false, learned = false;
    CaSet tr, va;
    hipStream_t stream = nullptr;
    DevPool buf;
    double *d_disc = nullptr, *d_m = nullptr, *d_sums = nullptr; uint32_t *d_done = nullptr;
    double *h_sums = nullptr;
    int32_t *d_col = nullptr; double *d_thr = nullptr, *d_w = nullptr; int32_t model_cap = -1;   // lin_score_model's copy of the model
    double train_score = 0, valid_score = 0;
    ~LinCtx()
    {
        if (h_sums) (void)hipHostFree(h_sums);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

template <class H> static LinCtx *lin_ctx(H *h) { return h ? &h->ctx : nullptr; }
template <class H> static const LinCtx *lin_ctx(const H *h) { return h ? &h->ctx : nullptr; }

// rl_ca.hip: trials [0, T) of one direction on set d through k_ca_trials
static int ca_trials(LinCtx *c, CaSet &d, const float *xcol, const double *steps, int T, int first, double *out);

static int ca_check_set(const float *X, int64_t n, int32_t F, const float *labels, const int32_t *qoff, int32_t Q)
{
    if (!X || !labels || !qoff) return fail(RL_ERR_INVALID, "null data pointer");
    if (n <= 0 || Q <= 0 || F <= 0) return fail(RL_ERR_INVALID, "There are no training samples / features");
    if (n >= (int64_t)2147483647 - 4096) return fail(RL_ERR_UNSUPPORTED, "more than 2^31 documents per GPU");
    std::string err;
    const int rc = check_lists("", labels, n, qoff, Q, err);
    if (rc) return fail(rc, err);
    for (int64_t i = 0; i < n * F; i++) {
        if (std::isnan(X[i])) return fail(RL_ERR_INVALID, "NaN in X (a missing feature must be passed as 0)");
        if (std::isinf(X[i])) return fail(RL_ERR_UNSUPPORTED, "+-Infinity feature value: the Java's cached scores turn NaN (0 * Infinity), not reproduced (DESIGN.md 7)");
    }
    return RL_OK;
}

static void ca_store(CaSet &d, const float *X, int64_t n, int32_t F, const float *labels, const int32_t *qoff, int32_t Q, const int32_t *qkey)
{
    d.store(labels, n, qoff, Q, qkey);
    d.X.assign(X, X + n * F);
}

static int ca_upload(LinCtx *c, CaSet &d, const std::vector<double> &ideal)
{
    const int64_t N = d.N; const int32_t F = c->F;
    std::vector<float> xc((size_t)N * F);
    for (int64_t i = 0; i < N; i++)
        for (int32_t f = 0; f < F; f++) xc[(size_t)f * N + i] = d.X[(size_t)i * F + f];
    std::vector<float>().swap(d.X);                  // the rows are not needed on the host any more
    RL_HIP(c->buf.alloc(&d.d_xc, xc.size()));
    RL_HIP(hipMemcpy(d.d_xc, xc.data(), xc.size() * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(c->buf.alloc(&d.d_labels, (size_t)N));
    RL_HIP(hipMemcpy(d.d_labels, d.labels.data(), N * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(c->buf.alloc(&d.d_qoff, (size_t)d.Q + 1));
    RL_HIP(hipMemcpy(d.d_qoff, d.qoff.data(), ((size_t)d.Q + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(c->buf.alloc(&d.d_ideal, (size_t)d.Q));
    RL_HIP(hipMemcpy(d.d_ideal, ideal.data(), d.Q * sizeof(double), hipMemcpyHostToDevice));
    if (!d.ext_rd.empty()) {
        RL_HIP(c->buf.alloc(&d.d_rd, (size_t)d.Q));
        RL_HIP(hipMemcpy(d.d_rd, d.ext_rd.data(), d.Q * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    RL_HIP(c->buf.alloc(&d.d_cache, (size_t)N));
    RL_HIP(c->buf.alloc(&d.d_cache2, (size_t)N));
    std::vector<int32_t> lists[4];
    std::vector<int64_t> hoff;
    int64_t nh = 0;
    for (int32_t q = 0; q < d.Q; q++) {
        const int n = d.qoff[q + 1] - d.qoff[q];
        const int k = n <= kCaTiny ? 0 : n <= kCaWave ? 1 : n <= kCaBlock ? 2 : 3;
        lists[k].push_back(q);
        if (k == 3) { hoff.push_back(nh); nh += n; }
    }
    for (int k = 0; k < 4; k++) {
        CaClass &cl = d.cls[k];
        cl.nq = (int32_t)lists[k].size();
        if (!cl.nq) continue;
        RL_HIP(c->buf.alloc(&cl.d_qlist, lists[k].size()));
        RL_HIP(hipMemcpy(cl.d_qlist, lists[k].data(), lists[k].size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (d.cls[3].nq) {
        CaClass &cl = d.cls[3];
        cl.nh = nh;
        RL_HIP(c->buf.alloc(&cl.d_hoff, hoff.size()));
        RL_HIP(hipMemcpy(cl.d_hoff, hoff.data(), hoff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        d.hchunks = std::max(1, std::min(kCaSteps, 1024 / cl.nq));     // chunks of the trials of one launch (sizes the scratch)
        RL_HIP(c->buf.alloc(&d.d_hsc, (size_t)d.hchunks * nh));
        RL_HIP(c->buf.alloc(&d.d_hrel, (size_t)d.hchunks * nh));
    }
    return RL_OK;
}

// the discounts, the ideal DCGs (the qid-keyed cache with the -qrel entries first: ideal_cache, rl_lists_host.h) and both sets on the device
static int ca_prepare(LinCtx *c)
{
    const std::vector<double> disc = discount_table(std::max(c->tr.maxq, c->has_valid ? c->va.maxq : 0));
    RL_HIP(c->buf.alloc(&c->d_disc, disc.size()));
    RL_HIP(hipMemcpy(c->d_disc, disc.data(), disc.size() * sizeof(double), hipMemcpyHostToDevice));
    const int k = c->metric_k;
    std::vector<double> ideal[2];
    ideal_cache(c->tr, c->has_valid ? &c->va : nullptr, disc, [k](int n) { return (k > n || k <= 0) ? n : k; }, ideal);
    int rc = ca_upload(c, c->tr, ideal[0]);
    if (rc) return rc;
    if (c->has_valid && (rc = ca_upload(c, c->va, ideal[1]))) return rc;
    RL_HIP(c->buf.alloc(&c->d_m, (size_t)std::max(c->tr.Q, c->has_valid ? c->va.Q : 0) * kCaSteps));
    RL_HIP(c->buf.alloc(&c->d_sums, (size_t)kCaSteps));
    RL_HIP(c->buf.alloc(&c->d_done, 1));
    RL_HIP(hipMemset(c->d_done, 0, sizeof(uint32_t)));
    RL_HIP(hipHostMalloc((void **)&c->h_sums, kCaSteps * sizeof(double), hipHostMallocDefault));
    c->uploaded = true;
    return RL_OK;
}

// out[i] = the model's score of document i; m holds device pointers
static int lin_launch_score(hipStream_t stream, double *out, const float *xc, const float *rows, int64_t stride, int64_t n, const LinModel &m)
{
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (m.thr) hipLaunchKernelGGL((k_lin_score<true, false>), grid, block, 0, stream, out, xc, rows, stride, n, m.col, m.nt, m.thr, m.w, m.nw);
    else if (m.bias) hipLaunchKernelGGL((k_lin_score<false, true>), grid, block, 0, stream, out, xc, rows, stride, n, m.col, m.nt, m.thr, m.w, m.nw);
    else hipLaunchKernelGGL((k_lin_score<false, false>), grid, block, 0, stream, out, xc, rows, stride, n, m.col, m.nt, m.thr, m.w, m.nw);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// scorer.score(rank(d)) of the model m (host pointers), the cache computed from scratch.  The context keeps the device copy of the model
// (it grows with the largest model seen and is freed with the handle): no temporary is freed while the stream still reads it.
static int lin_score_model(LinCtx *c, CaSet &d, const LinModel &m, double *score)
{
    if (m.nw > c->model_cap) {
        RL_HIP(c->buf.alloc(&c->d_col, (size_t)m.nw));
        RL_HIP(c->buf.alloc(&c->d_thr, (size_t)m.nw));
        RL_HIP(c->buf.alloc(&c->d_w, (size_t)m.nw));
        c->model_cap = m.nw;
    }
    LinModel dm = m;
    dm.col = m.col ? c->d_col : nullptr; dm.thr = m.thr ? c->d_thr : nullptr; dm.w = c->d_w;
    if (m.col && m.nt) RL_HIP(hipMemcpyAsync(c->d_col, m.col, m.nt * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (m.thr && m.nt) RL_HIP(hipMemcpyAsync(c->d_thr, m.thr, m.nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (m.nw) RL_HIP(hipMemcpyAsync(c->d_w, m.w, m.nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int rc = lin_launch_score(c->stream, d.d_cache, d.d_xc, nullptr, 0, d.N, dm);
    if (rc) return rc;
    return ca_trials(c, d, nullptr, nullptr, 1, 0, score);       // synchronises the stream: m's arrays are the caller's again
}

// the end of every learn(): the model's scores on both sets
static int lin_finish(LinCtx *c, const LinModel &m)
{
    int rc = lin_score_model(c, c->tr, m, &c->train_score);
    if (rc) return rc;
    c->valid_score = 0;
    if (c->has_valid && (rc = lin_score_model(c, c->va, m, &c->valid_score))) return rc;
    c->learned = true;
    return RL_OK;
}

// rl_*_predict after the entry point's own argument checks: out[i] = the model's score of row i of X (m: host pointers)
static int lin_predict(int32_t device, const LinModel &m, const float *X, int64_t n_docs, int32_t row_stride, double *out)
{
    const int gate = open_device(device, false);      // prediction has never tested the architecture
    if (gate || n_docs == 0) return gate;
    DevPool buf;
    float *dX = nullptr; int32_t *dF = nullptr; double *dT = nullptr, *dW = nullptr, *dO = nullptr;
    RL_HIP(buf.alloc(&dX, (size_t)n_docs * row_stride));
    RL_HIP(buf.alloc(&dF, (size_t)m.nt));
    RL_HIP(buf.alloc(&dT, (size_t)m.nt));
    RL_HIP(buf.alloc(&dW, (size_t)m.nw));
    RL_HIP(buf.alloc(&dO, (size_t)n_docs));
    RL_HIP(hipMemcpy(dX, X, (size_t)n_docs * row_stride * sizeof(float), hipMemcpyHostToDevice));
    if (m.nt) RL_HIP(hipMemcpy(dF, m.col, m.nt * sizeof(int32_t), hipMemcpyHostToDevice));
    if (m.nt && m.thr) RL_HIP(hipMemcpy(dT, m.thr, m.nt * sizeof(double), hipMemcpyHostToDevice));
    if (m.nw) RL_HIP(hipMemcpy(dW, m.w, m.nw * sizeof(double), hipMemcpyHostToDevice));
    LinModel dm = m;
    dm.col = dF; dm.thr = m.thr ? dT : nullptr; dm.w = dW;
    int rc = lin_launch_score(nullptr, dO, nullptr, dX, row_stride, n_docs, dm);
    if (rc) return rc;
    RL_HIP(hipMemcpy(out, dO, n_docs * sizeof(double), hipMemcpyDeviceToHost));
    return RL_OK;
}

// rl_*_create: the checks every ranker makes and the stream.  name: the ranker as its messages call it
static int lin_create(LinCtx *c, const char *name, int32_t metric, int32_t metric_k, int32_t device, double err_max)
{
    if (metric < RL_METRIC_NDCG || metric > RL_METRIC_RR)
        return fail(RL_ERR_UNSUPPORTED, std::string(name) + " train metric must be NDCG, DCG, MAP, ERR, P or RR (BEST is not built for training)");
    const int gate = open_device(device, true);
    if (gate) return gate;
    if (!(err_max > 0.0) || !std::isfinite(err_max)) return fail(RL_ERR_INVALID, "err_max (ERRScorer.MAX) must be positive and finite");
    c->metric = metric; c->metric_k = metric_k; c->device = device; c->err_max = err_max;
    RL_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    return RL_OK;
}

template <class H> static void lin_destroy(H *h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx.device);
    if (h->ctx.stream) (void)hipStreamSynchronize(h->ctx.stream);
    delete h;
}

// api: the caller's prefix ("rl_ada_"), for the state errors
static int lin_set_train(LinCtx *c, const char *api, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                         int32_t n_queries, const int32_t *qkey)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (c->uploaded) return fail(RL_ERR_STATE, std::string(api) + "set_train after " + api + "learn");
    int rc = ca_check_set(X, n_docs, n_features, labels, qoff, n_queries);
    if (rc) return rc;
    c->F = n_features;
    ca_store(c->tr, X, n_docs, n_features, labels, qoff, n_queries, qkey);
    c->has_train = true;
    return RL_OK;
}

static int lin_set_validation(LinCtx *c, const char *api, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff,
                              int32_t n_queries, const int32_t *qkey)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (!c->has_train) return fail(RL_ERR_STATE, "set the training data first");
    if (c->uploaded) return fail(RL_ERR_STATE, std::string(api) + "set_validation after " + api + "learn");
    int rc = ca_check_set(X, n_docs, c->F, labels, qoff, n_queries);
    if (rc) return rc;
    ca_store(c->va, X, n_docs, c->F, labels, qoff, n_queries, qkey);
    c->has_valid = true;
    return RL_OK;
}

static int lin_set_external_judgments(LinCtx *c, const char *api, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (c->uploaded) return fail(RL_ERR_STATE, std::string(api) + "set_external_judgments after " + api + "learn");
    if (validation ? !c->has_valid : !c->has_train) return fail(RL_ERR_STATE, "set the data first");
    std::string err;
    const int rc = (validation ? c->va : c->tr).set_external(ideal_dcg, rel_doc_count, err);
    return rc ? fail(rc, err) : RL_OK;
}

// the guards of rl_*_learn; leaves the handle's device current
static int lin_begin_learn(LinCtx *c, const char *api)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (!c->has_train) return fail(RL_ERR_STATE, "set the training data first");
    if (c->uploaded) return fail(RL_ERR_STATE, std::string(api) + "learn runs once per handle");
    RL_HIP(hipSetDevice(c->device));
    return RL_OK;
}

static int lin_scores(const LinCtx *c, const char *api, double *train, double *valid)
{
    if (!c) return fail(RL_ERR_INVALID, "null handle");
    if (!c->learned) return fail(RL_ERR_STATE, std::string(api) + "learn has not run");
    if (train) *train = c->train_score;
    if (valid) *valid = c->valid_score;
    return RL_OK;
}

template <class Rec> static int lin_trace(const std::vector<Rec> *trace, Rec *out, int64_t cap, int64_t *n)
{
    if (!trace || !n) return fail(RL_ERR_INVALID, "null argument");
    *n = (int64_t)trace->size();
    if (out) std::copy(trace->begin(), trace->begin() + std::max<int64_t>(0, std::min<int64_t>(cap, *n)), out);
    return RL_OK;
}

}  // namespace rl
