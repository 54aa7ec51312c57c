// rl_ada.inc -- AdaRank (-ranker 3, learning/boosting/AdaRank.java) on gfx950; included at the end of rl_ca.hip.  The handle holds a
// ranking context (LinCtx, rl_linear.inc: the device sets, the stream, the common entry-point bodies) and uses rl_ca.hip's scorer
// (ca_metric) and trial kernel (k_ca_trials).
//
// Every number an AdaRank round needs is a list metric:
//   * the weak rankers' table M[q][f] = scorer.score(WeakRanker(f).rank(list q)): constant over the run (the list ranked by feature f
//     alone, WeakRanker.java:34-41), built once per learn() by k_ada_weak;
//   * the candidates' sums s_f = sum_q M[q][f] * sweight[q] and the alpha sums num_f / denom_f (AdaRank.java:74-95, :128-134), serial in
//     list order, one lane per feature: k_ada_select;
//   * the ensemble after a new term alpha * x_f: one trial of a Coordinate Ascent direction (k_ca_trials with T = 1), which leaves the
//     per-list metrics m_q behind and the new cache in the set's second buffer: undoing the term (ROLLBACK :108-118, the stop :189-193)
//     is a swap back, always one level.
//
//   k_ada_weak<G, CAP>   a group of G threads owns one (feature, list) pair and replays utilities/Sorter.sort(double[], false) on it: at
//                        step i the FIRST position >= i that holds the maximum (strict <) is swapped into slot i.  Not stable, so it is
//                        replayed step by step: a group argmax per step, (value, position) pairs swapped in LDS (or global scratch for
//                        lists beyond kCaBlock).  Cut-off metrics need the first min(k, n) steps, MAP all n - 1.  Length classes as
//                        k_ca_trials': <= 16 documents (16 lanes), <= 384 (one wavefront), <= 5000 (one block, LDS), longer (one block,
//                        global scratch, features in chunks).
//   k_ada_select         lane f: the three list-order f64 chains of feature f; M is [Q][F] so a row load is contiguous across lanes.
// The final model is scored from scratch by k_lin_score: 0.0 + w[0] x[c0] + w[1] x[c1] + ... (AdaRank.eval :265-271, repeated columns).
//
// log / exp are the host C library's (SimpleMath.ln = log(x) / log(e), Math.exp), the functions Python's math module calls too.

namespace rl {

__device__ __forceinline__ void ada_better(float &bv, int &bj, float ov, int oj)
{   // (value, position): the larger value, the lower position among equal values; bj < 0 = no candidate
    if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
}

template <int G, int CAP>
__global__ __launch_bounds__(kThreads) void k_ada_weak(const CaArgs a, const float *xc, int64_t N, double *M, int32_t F, int32_t f0,
                                                       int32_t nf, float *hv, int32_t *hr)
{
    constexpr int GPB = kThreads / G;
    constexpr int LDS = CAP > 0 ? CAP : 1;
    constexpr int NW = G > kWave ? G / kWave : 1;
    __shared__ float s_v[GPB][LDS];
    __shared__ int s_r[GPB][LDS];
    __shared__ float s_bv[NW];
    __shared__ int s_bj[NW];
    const int grp = threadIdx.x / G, tid = threadIdx.x % G;
    const int64_t g = (int64_t)blockIdx.x * GPB + grp;
    if (g >= (int64_t)a.nq * nf) return;                  // whole groups only (G == kThreads: the whole block)
    const int slot = (int)(g % a.nq), fl = (int)(g / a.nq), f = f0 + fl;
    const int q = a.qlist[slot];
    const int cur = a.qoff[q], n = a.qoff[q + 1] - cur;
    float *v = s_v[grp];
    int *r = s_r[grp];
    if (CAP == 0) { v = hv + (size_t)fl * a.nh + a.hoff[slot]; r = hr + (size_t)fl * a.nh + a.hoff[slot]; }
    const float *x = xc + (size_t)f * N + cur;
    for (int i = tid; i < n; i += G) { v[i] = x[i]; r[i] = ca_rel(a, a.labels[cur + i]); }
    ca_sync<G>();
    const int size = (a.k > n || a.k <= 0) ? n : a.k;
    const int steps = min(a.metric == RL_METRIC_MAP ? n : size, n - 1);
    for (int i = 0; i < steps; i++) {
        float bv = 0.f; int bj = -1;
        for (int j = i + tid; j < n; j += G) { const float y = v[j]; if (bj < 0 || y > bv) { bv = y; bj = j; } }
#pragma unroll
        for (int off = 1; off < (G < kWave ? G : kWave); off <<= 1) {
            const float ov = __shfl_xor(bv, off, G < kWave ? G : kWave);
            const int oj = __shfl_xor(bj, off, G < kWave ? G : kWave);
            ada_better(bv, bj, ov, oj);
        }
        if (G > kWave) {
            if ((tid % kWave) == 0) { s_bv[tid / kWave] = bv; s_bj[tid / kWave] = bj; }
            __syncthreads();
            bv = s_bv[0]; bj = s_bj[0];
            for (int w = 1; w < NW; w++) ada_better(bv, bj, s_bv[w], s_bj[w]);
        }
        if (tid == 0 && bj != i) {                          // Sorter.java: swap freqIdx[i] and freqIdx[max]
            const float tv = v[i]; v[i] = v[bj]; v[bj] = tv;
            const int tr = r[i]; r[i] = r[bj]; r[bj] = tr;
        }
        ca_sync<G>();
    }
    if (tid == 0) M[(size_t)q * F + f] = ca_metric(a, q, n, r);
}

__global__ void k_ada_select(const double *M, const double *sw, int32_t Q, int32_t F, double *out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double s = 0.0, num = 0.0, denom = 0.0;
#pragma unroll 8
    for (int q = 0; q < Q; q++) {
        const double m = M[(size_t)q * F + f], w = sw[q];
        s += m * w;                                         // learnWeakRanker :85-86
        num += w * (1.0 + m);                               // :132-133
        denom += w * (1.0 - m);
    }
    out[f] = s;
    out[F + f] = num;
    out[2 * F + f] = denom;
}

}  // namespace rl

struct rl_ada {
    rl_ada_params p;
    LinCtx ctx;
    double *d_M = nullptr, *d_sw = nullptr, *d_sel = nullptr;
    std::vector<int32_t> fid; std::vector<double> weight;
    std::vector<rl_ada_trace_rec> trace;
};

namespace rl {

// M[q][f] for every list of set d (the training set): one launch per length class (the longest class in feature chunks of its scratch)
static int ada_weak_table(rl_ada *A)
{
    LinCtx *c = &A->ctx;
    CaSet &d = c->tr;
    const int F = c->F;
    RL_HIP(c->buf.alloc(&A->d_M, (size_t)d.Q * F));
    CaArgs a;
    memset(&a, 0, sizeof(a));
    a.labels = d.d_labels; a.qoff = d.d_qoff; a.ideal = d.d_ideal; a.rd_ext = d.d_rd; a.disc = c->d_disc;
    a.Q = d.Q; a.metric = c->metric; a.k = c->metric_k; a.err_max = c->err_max;
    float *hv = nullptr; int32_t *hr = nullptr; int fchunk = F;
    if (d.cls[3].nq) {
        fchunk = (int)std::max<int64_t>(1, std::min<int64_t>(F, ((int64_t)64 << 20) / std::max<int64_t>(1, d.cls[3].nh)));   // <= 512 MiB
        RL_HIP(c->buf.alloc(&hv, (size_t)fchunk * d.cls[3].nh));
        RL_HIP(c->buf.alloc(&hr, (size_t)fchunk * d.cls[3].nh));
    }
    static const int G[4] = {kCaTiny, kWave, kThreads, kThreads};
    for (int k = 0; k < 4; k++) {
        const CaClass &cl = d.cls[k];
        if (!cl.nq) continue;
        a.qlist = cl.d_qlist; a.nq = cl.nq; a.hoff = cl.d_hoff; a.nh = cl.nh;
        const int nf0 = k == 3 ? fchunk : F;
        for (int f0 = 0; f0 < F; f0 += nf0) {
            const int nf = std::min(nf0, F - f0);
            const int gpb = kThreads / G[k];
            const unsigned grid = (unsigned)(((int64_t)cl.nq * nf + gpb - 1) / gpb);
            if (k == 0) hipLaunchKernelGGL((k_ada_weak<kCaTiny, kCaTiny>), dim3(grid), dim3(kThreads), 0, c->stream, a, d.d_xc, d.N, A->d_M, F, f0, nf, hv, hr);
            else if (k == 1) hipLaunchKernelGGL((k_ada_weak<kWave, kCaWave>), dim3(grid), dim3(kThreads), 0, c->stream, a, d.d_xc, d.N, A->d_M, F, f0, nf, hv, hr);
            else if (k == 2) hipLaunchKernelGGL((k_ada_weak<kThreads, kCaBlock>), dim3(grid), dim3(kThreads), 0, c->stream, a, d.d_xc, d.N, A->d_M, F, f0, nf, hv, hr);
            else hipLaunchKernelGGL((k_ada_weak<kThreads, 0>), dim3(grid), dim3(kThreads), 0, c->stream, a, d.d_xc, d.N, A->d_M, F, f0, nf, hv, hr);
            RL_HIP(hipGetLastError());
        }
    }
    RL_HIP(hipStreamSynchronize(c->stream));
    return RL_OK;
}

// s_f, num_f, denom_f of every feature under the sample weights sw (3 F doubles)
static int ada_select(rl_ada *A, const std::vector<double> &sw, std::vector<double> &sel)
{
    LinCtx *c = &A->ctx;
    const int F = c->F;
    RL_HIP(hipMemcpyAsync(A->d_sw, sw.data(), sw.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_ada_select, dim3((unsigned)((F + kWave - 1) / kWave)), dim3(kWave), 0, c->stream, (const double *)A->d_M,
                       (const double *)A->d_sw, c->tr.Q, F, A->d_sel);
    RL_HIP(hipGetLastError());
    sel.resize((size_t)3 * F);
    RL_HIP(hipMemcpyAsync(sel.data(), A->d_sel, sel.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RL_HIP(hipStreamSynchronize(c->stream));
    return RL_OK;
}

// the ensemble + alpha * x_f on set d: its per-list metrics into m (when given) and scorer.score(rank(d)) into *score
static int ada_step(rl_ada *A, CaSet &d, int f, double alpha, std::vector<double> *m, double *score)
{
    LinCtx *c = &A->ctx;
    int rc = ca_trials(c, d, d.d_xc + (size_t)f * d.N, &alpha, 1, 1, score);
    if (rc) return rc;
    if (m) {
        m->resize(d.Q);
        RL_HIP(hipMemcpy(m->data(), c->d_m, (size_t)d.Q * sizeof(double), hipMemcpyDeviceToHost));
    }
    return RL_OK;
}

// the most recent term off the ensemble: the caches before it are still in the second buffers
static void ada_undo(rl_ada *A)
{
    LinCtx *c = &A->ctx;
    std::swap(c->tr.d_cache, c->tr.d_cache2);
    if (c->has_valid) std::swap(c->va.d_cache, c->va.d_cache2);
}

static double ada_ln(double v)
{   // utilities/SimpleMath.java ln: log(v) / log(Math.E), both at run time (no compile-time folding of log(e))
    volatile double e = 2.718281828459045;
    return std::log(v) / std::log((double)e);
}

struct AdaState {                      // the Java object's fields (AdaRank.java:42-57)
    std::vector<char> used;            // usedFeatures
    std::vector<double> sweight, backup;
    std::vector<int32_t> rankers, bestRankers; std::vector<double> rweight, bestWeights;
    std::vector<int32_t> queue;        // featureQueue
    int lastFeature = -1, lastCount = 0;
    double backupTrainScore = 0.0, lastTrainedScore = -1.0, bestValid = 0.0;
};

// AdaRank.learn(startIteration, withEnqueue) :97-202
static int ada_learn_phase(rl_ada *A, AdaState &S, int start, bool withEnqueue, int *t_out)
{
    LinCtx *c = &A->ctx;
    const rl_ada_params &P = A->p;
    const int F = c->F, Q = c->tr.Q;
    std::vector<double> sel, m;
    int t = start;
    for (; t <= P.n_iteration; t++) {
        int rc = ada_select(A, S.sweight, sel);
        if (rc) return rc;
        int best = -1; double bestScore = -1.0;              // learnWeakRanker :74-95
        for (int f = 0; f < F; f++) {
            if (S.used[f] || std::find(S.queue.begin(), S.queue.end(), f) != S.queue.end()) continue;
            if (bestScore < sel[f]) { bestScore = sel[f]; best = f; }
        }
        if (best < 0) break;
        rl_ada_trace_rec rec; memset(&rec, 0, sizeof(rec));
        rec.iteration = t; rec.feature = best;
        if (withEnqueue) {
            if (best == S.lastFeature) {                     // :108-119
                S.queue.push_back(S.lastFeature);
                S.rankers.pop_back(); S.rweight.pop_back();
                ada_undo(A);
                S.sweight = S.backup;
                S.bestValid = 0.0;
                S.lastTrainedScore = S.backupTrainScore;
                rec.kind = RL_ADA_ROLLBACK;
                A->trace.push_back(rec);
                continue;
            }
            S.lastFeature = best;
            S.backup = S.sweight;
            S.backupTrainScore = S.lastTrainedScore;
        }
        const double num = sel[(size_t)F + best], denom = sel[(size_t)2 * F + best];
        const double alpha = 0.5 * ada_ln(num / denom);
        if (!std::isfinite(alpha)) {
            char msg[320];
            snprintf(msg, sizeof(msg), "AdaRank round %d: feature index %d gives alpha = 0.5 ln(num / denom) = %.17g with num = %.17g, "
                     "denom = %.17g; the Java goes on with a non-finite weight, not reproduced (DESIGN.md 9)", t, best, alpha, num, denom);
            return fail(RL_ERR_UNSUPPORTED, msg);
        }
        S.rankers.push_back(best); S.rweight.push_back(alpha);
        double ignored;
        rc = ada_step(A, c->tr, best, alpha, &m, &ignored);
        if (rc) return rc;
        double trainedScore = 0.0, total = 0.0;              // :140-148
        std::vector<double> e((size_t)Q);
        for (int q = 0; q < Q; q++) {
            e[q] = std::exp(-alpha * m[q]);
            total += e[q];
            trainedScore += m[q];
        }
        trainedScore /= Q;
        const double delta = trainedScore + P.tolerance - S.lastTrainedScore;
        int status = delta > 0 ? RL_ADA_OK : RL_ADA_DAMN;
        if (!withEnqueue) {                                   // :152-174
            if (trainedScore != S.lastTrainedScore) {
                S.lastCount = 0;
                std::fill(S.used.begin(), S.used.end(), 0);
            } else if (S.lastFeature == best) {
                S.lastCount++;
                if (S.lastCount == P.max_sel_count) {
                    status = RL_ADA_FREM;
                    S.lastCount = 0;
                    S.used[S.lastFeature] = 1;
                }
            } else {
                S.lastCount = 0;
                std::fill(S.used.begin(), S.used.end(), 0);
            }
            S.lastFeature = best;
        }
        double vs = 0.0;
        if (c->has_valid) {                                   // :177-183
            rc = ada_step(A, c->va, best, alpha, nullptr, &vs);
            if (rc) return rc;
            if (vs > S.bestValid) { S.bestValid = vs; S.bestRankers = S.rankers; S.bestWeights = S.rweight; }
        }
        rec.kind = RL_ADA_ROUND; rec.status = status; rec.alpha = alpha; rec.train_score = trainedScore; rec.valid_score = vs;
        A->trace.push_back(rec);
        if (delta <= 0) {                                     // :189-194
            S.rankers.pop_back(); S.rweight.pop_back();
            ada_undo(A);
            break;
        }
        S.lastTrainedScore = trainedScore;
        for (int q = 0; q < Q; q++) S.sweight[q] = S.sweight[q] * (e[q] / total);    // :197-199, Math.exp computed once per list
    }
    *t_out = t;
    return RL_OK;
}

static int ada_learn(rl_ada *A)
{
    LinCtx *c = &A->ctx;
    const int F = c->F, Q = c->tr.Q;
    A->trace.clear();
    int rc = ada_weak_table(A);
    if (rc) return rc;
    RL_HIP(c->buf.alloc(&A->d_sw, (size_t)Q));
    RL_HIP(c->buf.alloc(&A->d_sel, (size_t)3 * F));
    RL_HIP(hipMemsetAsync(c->tr.d_cache, 0, c->tr.N * sizeof(double), c->stream));       // the empty ensemble scores 0.0
    if (c->has_valid) RL_HIP(hipMemsetAsync(c->va.d_cache, 0, c->va.N * sizeof(double), c->stream));
    AdaState S;                                               // init() :205-227
    S.used.assign((size_t)F, 0);
    S.sweight.assign((size_t)Q, (double)(1.0f / (float)Q));
    S.backup = S.sweight;
    auto phase = [&](int t, int f, bool enq) {
        rl_ada_trace_rec rec; memset(&rec, 0, sizeof(rec));
        rec.iteration = t; rec.kind = RL_ADA_PHASE; rec.feature = f; rec.status = enq ? 1 : 0;
        A->trace.push_back(rec);
    };
    int t = 1;
    if (A->p.train_with_enqueue) {                            // :234-243
        phase(1, -1, true);
        if ((rc = ada_learn_phase(A, S, 1, true, &t))) return rc;
        for (int i = (int)S.queue.size() - 1; i >= 0; i--) {
            const int f = S.queue[i];
            S.queue.erase(S.queue.begin() + i);
            phase(t, f, false);
            if ((rc = ada_learn_phase(A, S, t, false, &t))) return rc;
        }
    } else {
        phase(1, -1, false);
        if ((rc = ada_learn_phase(A, S, 1, false, &t))) return rc;
    }
    if (c->has_valid && !S.bestRankers.empty()) { S.rankers = S.bestRankers; S.rweight = S.bestWeights; }    // :247-252
    A->fid = S.rankers; A->weight = S.rweight;
    LinModel m;
    m.col = A->fid.data(); m.w = A->weight.data(); m.nt = m.nw = (int32_t)A->fid.size();
    return lin_finish(c, m);
}

}  // namespace rl

extern "C" {

void rl_ada_params_default(rl_ada_params *p)
{   // learning/boosting/AdaRank.java:37-40
    if (!p) return;
    p->n_iteration = 500; p->tolerance = 0.002; p->train_with_enqueue = 1; p->max_sel_count = 5;
    p->metric = RL_METRIC_NDCG; p->metric_k = 10; p->device = 0; p->err_max = 16.0;
}

int rl_ada_create(const rl_ada_params *p, rl_ada **out)
{
    if (!p || !out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<rl_ada> A(new rl_ada());
    A->p = *p;
    int rc = lin_create(&A->ctx, "AdaRank", p->metric, p->metric_k, p->device, p->err_max);
    if (rc) return rc;
    *out = A.release();
    return RL_OK;
}

void rl_ada_destroy(rl_ada *a) { lin_destroy(a); }

int rl_ada_set_train(rl_ada *a, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                     int32_t n_queries, const int32_t *qkey)
{
    return lin_set_train(lin_ctx(a), "rl_ada_", X, n_docs, n_features, labels, qoff, n_queries, qkey);
}

int rl_ada_set_validation(rl_ada *a, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                          const int32_t *qkey)
{
    return lin_set_validation(lin_ctx(a), "rl_ada_", X, n_docs, labels, qoff, n_queries, qkey);
}

int rl_ada_set_external_judgments(rl_ada *a, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count)
{
    return lin_set_external_judgments(lin_ctx(a), "rl_ada_", validation, ideal_dcg, rel_doc_count);
}

int rl_ada_learn(rl_ada *a)
{
    int rc = lin_begin_learn(lin_ctx(a), "rl_ada_");
    if (rc) return rc;
    if (a->p.max_sel_count < 0) return fail(RL_ERR_INVALID, "max_sel_count must be >= 0");
    if ((rc = ca_prepare(&a->ctx))) return rc;
    return ada_learn(a);
}

int rl_ada_get_model(const rl_ada *a, int32_t *fid, double *weight, int32_t cap, int32_t *n)
{
    if (!a || !n) return fail(RL_ERR_INVALID, "null argument");
    if (!a->ctx.learned) return fail(RL_ERR_STATE, "rl_ada_learn has not run");
    *n = (int32_t)a->fid.size();
    const size_t m = std::min<size_t>(a->fid.size(), (size_t)std::max(0, cap));
    if (fid) std::copy(a->fid.begin(), a->fid.begin() + m, fid);
    if (weight) std::copy(a->weight.begin(), a->weight.begin() + m, weight);
    return RL_OK;
}

int rl_ada_scores(const rl_ada *a, double *train, double *valid) { return lin_scores(lin_ctx(a), "rl_ada_", train, valid); }

int rl_ada_trace(const rl_ada *a, rl_ada_trace_rec *out, int64_t cap, int64_t *n) { return lin_trace(a ? &a->trace : nullptr, out, cap, n); }

int rl_ada_debug_weak_table(const rl_ada *a, double *out, int64_t cap)
{
    if (!a || !out) return fail(RL_ERR_INVALID, "null argument");
    if (!a->d_M) return fail(RL_ERR_STATE, "rl_ada_learn has not built the weak-ranker table");
    const int64_t F = a->ctx.F, Q = a->ctx.tr.Q;
    if (cap < F * Q) return fail(RL_ERR_INVALID, "weak-table buffer too small");
    RL_HIP(hipSetDevice(a->ctx.device));
    std::vector<double> m((size_t)(F * Q));
    RL_HIP(hipMemcpy(m.data(), a->d_M, m.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < Q; q++)
        for (int64_t f = 0; f < F; f++) out[f * Q + q] = m[(size_t)(q * F + f)];
    return RL_OK;
}

}  // extern "C"
