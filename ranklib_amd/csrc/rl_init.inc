// rl_init.inc -- the stages of rl_init, in the order rl_init (rl_trainer.hip) calls them.  Included by rl_trainer.hip right in front of rl_init,
// behind the host helpers the stages use (DevPool, upload_query_side, alloc_chain, launch_rank).
//
// A stage leaves its results in the trainer's Ctx; InitWork carries what only rl_init's later stages need.  Sharded runs: every rank walks the
// same stages and meets its peers in the same collectives in the same order -- a stage never returns between two collectives for a reason only
// this rank can have (init_threshold_tables, host_table_of_column).

namespace rl {

struct InitWork {
    float *Xt = nullptr;                  // the training rows, column-major [F][Npad] (released behind the last stage that reads them)
    FeatStats fs; int slices = 1;         // per-column min / max / distinct values (k_feat_stats), and the grid of the passes over Xt
    float *thr0 = nullptr;                // threshold tables of the device, [columns][fs.limit + 1]
    std::vector<std::vector<float>> big; bool any_big = false;      // per column: its host-built table of more than 4 095 entries, or empty
    std::vector<int32_t> h_nthr; int32_t *d_nthr = nullptr; float *d_thr = nullptr;      // entries per table; the tables [F][TS]
    int F = 0, TS = 0;                    // columns of the row matrix until init_hist_features, histogram (virtual) features and their table stride after
    uint16_t *d_bins = nullptr, *d_gbins = nullptr; int32_t *d_mode = nullptr;      // bins by feature and by 16-feature group; every feature's mode bin
    std::vector<int32_t> h_cum_cnt, h_mode;      // host copies of the root's cumulative counts [F][TS] and the mode bins (fetch_root_counts)
};

// chunks a child node is cut into: every chunk flushes a partial histogram of F x T x 12 bytes that the finish reads back, so wide data wants fewer
// (measured, rounds/s: c3, 700 columns: 3 / 4 / 6 / 8 / 12 / 16 / 24 -> 542 / 548 / 548 / 549-556 / 534 / 537 / 513; c2, 136 columns: flat from 8 to 32)
// (round 5, k_fin2: 16 partials per thread in one batch -- c2 sustained 345 -> 351 from 12 to 24 chunks; wide data keeps few)
static int default_node_div(int F) { return std::max(4, std::min(24, (int)(24.0 * 136.0 / (double)std::max(F, 1) + 0.5))); }

// the root's cumulative counts and the mode bins on the host, downloaded once (nothing writes them after init_bins)
static int fetch_root_counts(rl_trainer *t, InitWork &w)
{
    if (!w.h_cum_cnt.empty()) return RL_OK;
    w.h_cum_cnt.resize((size_t)w.F * w.TS); w.h_mode.resize((size_t)w.F);
    RL_HIP(hipStreamSynchronize(t->stream));
    RL_HIP(hipMemcpy(w.h_cum_cnt.data(), t->ctx.cum_cnt, w.h_cum_cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(w.h_mode.data(), w.d_mode, w.h_mode.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RL_OK;
}

// cells of feature f outside its mode bin, of n_docs documents (the counts' own total: all ranks' documents when they are all-reduced)
static int64_t cells_outside_mode(const InitWork &w, int f, int64_t n_docs)
{
    const int32_t *cc = w.h_cum_cnt.data() + (size_t)f * w.TS;
    const int m = w.h_mode[f];
    return n_docs - ((int64_t)cc[m] - (m > 0 ? cc[m - 1] : 0));
}

// ---- leaf budget, Ctx sizes, tuning defaults with their knob overrides -----------------------------------
static int init_shape(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx; hipStream_t s = t->stream; const Knobs &kn = t->knobs;
    const int N = (int)t->tr.N, Npad = (N + 127) / 128 * 128, F = w.F = t->F;
    // -leaf -1 (RegressionTree.java:72 `nodes == -1`): growth ends when no leaf can be split any more.  Every leaf holds at least
    // min_leaf_support documents, so a tree has at most floor(N / mls) leaves -- and with exactly that many none is left with 2 * mls
    // documents: a budget of floor(N / mls) leaves never binds before the Java's own loop ends.
    int L_eff = t->p.n_leaves;
    if (L_eff == -1) {
        long long Nall = N;          // sharded: the budget comes from the GLOBAL document count (every rank grows the same tree)
        if (t->dist) {
            long long *d_n = nullptr;
            RL_HIP(t->pool.alloc(&d_n, (size_t)1));
            RL_HIP(hipMemcpy(d_n, &Nall, sizeof(Nall), hipMemcpyHostToDevice));
            int rcd = t->dist->allreduce(d_n, 1, DT_I64, OP_SUM, s); if (rcd) return rcd;
            RL_HIP(hipStreamSynchronize(s));
            RL_HIP(hipMemcpy(&Nall, d_n, sizeof(Nall), hipMemcpyDeviceToHost));
            t->pool.release(d_n);
        }
        L_eff = (int)std::max<long long>(1, std::min<long long>(Nall / std::max(1, t->p.min_leaf_support), 1 << 28));
    }
    t->L_eff = L_eff;
    c.N = N; c.Npad = Npad; c.Q = t->tr.Q; c.F = F; c.L = L_eff;
    // the root is split unconditionally before the leaf budget is looked at (RegressionTree.java:62-67): even -leaf 1 gives 3 nodes
    c.MAXN = std::max(2 * L_eff - 1, 3);
    c.NC = 4 * L_eff + 2;     // node records: committed (2L-1) + prepared but never reached (see select_step)
    c.mls = t->p.min_leaf_support; c.lr = t->p.learning_rate;
    c.node_div = kn.node_div.or_else(default_node_div(F));
    c.node_min = kn.node_min;      // smallest chunk of a child node.  Every round-5 number was measured at 256 (ADVICE r05: the assignment of kMinChunk had been swallowed by a comment; 256 is what ran)
    c.fs_size = F; c.fs_on = 0; c.seed = t->p.seed;
    if (t->p.feature_sampling_rate > 0.0f && t->p.feature_sampling_rate < 1.0f) { c.fs_size = (int32_t)(t->p.feature_sampling_rate * (float)F); c.fs_on = c.fs_size < F ? 1 : 0; }   // :274
    c.hist_nt = kn.hist_nt.or_else(kThreads); c.sub_child = kn.sub_child;
    // largest chunk: smaller ones spread a mid-sized node over more blocks (measured, same box: c1, 1.2 M x 136: 4096 -> +0.9 % / +1.6 % sustained; c2, 3.77 M: -0.7 %;
    // c3, 700 columns: -1.8 %: every chunk more is another partial histogram of F x T x 12 bytes)
    c.node_chunk = (N <= (2 << 20) && F <= 256) ? 4096 : kNodeChunk;
    // balanced chunks for the steps that fill the chip (balance_slots): rows of the child-pass grid = chunks per round of blocks, largest chunk, steps of at most balance_min chunks keep chunk_docs' rule
    // Rows: about two blocks per CU -- 512 / (feature-group blocks per chunk), to the nearest multiple of 8 (k_hist's XCD map), at least 16.
    // Measured, same box, rounds/s: c2 / c1 (9 groups, 56 rows) 362.6 -> 372.7, 316.5 -> 326.0 over 300 rounds, c2ns 346.5 -> 363.9, c1 632 -> 646 (80 rows: +1 %, 64 / 72: worse
    // than none, 48: +0.5 %); c3 (44 groups) 486 -> 522 with 16 rows (8 rows: 477, 24 rows: 494).
    {
        const int gxb = (F + kHistFG - 1) / kHistFG;
        c.balance = kn.balance; c.balance_cap = std::min(kChunk, kn.balance_cap.or_else(kChunk));
        const int target = std::max(16, ((512 / std::max(gxb, 1) + 4) / 8) * 8);
        c.balance_target = kn.balance_target.or_else(target);
        c.balance_min = kn.balance_min.or_else(target / 2);
    }
    c.skip_last = kn.skip_last;
    c.metric = t->p.metric; c.mart = (t->p.ranker == RL_RANKER_MART) ? 1 : 0;
    // lazy Java-order tie-break (rl_tie.inc): the default path's exact ties resolved as the Java's summation order resolves them.  Not with
    // feature sampling (the Java's draw is unseeded: nothing to match), not sharded (the Java's order is ONE sequence over all documents), not in
    // the strict mode (every candidate already comes from the Java-order histogram)
    c.tie_on = (c.fs_size == F && !(t->p.flags & (RL_FLAG_JAVA_ORDER | RL_FLAG_FIRST_TIE)) && !kn.tie_off) ? 1 : 0;      // (sharded runs: decided below, once TS is known)
    // rows of a ranked list whose pairs the lambda loop visits (LambdaMART.java:375-377: j <= cutoff or k <= cutoff); for
    // NDCG / DCG / ERR / P / RR row `cutoff` itself only holds zero swap changes (P, RR: every non-zero entry has min(i, j) < size <= k)
    c.k = (t->p.metric == RL_METRIC_MAP) ? t->p.metric_k + 1 : t->p.metric_k;
    c.rank = t->rank; c.n_ranks = t->n_ranks; c.sharded = t->dist ? 1 : 0;
    if (c.sharded) c.skip_last = 0;       // (the last split's lambda^2 sums travel with its histogram's all-reduce)
    return RL_OK;
}

// the table of column f on the host (sort + unique of the column; sharded: of the distinct values of every rank): what LambdaMART.java:108-150 builds
static int host_table_of_column(rl_trainer *t, const InitWork &w, int f, int nT, std::vector<float> &colv, std::vector<float> &tab)
{
    hipStream_t s = t->stream;
    const int N = t->ctx.N, Npad = t->ctx.Npad;
    RL_HIP(hipMemcpy(colv.data(), w.Xt + (size_t)f * Npad, (size_t)N * sizeof(float), hipMemcpyDeviceToHost));
    float fmax = -std::numeric_limits<float>::infinity(), fmin = 3.4028234663852886e38f;       // :114-115
    for (auto &v : colv) { if (v == 0.f) v = 0.f; if (fmax < v) fmax = v; if (fmin > v) fmin = v; }      // (-0.0 folded as on the device)
    std::vector<float> vals(colv);
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    if (t->dist) {
        // sharded: the table is built from the distinct values of the column over ALL ranks (LambdaMART.java:108-150 walks one sorted list of every
        // sample).  Every rank contributes its own sorted distinct values -- counts first, then the values padded to the largest count -- and merges
        // what it receives; the overflow flags were all-reduced above, so the ranks take this branch for the same columns in the same order.
        const int R = t->n_ranks;
        // (ADVICE r05: temporaries are released on every path -- DevTmp -- and nothing returns between the two collectives of a column for a LOCAL
        // reason: a copy that fails is reported after the second all-gather, so the peers are not left waiting in it)
        struct DevTmp { void *p = nullptr; ~DevTmp() { if (p) (void)hipFree(p); } hipError_t get(size_t bytes) { return hipMalloc(&p, bytes); } };
        DevTmp t_cnt, t_cnts, t_v, t_all;
        hipError_t herr = t_cnt.get(sizeof(int32_t));
        if (herr == hipSuccess) herr = t_cnts.get((size_t)R * sizeof(int32_t));
        if (herr != hipSuccess) return fail(RL_ERR_HIP, std::string("hipMalloc (threshold-table merge): ") + hipGetErrorString(herr));
        const int32_t mycnt = (int32_t)vals.size();
        herr = hipMemcpy(t_cnt.p, &mycnt, sizeof(int32_t), hipMemcpyHostToDevice);
        int rcd = t->dist->allgather(t_cnt.p, t_cnts.p, sizeof(int32_t), s);
        if (rcd) return rcd;
        std::vector<int32_t> cnts((size_t)R);
        if (herr == hipSuccess) herr = hipStreamSynchronize(s);
        if (herr == hipSuccess) herr = hipMemcpy(cnts.data(), t_cnts.p, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (herr != hipSuccess) return fail(RL_ERR_HIP, std::string("threshold-table merge (counts): ") + hipGetErrorString(herr));
        const size_t mx = std::max<size_t>((size_t)*std::max_element(cnts.begin(), cnts.end()), 1);
        herr = t_v.get(mx * sizeof(float));
        if (herr == hipSuccess) herr = t_all.get(mx * R * sizeof(float));
        if (herr != hipSuccess) return fail(RL_ERR_HIP, std::string("hipMalloc (threshold-table merge): ") + hipGetErrorString(herr));
        herr = hipMemset(t_v.p, 0, mx * sizeof(float));
        if (herr == hipSuccess && !vals.empty()) herr = hipMemcpy(t_v.p, vals.data(), vals.size() * sizeof(float), hipMemcpyHostToDevice);
        rcd = t->dist->allgather(t_v.p, t_all.p, mx * sizeof(float), s);
        if (rcd) return rcd;
        std::vector<float> all(mx * R);
        if (herr == hipSuccess) herr = hipStreamSynchronize(s);
        if (herr == hipSuccess) herr = hipMemcpy(all.data(), t_all.p, all.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (herr != hipSuccess) return fail(RL_ERR_HIP, std::string("threshold-table merge (values): ") + hipGetErrorString(herr));
        vals.clear();
        for (int r = 0; r < R; r++) vals.insert(vals.end(), all.begin() + (size_t)r * mx, all.begin() + (size_t)r * mx + cnts[r]);
        std::sort(vals.begin(), vals.end());
        vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
        if (!vals.empty()) { fmin = vals.front(); fmax = vals.back(); }
    }
    if (nT == -1 || (long long)vals.size() <= (long long)nT) { tab = vals; tab.push_back(3.4028234663852886e38f); }      // :135-140
    else {                                                                                                              // :141-149
        const float step = fabsf(fmax - fmin) / (float)nT;
        tab.resize((size_t)nT + 1);
        tab[0] = fmin;
        for (int j = 1; j < nT; j++) tab[j] = tab[j - 1] + step;
        tab[nT] = 3.4028234663852886e38f;
    }
    return RL_OK;
}

// ---- K9: thresholds on the device; tables of more than 4 095 entries on the host -------------------------
static int init_threshold_tables(rl_trainer *t, InitWork &w)
{
    hipStream_t s = t->stream;
    const int N = t->ctx.N, Npad = t->ctx.Npad, F = w.F;
    RL_HIP(t->pool.alloc(&w.Xt, (size_t)F * Npad));
    hipLaunchKernelGGL(k_transpose, dim3((N + 31) / 32, (F + 31) / 32), dim3(kThreads), 0, s, (const float *)t->tr.d_X, w.Xt, N, F, Npad);
    const int nT = t->p.n_threshold;
    w.fs.limit = (nT == -1 || nT > kMaxBins - 1) ? kMaxBins - 1 : nT;        // the device's distinct-value sets hold up to 4 095 values; larger tables are built on the host (below)
    w.fs.HS = next_pow2(2 * (w.fs.limit + 2));
    RL_HIP(t->pool.alloc(&w.fs.minkey, (size_t)F)); RL_HIP(t->pool.alloc(&w.fs.maxkey, (size_t)F));
    RL_HIP(t->pool.alloc(&w.fs.set, (size_t)F * w.fs.HS)); RL_HIP(t->pool.alloc(&w.fs.nset, (size_t)F));
    RL_HIP(t->pool.alloc(&w.fs.overflow, (size_t)F)); RL_HIP(t->pool.alloc(&w.fs.bad, (size_t)1));
    RL_HIP(hipMemsetAsync(w.fs.minkey, 0xFF, F * sizeof(uint32_t), s));
    RL_HIP(hipMemsetAsync(w.fs.maxkey, 0, F * sizeof(uint32_t), s));
    RL_HIP(hipMemsetAsync(w.fs.set, 0, (size_t)F * w.fs.HS * sizeof(uint32_t), s));
    RL_HIP(hipMemsetAsync(w.fs.nset, 0, F * sizeof(int32_t), s));
    RL_HIP(hipMemsetAsync(w.fs.overflow, 0, F * sizeof(int32_t), s));
    RL_HIP(hipMemsetAsync(w.fs.bad, 0, sizeof(int32_t), s));
    w.slices = std::max(1, std::min(64, N / 4096));
    hipLaunchKernelGGL(k_feat_stats, dim3(F, w.slices), dim3(kThreads), w.fs.HS * sizeof(uint32_t), s, (const float *)w.Xt, N, Npad, w.fs);
    RL_HIP(hipGetLastError());
    if (t->dist) {      // global min / max / distinct sets: every rank must build the same threshold table
        int rcd = t->dist->allreduce(w.fs.minkey, F, DT_U32, OP_MIN, s); if (rcd) return rcd;
        rcd = t->dist->allreduce(w.fs.maxkey, F, DT_U32, OP_MAX, s); if (rcd) return rcd;
        rcd = t->dist->allreduce(w.fs.overflow, F, DT_I32, OP_MAX, s); if (rcd) return rcd;
        rcd = t->dist->allreduce(w.fs.bad, 1, DT_I32, OP_MAX, s); if (rcd) return rcd;
        uint32_t *gsets = nullptr;
        RL_HIP(t->pool.alloc(&gsets, (size_t)t->n_ranks * F * w.fs.HS));
        rcd = t->dist->allgather(w.fs.set, gsets, (size_t)F * w.fs.HS * sizeof(uint32_t), s); if (rcd) return rcd;
        RL_HIP(hipMemsetAsync(w.fs.set, 0, (size_t)F * w.fs.HS * sizeof(uint32_t), s));
        RL_HIP(hipMemsetAsync(w.fs.nset, 0, F * sizeof(int32_t), s));
        hipLaunchKernelGGL(k_merge_sets, dim3(F, t->n_ranks), dim3(kThreads), 0, s, (const uint32_t *)gsets, t->n_ranks, w.fs);
        RL_HIP(hipGetLastError());
        RL_HIP(hipStreamSynchronize(s));
        t->pool.release(gsets);
    }
    std::vector<int32_t> h_over(F);
    int32_t h_bad = 0;
    RL_HIP(hipStreamSynchronize(s));
    RL_HIP(hipMemcpy(h_over.data(), w.fs.overflow, F * sizeof(int32_t), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(&h_bad, w.fs.bad, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (h_bad) return fail(RL_ERR_INVALID, "NaN feature value (resolve NaN to 0 as DataPoint.getFeatureValue does)");
    if (nT == 1) {
        // -tc 1 on a column that overflows into the step table [fmin, MAX_VALUE]: a +Infinity value is above every threshold, and the Java's binning loop
        // (FeatureHistogram.java:88-107) then never assigns it -- stMap stays 0 and the counts exclude it, i.e. node counts that do not add up.  Not
        // reproduced (the binning here would put it into the last bin and count it): refused, with the reason (ADVICE r04)
        std::vector<uint32_t> h_max(F);
        RL_HIP(hipMemcpy(h_max.data(), w.fs.maxkey, F * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int f = 0; f < F; f++)
            if (h_over[f] && h_max[f] == 0xFF800000u)      // float_key(+Infinity)
                return fail(RL_ERR_UNSUPPORTED, "-tc 1 with a +Infinity value in feature column " + std::to_string(f) + ": RankLib leaves such documents out of the histogram counts (unsupported)");
    }
    const bool want_big = (nT == -1 || nT > kMaxBins - 1);         // tables of more than 4 095 entries are possible
    const int TS0 = w.fs.limit + 1;
    RL_HIP(t->pool.alloc(&w.thr0, (size_t)F * TS0)); RL_HIP(t->pool.alloc(&w.d_nthr, (size_t)F));
    hipLaunchKernelGGL(k_thresholds, dim3(F), dim3(kThreads), w.fs.HS * sizeof(uint32_t), s, w.fs, want_big ? w.fs.limit : nT, TS0, w.thr0, w.d_nthr);
    RL_HIP(hipGetLastError());
    w.h_nthr.assign((size_t)F, 0);
    RL_HIP(hipStreamSynchronize(s));
    RL_HIP(hipMemcpy(w.h_nthr.data(), w.d_nthr, F * sizeof(int32_t), hipMemcpyDeviceToHost));
    // tables of more than 4 095 entries are built on the host (init_hist_features splits them into virtual features)
    w.big.assign((size_t)F, std::vector<float>());
    if (want_big) {
        std::vector<float> colv((size_t)N);
        for (int f = 0; f < F; f++) {
            if (!h_over[f]) continue;
            { int rcb = host_table_of_column(t, w, f, nT, colv, w.big[f]); if (rcb) return rcb; }
            w.any_big = true;
        }
    }
    return RL_OK;
}

// ---- the histogram features.  Threshold tables of more than 4 095 entries (-tc -1 on a column with that many distinct values, or -tc N > 4095: learning/tree/
// LambdaMART.java:135-149 has no limit).  The histogram kernels keep a feature's bins in LDS, so such a REAL feature becomes several VIRTUAL
// features, one per run of 4 094 consecutive thresholds: virtual feature r has the table [thr[r W], .., thr[r W + W - 1], MAX_VALUE] over the same
// column.  "Smallest t with value <= table[t]" then clamps a document's real bin into the run -- documents below it join the run's first bin,
// documents above it the MAX_VALUE bin -- so the run's cumulative histogram is the real feature's cumulative histogram on its thresholds, every
// real candidate is a candidate of exactly one virtual feature, in the Java's scan order, and the MAX_VALUE bin of a run that is not the last
// never splits (nothing on its right).  Every later stage sees F = the number of virtual features; trees are exported with the real
// column (Ctx::vcol).  Then the features that can split at all, and what TS decides: fin_split, tie_on.
static int init_hist_features(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx; hipStream_t s = t->stream; const Knobs &kn = t->knobs;
    int F = w.F, TS = 2;
    const int TS0 = w.fs.limit + 1;
    t->vcol.clear();
    c.vcol = nullptr;
    if (!w.any_big) {
        for (int f = 0; f < F; f++) TS = std::max(TS, w.h_nthr[f]);
        c.TS = TS;
        RL_HIP(t->pool.alloc(&w.d_thr, (size_t)F * TS));
        RL_HIP(hipMemsetAsync(w.d_thr, 0, (size_t)F * TS * sizeof(float), s));
        RL_HIP(hipMemcpy2DAsync(w.d_thr, TS * sizeof(float), w.thr0, TS0 * sizeof(float), TS * sizeof(float), F, hipMemcpyDeviceToDevice, s));
    } else {
        if (t->p.flags & RL_FLAG_JAVA_ORDER) return fail(RL_ERR_UNSUPPORTED, "a threshold table of more than 4095 entries with RL_FLAG_JAVA_ORDER (the Java's prefix over ALL bins of a feature is one f64 chain)");
        std::vector<float> h_thr0((size_t)F * TS0);
        RL_HIP(hipMemcpy(h_thr0.data(), w.thr0, h_thr0.size() * sizeof(float), hipMemcpyDeviceToHost));
        constexpr int W = kMaxBins - 2;
        std::vector<std::vector<float>> rows;
        for (int f = 0; f < F; f++) {
            const float *tab = w.big[f].empty() ? h_thr0.data() + (size_t)f * TS0 : w.big[f].data();
            const long long T = w.big[f].empty() ? w.h_nthr[f] : (long long)w.big[f].size();
            if (T <= kMaxBins - 1) { rows.emplace_back(tab, tab + T); t->vcol.push_back(f); continue; }
            for (long long r0 = 0; r0 < T; r0 += W) {
                const long long e1 = std::min<long long>(r0 + W, T);
                std::vector<float> row(tab + r0, tab + e1);
                if (e1 < T) row.push_back(3.4028234663852886e38f);
                rows.push_back(std::move(row)); t->vcol.push_back(f);
            }
        }
        if (rows.size() > (size_t)(1 << 20)) return fail(RL_ERR_UNSUPPORTED, "threshold tables of more than 2^32 entries in total");
        F = (int)rows.size();
        for (auto &r : rows) TS = std::max(TS, (int)r.size());
        c.TS = TS;
        std::vector<float> h_thr((size_t)F * TS, 0.f);
        w.h_nthr.assign((size_t)F, 0);
        for (int v = 0; v < F; v++) { memcpy(h_thr.data() + (size_t)v * TS, rows[v].data(), rows[v].size() * sizeof(float)); w.h_nthr[v] = (int32_t)rows[v].size(); }
        t->pool.release(w.d_nthr); w.d_nthr = nullptr;
        RL_HIP(t->pool.alloc(&w.d_thr, (size_t)F * TS)); RL_HIP(t->pool.alloc(&w.d_nthr, (size_t)F));
        RL_HIP(hipMemcpy(w.d_thr, h_thr.data(), h_thr.size() * sizeof(float), hipMemcpyHostToDevice));
        RL_HIP(hipMemcpy(w.d_nthr, w.h_nthr.data(), (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice));
        int32_t *d_vcol = nullptr;
        RL_HIP(t->pool.alloc(&d_vcol, (size_t)F));
        RL_HIP(hipMemcpy(d_vcol, t->vcol.data(), (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice));
        c.vcol = d_vcol;
        c.F = F; if (!c.fs_on) c.fs_size = F;          // (with feature sampling fs_size stays a number of REAL features: the draw is over columns)
        c.node_div = kn.node_div.or_else(default_node_div(F));
        // exact ties: the first candidate in the Java's scan order.  The lazy re-decision needs the Java's own f64 prefix over ALL bins of a real feature,
        // which a run of a split table does not hold (its first bin is a merged sum)
        c.tie_on = 0;
    }
    c.thr = w.d_thr; c.nthr = w.d_nthr;
    c.live = nullptr; c.live_nthr = nullptr; c.n_live = F;
    if (!t->dist) {       // features that can split at all (> 1 distinct value <=> more than the value + Float.MAX_VALUE thresholds)
        std::vector<int32_t> live, live_n;
        for (int f = 0; f < F; f++) if (w.h_nthr[f] > 2) { live.push_back(f); live_n.push_back(w.h_nthr[f]); }
        if (live.empty()) { live.push_back(0); live_n.push_back(w.h_nthr[0]); }
        int32_t *d_live = nullptr, *d_live_n = nullptr;
        RL_HIP(t->pool.alloc(&d_live, live.size())); RL_HIP(t->pool.alloc(&d_live_n, live.size()));
        RL_HIP(hipMemcpy(d_live, live.data(), live.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        RL_HIP(hipMemcpy(d_live_n, live_n.data(), live_n.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        c.live = d_live; c.live_nthr = d_live_n; c.n_live = (int32_t)live.size();
    }
    {   // more finish blocks a step than the fused kernel keeps resident (5 a CU): the per-feature work and the bookkeeping become two launches
        int n_cu = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, t->p.device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
        t->fin_split = !t->dist && !(t->p.flags & RL_FLAG_JAVA_ORDER) && (kn.fin_split.set ? kn.fin_split.v != 0 : (long long)c.n_live * kSpec > 5ll * n_cu);
    }
    if ((size_t)TS * 12 > (size_t)kHistLdsBytes) return fail(RL_ERR_UNSUPPORTED, "too many threshold candidates for the LDS histogram");
    // sharded runs evaluate the tie-break on gathered arrays through the contiguous-chain path only: with threshold tables too large for its sort
    // (the literal walk reads one rank's documents) they keep the first candidate.  TS is the same on every rank, so is the decision.
    if (t->dist && t->n_ranks > 1 && (size_t)kTsWaves * TS * 4 > (size_t)60 * 1024) c.tie_on = 0;
    // bit 1: ties over several features that all cut a node the same way are deferred to the end of the tree like plateau ties (the check that it
    // IS one cut reads the node's documents, rl_tie.inc k_tie_verify: every rank its own, the verdict is all-reduced)
    if (c.tie_on && !kn.tie_no_xdefer) c.tie_on |= 2;
    w.F = F; w.TS = TS;
    return RL_OK;
}

// ---- bins: by feature, by group, document-major, packed; root counts, mode bins, run statistics ------------
static int init_bins(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx; hipStream_t s = t->stream; const Knobs &kn = t->knobs;
    const int N = c.N, Npad = c.Npad, F = w.F, TS = w.TS;
    if (t->p.n_leaves == -1) {      // -leaf -1: the node histograms are sized for floor(N / mls) leaves -- say so before an allocation fails
        // ADVICE r06: the estimate leaves out cum_cnt_loc, which a sharded run allocates below at the same size as cum_cnt
        const double need = (double)c.NC * F * TS * ((t->p.flags & RL_FLAG_JAVA_ORDER) ? 28.0 : 20.0);
        size_t mem_free = 0, mem_total = 0;
        RL_HIP(hipMemGetInfo(&mem_free, &mem_total));
        if (need > 0.8 * (double)mem_free) return fail(RL_ERR_UNSUPPORTED, "-leaf -1: up to " + std::to_string(t->L_eff) + " leaves would need " + std::to_string((long long)(need / 1e9)) +
                                                                          " GB of node histograms; raise -mls or set -leaf");
    }
    // features of a 16-feature group handled by one histogram block: all 16 when the LDS budget allows
    c.FG = kHistFG;
    c.numFG = (F + kHistFG - 1) / kHistFG;
    c.sub = 16;
    while (c.sub > 1 && (size_t)c.sub * TS * 12 > (size_t)kHistLdsBytes) c.sub >>= 1;

    RL_HIP(t->pool.alloc(&w.d_bins, (size_t)F * Npad));
    RL_HIP(hipMemsetAsync(w.d_bins, 0, (size_t)F * Npad * sizeof(uint16_t), s));
    RL_HIP(t->pool.alloc(&w.d_gbins, (size_t)c.numFG * Npad * kHistFG));
    RL_HIP(hipMemsetAsync(w.d_gbins, 0, (size_t)c.numFG * Npad * kHistFG * sizeof(uint16_t), s));
    c.bins = w.d_bins; c.gbins = w.d_gbins;
    // chunks of one growth step (all slots; see prepare_children), and of the root pass
    c.maxChunks = N / c.node_chunk + 67 * kSpec + 2;
    c.nTiles = (N + kPartTile - 1) / kPartTile + kSpec;      // tiles of one growth step (disjoint nodes, one ragged tile each)
    RL_HIP(t->pool.alloc(&c.cum_hi, (size_t)c.NC * F * TS));
    RL_HIP(t->pool.alloc(&c.cum_lo, (size_t)c.NC * F * TS));
    RL_HIP(t->pool.alloc(&c.cum_cnt, (size_t)c.NC * F * TS));
    RL_HIP(hipMemsetAsync(c.cum_cnt, 0, (size_t)F * TS * sizeof(int32_t), s));
    c.java = (t->p.flags & RL_FLAG_JAVA_ORDER) ? 1 : 0;
    if (c.java) {
        if (t->dist) return fail(RL_ERR_UNSUPPORTED, "RL_FLAG_JAVA_ORDER with multi-GPU training: the Java's summation order is a single sequence over all documents");
        RL_HIP(t->pool.alloc(&c.jl, (size_t)Npad)); RL_HIP(t->pool.alloc(&c.jb, (size_t)F * Npad));
        RL_HIP(t->pool.alloc(&c.jbin, (size_t)kSpec * F * TS)); RL_HIP(t->pool.alloc(&c.jtot, (size_t)kSpec * 2));
        RL_HIP(t->pool.alloc(&c.jcum, (size_t)c.NC * F * TS));
        RL_HIP(hipMemsetAsync(c.jcum, 0, (size_t)c.NC * F * TS * sizeof(double), s));
        RL_HIP(hipMemsetAsync(c.jbin, 0, (size_t)kSpec * F * TS * sizeof(double), s));
    }
    hipLaunchKernelGGL(k_binning, dim3(F, w.slices), dim3(kThreads), (size_t)TS * 8, s, (const float *)w.Xt, N, Npad, TS, (const float *)w.d_thr,
                       (const int32_t *)w.d_nthr, w.d_bins, w.d_gbins, c.cum_cnt, c.vcol);
    c.cum_cnt_loc = nullptr;
    if (t->dist && !kn.dist_count_pass) {       // this rank's own root counts, kept beside the all-reduced ones (knobs.dist_count_pass: round 5's count pass + two-pass partition)
        // ADVICE r06: 4 more bytes per entry of the node histograms, which the -leaf -1 estimate above does not count
        RL_HIP(t->pool.alloc(&c.cum_cnt_loc, (size_t)c.NC * F * TS));
        RL_HIP(hipMemsetAsync(c.cum_cnt_loc, 0, (size_t)c.NC * F * TS * sizeof(int32_t), s));
        RL_HIP(hipMemcpyAsync(c.cum_cnt_loc, c.cum_cnt, (size_t)F * TS * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    if (t->dist) { int rcd = t->dist->allreduce(c.cum_cnt, (size_t)F * TS, DT_I32, OP_SUM, s); if (rcd) return rcd; }
    {
        uint16_t *d_dbins = nullptr;
        c.dm_gstride = (c.numFG + 3) & ~3;
        RL_HIP(t->pool.alloc(&d_dbins, (size_t)c.dm_gstride * Npad * kHistFG));
        RL_HIP(hipMemsetAsync(d_dbins, 0, (size_t)c.dm_gstride * Npad * kHistFG * sizeof(uint16_t), s));
        hipLaunchKernelGGL(k_docmajor, dim3(4096), dim3(kThreads), 0, s, (const uint16_t *)w.d_gbins, d_dbins, Npad, c.numFG, c.dm_gstride);
        c.dbins = d_dbins;
        // packed rows: one byte per bin + a mask for bin 256 (possible when no table has more than 257 entries; knobs.p8 = 0 keeps the 16-bit rows)
        c.p8 = 0;
        const int p8_mode = kn.p8;        // 0 = 16-bit rows everywhere, 1 = packed rows for the root pass (default), 2 = also for child passes
        if (TS <= 257 && c.sub == 16 && p8_mode > 0) {
            unsigned char *d_pb = nullptr, *d_pd = nullptr; uint16_t *d_ph = nullptr;
            c.pd_stride = (c.numFG * 18 + 63) & ~63;
            RL_HIP(t->pool.alloc(&d_pb, (size_t)c.numFG * Npad * 16)); RL_HIP(t->pool.alloc(&d_ph, (size_t)c.numFG * Npad));
            // (document-major packed rows: for the child passes, and for a root pass that reads document-major rows -- RLHIP_DM_ROOT with the default
            // packed root pass used to read them through a null pointer)
            if (p8_mode > 1 || kn.dm_root) {
                RL_HIP(t->pool.alloc(&d_pd, (size_t)Npad * c.pd_stride));
                RL_HIP(hipMemsetAsync(d_pd, 0, (size_t)Npad * c.pd_stride, s));
            }
            hipLaunchKernelGGL(k_pack_rows, dim3(4096), dim3(kThreads), 0, s, (const uint16_t *)w.d_gbins, d_pb, d_ph, d_pd, Npad, c.numFG, c.pd_stride);
            c.pbins = d_pb; c.phib = d_ph; c.pdbins = d_pd; c.p8 = p8_mode > 1 ? 2 : 1;
        }
        c.dm_root = kn.dm_root ? 1 : 0; c.dm_div = kn.dm_div;      // (defaults 0 / 1) measured at c2 (profiles/r02d_dm_sweep.txt): every child pass gains, the root pass loses
    }
    RL_HIP(t->pool.alloc(&w.d_mode, (size_t)F));
    c.mode = w.d_mode;
    hipLaunchKernelGGL(k_cumulate_counts, dim3(F), dim3(64), 0, s, TS, (const int32_t *)w.d_nthr, c.cum_cnt, w.d_mode);
    if (c.cum_cnt_loc) {       // (the mode bins are the GLOBAL ones: the local pass only cumulates)
        int32_t *d_mode_scratch = nullptr;
        RL_HIP(t->pool.alloc(&d_mode_scratch, (size_t)F));
        hipLaunchKernelGGL(k_cumulate_counts, dim3(F), dim3(64), 0, s, TS, (const int32_t *)w.d_nthr, c.cum_cnt_loc, d_mode_scratch);
    }
    {   // columns whose bins come in runs (nine in ten documents outside the mode bin are followed by an equal bin: a quad agrees 3 times in 4)
        unsigned long long *d_rs = nullptr;
        RL_HIP(t->pool.alloc(&d_rs, (size_t)2 * F));
        hipLaunchKernelGGL(k_run_stats, dim3(F), dim3(kThreads), 0, s, (const uint16_t *)w.d_bins, (const int32_t *)w.d_mode, N, Npad, d_rs);
        std::vector<unsigned long long> h_rs((size_t)2 * F);
        RL_HIP(hipMemcpyAsync(h_rs.data(), d_rs, h_rs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        t->pool.release(d_rs);
        std::vector<uint32_t> h_runs((size_t)c.numFG, 0u);
        const bool runs_on = !kn.runs_off && c.sub == 16 && TS <= kHistLdsStride;      // the instantiation that exists
        c.any_runs = 0;
        for (int f = 0; f < F && runs_on; f++)
            if (h_rs[2 * f] >= 64 && 10 * h_rs[2 * f + 1] >= 9 * h_rs[2 * f]) { h_runs[f / kHistFG] |= 1u << (f % kHistFG); c.any_runs = 1; }
        uint32_t *d_runs = nullptr;
        RL_HIP(t->pool.alloc(&d_runs, h_runs.size()));
        RL_HIP(hipMemcpy(d_runs, h_runs.data(), h_runs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c.runs = d_runs;
    }
    return RL_OK;
}

// ---- compact rows for the child passes of sparse data (BASELINE.json configs[3]: 85 % of the cells sit in their column's mode bin), decided per
// 16-column group: a group takes them when its rows average at most 5 entries outside the mode bins and at most one row in 20 needs the
// dense fallback; built when at least half of the groups do.  knobs.crows = 0 / 1 forces them off / on for every group
static int init_compact_rows(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx; hipStream_t s = t->stream; const Knobs &kn = t->knobs;
    const int N = c.N, Npad = c.Npad, F = w.F, TS = w.TS;
    c.crows = nullptr; c.cr_stride = 0; c.cr_grp = nullptr;
    const int force = kn.crows;
    bool maybe = force == 1;
    if (c.any_runs) maybe = false;      // (launch_hist takes the RUNS instantiation on such data, which reads dense rows: the compact rows would be built and never read -- ADVICE r04)
    if (force < 0 && TS <= kHistLdsStride && c.sub == 16 && !c.any_runs) {
        // cheap look first (the exact root counts are on the device already): dense data -- more than 5 cells a row outside the mode bins on
        // average -- never builds the rows (a gigabyte of transient memory and 8 ms at the MSLR-WEB30K shape)
        { int rcc = fetch_root_counts(t, w); if (rcc) return rcc; }
        double cells = 0;
        const int32_t n_all = w.h_cum_cnt[(size_t)w.h_nthr[0] - 1];         // documents over all ranks (the counts are all-reduced when sharded)
        for (int f = 0; f < F; f++) cells += (double)cells_outside_mode(w, f, n_all);
        maybe = cells <= 5.0 * (double)n_all * (double)c.numFG;
    }
    if (maybe && TS <= kHistLdsStride && c.sub == 16) {
        unsigned long long *d_st = nullptr; uint4 *d_cr = nullptr;
        const int crs = (c.numFG + 7) & ~7;           // rows start on 128-byte lines
        RL_HIP(t->pool.alloc(&d_st, (size_t)2 * c.numFG)); RL_HIP(hipMemsetAsync(d_st, 0, (size_t)2 * c.numFG * sizeof(unsigned long long), s));
        RL_HIP(t->pool.alloc(&d_cr, (size_t)Npad * crs));
        RL_HIP(hipMemsetAsync(d_cr, 0xff, (size_t)Npad * crs * sizeof(uint4), s));
        hipLaunchKernelGGL(k_compact_rows, dim3(4096), dim3(kThreads), 0, s, (const uint16_t *)w.d_gbins, (const int32_t *)w.d_mode, d_cr, N, Npad, c.numFG, crs, F, d_st);
        std::vector<unsigned long long> h_st((size_t)2 * c.numFG);
        RL_HIP(hipMemcpyAsync(h_st.data(), d_st, h_st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        t->pool.release(d_st);
        std::vector<uint8_t> h_cg((size_t)c.numFG, 0);
        int n_on = 0; double ents = 0, over = 0;
        for (int g = 0; g < c.numFG; g++) {
            const double eg = (double)h_st[2 * g], og = (double)h_st[2 * g + 1];
            const bool on = force == 1 || (eg <= 5.0 * (double)N && og * 20.0 <= (double)N);
            h_cg[g] = on ? 1 : 0;
            if (on) { n_on++; ents += eg; over += og; }
        }
        if (force == 1 || 2 * n_on >= c.numFG) {
            uint8_t *d_cg = nullptr;
            RL_HIP(t->pool.alloc(&d_cg, (size_t)c.numFG));
            RL_HIP(hipMemcpy(d_cg, h_cg.data(), h_cg.size(), hipMemcpyHostToDevice));
            c.crows = d_cr; c.cr_stride = crs; c.cr_grp = d_cg;
            t->cr_groups = n_on; t->cr_entries = ents; t->cr_overflow = over;
        } else t->pool.release(d_cr);
    }
    RL_HIP(hipGetLastError());
    RL_HIP(hipStreamSynchronize(s));
    // (the last stage that reads the transposed rows)
    t->pool.release(w.Xt); t->pool.release(w.thr0); t->pool.release(w.fs.set);
    return RL_OK;
}

// ---- sparse-column path of the root pass (rl_csc.inc): the groups whose live columns keep at most 1 / dens of their cells
// outside the mode bins get entry lists, blocked by the root pass's chunks
static int init_sparse_root(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx; hipStream_t s = t->stream; const Knobs &kn = t->knobs;
    const int N = c.N, F = w.F, TS = w.TS;
    c.sp_on = 0; c.sp_ngroups = 0;
    const int dens = kn.csc_dens;               // 0 = no sparse path (tools/, tests)
    const int rootCs = std::min(kChunk, std::max(kMinChunk, (((N + 63) / 64 + 255) & ~255)));   // == chunk_docs<true>(N)
    const int rootChunks = (N + rootCs - 1) / rootCs;
    if (dens > 0 && !t->dist && TS <= kHistLdsStride && c.sub == 16) {
        { int rcc = fetch_root_counts(t, w); if (rcc) return rcc; }
        std::vector<int32_t> glist; std::vector<uint8_t> isg(c.numFG, 0);
        int sp_cols = 0;
        for (int g = 0; g < c.numFG; g++) {
            int64_t cells = 0, live = 0;
            for (int f = g * kHistFG; f < std::min(F, (g + 1) * kHistFG); f++) {
                if (w.h_nthr[f] <= 2) continue;                                   // dead column: its only bin is its mode bin
                cells += cells_outside_mode(w, f, N);           // (not sharded: this rank's documents are all of them)
                live++;
            }
            if (cells * dens <= (int64_t)N * live) { isg[g] = 1; glist.push_back(g); sp_cols += (int)live; }   // groups of dead columns too: nothing to read
        }
        if (!glist.empty()) {
            const int nsg = (int)glist.size();
            int32_t *d_glist = nullptr, *d_cnt = nullptr, *d_off = nullptr; uint8_t *d_isg = nullptr; uint32_t *d_ent = nullptr;
            RL_HIP(t->pool.alloc(&d_glist, (size_t)nsg)); RL_HIP(t->pool.alloc(&d_cnt, (size_t)nsg * rootChunks)); RL_HIP(t->pool.alloc(&d_off, (size_t)nsg * rootChunks + 1));
            RL_HIP(t->pool.alloc(&d_isg, (size_t)c.numFG));
            RL_HIP(hipMemcpy(d_glist, glist.data(), nsg * sizeof(int32_t), hipMemcpyHostToDevice));
            RL_HIP(hipMemcpy(d_isg, isg.data(), c.numFG, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_sp_build<false>, dim3(nsg, rootChunks), dim3(kThreads), 0, s, c, (const int32_t *)d_glist, nsg, rootCs, d_cnt, (const int32_t *)nullptr, (uint32_t *)nullptr);
            RL_HIP(hipGetLastError());
            RL_HIP(hipStreamSynchronize(s));
            std::vector<int32_t> cnt((size_t)nsg * rootChunks), off((size_t)nsg * rootChunks + 1);
            RL_HIP(hipMemcpy(cnt.data(), d_cnt, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            int64_t E = 0;
            for (size_t i = 0; i < cnt.size(); i++) { off[i] = (int32_t)E; E += cnt[i]; }
            if (E < 2000000000ll) {
                off[cnt.size()] = (int32_t)E;
                RL_HIP(t->pool.alloc(&d_ent, (size_t)E));
                RL_HIP(hipMemcpy(d_off, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
                hipLaunchKernelGGL(k_sp_build<true>, dim3(nsg, rootChunks), dim3(kThreads), 0, s, c, (const int32_t *)d_glist, nsg, rootCs, (int32_t *)nullptr, (const int32_t *)d_off, d_ent);
                RL_HIP(hipGetLastError());
                RL_HIP(hipStreamSynchronize(s));
                c.sp_on = 1; c.sp_ngroups = nsg; c.sp_grp = d_isg; c.sp_glist = d_glist; c.sp_ent = d_ent; c.sp_off = d_off;
                t->sp_entries = E; t->sp_cols = sp_cols;
            }
        }
    }
    return RL_OK;
}

// ---- RL_FLAG_JAVA_ORDER: the deal of a feature's bins to the wavefronts of k_jhist2 ------------------------------
static int init_java_deal(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx;
    const int N = c.N, F = w.F, TS = w.TS;
    if (!(c.java && TS <= kJ2MaxBins && !t->knobs.jhist_v1)) return RL_OK;
    // k_jhist2's deal of a feature's bins to the 8 wavefronts of its block: consecutive bins until a wavefront owns about an
    // eighth of the documents (root counts) or 64 bins; a bin that fills a share on its own keeps the wavefront to itself
    { int rcc = fetch_root_counts(t, w); if (rcc) return rcc; }
    const std::vector<int32_t> &h_cnt = w.h_cum_cnt;
    std::vector<uint16_t> jmap((size_t)F * TS, 0), jinv((size_t)F * kJ2MaxBins, 0xffffu);
    std::vector<uint32_t> jone(F, 0);
    for (int f = 0; f < F; f++) {
        const int T = w.h_nthr[f];
        // a wavefront's quota = (documents not dealt yet) / (wavefronts left), taken when it starts; a bin joins the current wavefront
        // while that brings it closer to its quota.  A wavefront that owns ONE bin adds without an owner test (8 cycles a sample
        // against ~20): a bin that fills more than 40 % of a quota-sized share on its own is therefore kept alone.
        int wv = 0, used = 0, wbins[kJ2Waves] = {0};
        int64_t docs = 0, left = N, quota = std::max<int64_t>(1, (int64_t)N / kJ2Waves);
        for (int tb = 0; tb < T; tb++) {
            const int64_t nb = (int64_t)h_cnt[(size_t)f * TS + tb] - (tb > 0 ? h_cnt[(size_t)f * TS + tb - 1] : 0);
            const bool room_later = (T - tb) <= (kJ2Waves - wv - 1) * 64;          // the wavefronts after this one can still hold all remaining bins
            const bool alone = nb * 5 > quota * 2;
            const bool full = used == 64 || docs + nb / 2 > quota || alone || (used == 1 && docs * 5 > quota * 2);
            if (wv < kJ2Waves - 1 && used > 0 && room_later && full) {
                wv++; used = 0; left -= docs; docs = 0;
                quota = std::max<int64_t>(1, left / (kJ2Waves - wv));
            }
            jmap[(size_t)f * TS + tb] = (uint16_t)((wv << 8) | used);
            jinv[(size_t)f * kJ2MaxBins + wv * 64 + used] = (uint16_t)tb;
            used++; docs += nb; wbins[wv]++;
        }
        for (int v = 0; v < kJ2Waves; v++) if (wbins[v] == 1) jone[f] |= 1u << v;
    }
    uint16_t *d_map = nullptr, *d_inv = nullptr; uint32_t *d_one = nullptr;
    RL_HIP(t->pool.alloc(&d_map, jmap.size())); RL_HIP(t->pool.alloc(&d_inv, jinv.size())); RL_HIP(t->pool.alloc(&d_one, jone.size()));
    RL_HIP(hipMemcpy(d_map, jmap.data(), jmap.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_inv, jinv.data(), jinv.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_one, jone.data(), jone.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c.jmap = d_map; c.jinv = d_inv; c.jone = d_one;
    return RL_OK;
}

// ---- query side: ideal DCGs with the qid-keyed cache quirk (NDCGScorer.java:114-122,134-143) --
static int init_query_side(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx;
    const int F = w.F;
    const std::vector<double> disc = discount_table(std::max(t->tr.maxq, t->has_valid ? t->va.maxq : 0));
    double *d_disc = nullptr;
    RL_HIP(t->pool.alloc(&d_disc, disc.size()));
    RL_HIP(hipMemcpy(d_disc, disc.data(), disc.size() * sizeof(double), hipMemcpyHostToDevice));
    c.disc = d_disc;
    {
        auto upload_rd = [&](DataSet &d) -> int {
            if (d.ext_rd.empty()) return RL_OK;
            RL_HIP(t->pool.alloc(&d.d_ext_rd, (size_t)d.Q));
            RL_HIP(hipMemcpy(d.d_ext_rd, d.ext_rd.data(), (size_t)d.Q * sizeof(int32_t), hipMemcpyHostToDevice));
            return RL_OK;
        };
        { int rcu = upload_rd(t->tr); if (rcu) return rcu; if (t->has_valid) { rcu = upload_rd(t->va); if (rcu) return rcu; } }
        // round 0 scores a list against its own ideal (ideal0), the later rounds against the cache's entry (ideal1): ideal_cache, rl_lists_host.h
        const int k = t->p.metric_k;
        std::vector<double> own[2], cached[2];
        ideal_cache(t->tr, t->has_valid ? &t->va : nullptr, disc, [k](int n) { return std::min(n, k); }, cached, own);
        int rc = upload_query_side(t, t->tr, own[0], cached[0]);
        if (rc) return rc;
        if (t->has_valid && (rc = upload_query_side(t, t->va, own[1], cached[1]))) return rc;
    }
    c.labels = t->tr.d_labels; c.qoff = t->tr.d_qoff; c.ideal0 = t->tr.d_ideal0; c.ideal1 = t->tr.d_ideal1;
    c.scores = t->tr.d_scores; c.ndcg_q = t->tr.d_ndcg;
    int32_t *d_fid = nullptr;
    RL_HIP(t->pool.alloc(&d_fid, (size_t)F));
    {   // feature sampling draws REAL features: the column behind every histogram feature, the later runs of a split table marked (half_wave_best_feature)
        std::vector<int32_t> fc((size_t)F);
        for (int v = 0; v < F; v++) {
            const int col = t->vcol.empty() ? v : t->vcol[v];
            fc[v] = (v > 0 && !t->vcol.empty() && t->vcol[v - 1] == col) ? (int32_t)((uint32_t)col | 0x80000000u) : col;
        }
        int32_t *d_fc = nullptr;
        RL_HIP(t->pool.alloc(&d_fc, (size_t)F));
        RL_HIP(hipMemcpy(d_fc, fc.data(), (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice));
        c.fcol = d_fc;
    }
    {   // (ids of the histogram features: a virtual feature carries its real column's id)
        std::vector<int32_t> ids((size_t)F);
        for (int v = 0; v < F; v++) ids[v] = t->feature_ids[t->vcol.empty() ? v : t->vcol[v]];
        RL_HIP(hipMemcpy(d_fid, ids.data(), F * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    c.feature_ids = d_fid;
    return RL_OK;
}

// ---- per-round state -------------------------------------------------------------------------
static int init_round_state(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx; const Knobs &kn = t->knobs;
    const int N = c.N, F = w.F, TS = w.TS;
    RL_HIP(t->pool.alloc(&c.lw, (size_t)N));
    RL_HIP(hipMemset(c.lw, 0, (size_t)N * sizeof(double2)));   // MART writes zero weights (MART.java:47-51)
    RL_HIP(t->pool.alloc(&c.q, (size_t)N)); RL_HIP(t->pool.alloc(&c.r, (size_t)N));
    RL_HIP(t->pool.alloc(&c.idx[0], (size_t)N)); RL_HIP(t->pool.alloc(&c.idx[1], (size_t)N));
    RL_HIP(t->pool.alloc(&c.ql[0], (size_t)N)); RL_HIP(t->pool.alloc(&c.ql[1], (size_t)N));
    RL_HIP(t->pool.alloc(&c.nodes, (size_t)c.NC + 2)); RL_HIP(t->pool.alloc(&c.st, (size_t)1));
    RL_HIP(hipMemset(c.st, 0, sizeof(TreeState)));
    t->tree_seq = 0;
    // the progress word is an optimisation: without host-visible coherent memory the host simply enqueues every step
    c.progress = nullptr;
    if (!t->h_progress && hipHostMalloc((void **)&t->h_progress, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        t->h_progress = nullptr; (void)hipGetLastError();
    }
    if (t->h_progress) {
        *t->h_progress = 0;
        if (t->knobs.step_ahead > 0 && hipHostGetDevicePointer((void **)&c.progress, t->h_progress, 0) != hipSuccess) {
            c.progress = nullptr; (void)hipGetLastError();
        }
    }
    if (t->dist) {
        // Sharded runs: every rank must enqueue the same collectives, so the way a tree's end is detected has to be the same on
        // all of them: the progress word (deterministic rule in growth_gate, rl_round.inc) only if every rank has one, else the stream
        // synchronisation at fixed steps.
        int32_t have = c.progress != nullptr ? 1 : 0, *d_have = nullptr;
        RL_HIP(t->pool.alloc(&d_have, (size_t)1));
        RL_HIP(hipMemcpy(d_have, &have, sizeof(have), hipMemcpyHostToDevice));
        int rcd = t->dist->allreduce(d_have, 1, DT_I32, OP_MIN, t->stream);
        if (rcd) return rcd;
        RL_HIP(hipStreamSynchronize(t->stream));
        RL_HIP(hipMemcpy(&have, d_have, sizeof(have), hipMemcpyDeviceToHost));
        if (!have) c.progress = nullptr;
    }
    RL_HIP(hipMemset(c.nodes, 0, ((size_t)c.NC + 2) * sizeof(NodeRec)));
    RL_HIP(t->pool.alloc(&c.queue, (size_t)c.MAXN + 2));
    RL_HIP(t->pool.alloc(&c.part_sum, (size_t)c.maxChunks * F * TS)); RL_HIP(t->pool.alloc(&c.part_cnt, (size_t)c.maxChunks * F * TS));
    RL_HIP(t->pool.alloc(&c.part_tot, (size_t)std::max(c.maxChunks, (N + kMinChunk - 1) / kMinChunk) + 1));
    RL_HIP(t->pool.alloc(&c.fb, (size_t)kSpec * 2 * F));
    {   // records of features that never get a finish block: "no admissible split"
        std::vector<FeatBest> init((size_t)kSpec * 2 * F);
        const double m1 = -1.0;
        for (auto &r : init) { memcpy(&r.S, &m1, 8); r.hi = 0; r.lo = 0; r.tc = 0; }
        RL_HIP(hipMemcpy(c.fb, init.data(), init.size() * sizeof(FeatBest), hipMemcpyHostToDevice));
    }
    RL_HIP(t->pool.alloc(&c.fb_root, (size_t)2 + kSpec)); c.fb_sq = c.fb_root + 2;
    RL_HIP(t->pool.alloc(&c.tile_cnt, (size_t)c.nTiles)); RL_HIP(t->pool.alloc(&c.tile_sq, (size_t)c.nTiles));
    RL_HIP(t->pool.alloc(&c.tile_desc, (size_t)c.nTiles)); RL_HIP(hipMemset(c.tile_desc, 0, (size_t)c.nTiles * 8));
    RL_HIP(t->pool.alloc(&c.tile_gdesc, (size_t)c.nTiles / 64 + kSpec + 2)); RL_HIP(hipMemset(c.tile_gdesc, 0, ((size_t)c.nTiles / 64 + kSpec + 2) * 8));
    RL_HIP(t->pool.alloc(&c.grow_stats, (size_t)4)); RL_HIP(hipMemset(c.grow_stats, 0, 16));
    RL_HIP(t->pool.alloc(&c.grow_docs, (size_t)10)); RL_HIP(hipMemset(c.grow_docs, 0, 80));      // ([4..9]: bubble stamps, RL_ARR_BUBBLES)
    c.steplog = nullptr;
    if (kn.steplog) { RL_HIP(t->pool.alloc(&c.steplog, (size_t)8 + 8 * kStepLogCap)); RL_HIP(hipMemset(c.steplog, 0, ((size_t)8 + 8 * kStepLogCap) * sizeof(int32_t))); }
    RL_HIP(t->pool.alloc(&c.clk, (size_t)64 * 32));
    RL_HIP(hipMemset(c.clk, 0, 64 * 32 * sizeof(long long)));
    c.trace_tree = -1;
    c.trace = nullptr;
    if (kn.trace_tree.set) {
        c.trace_tree = kn.trace_tree.v;
        RL_HIP(t->pool.alloc(&c.trace, (size_t)64 * 3 * kTraceBlocks * kTraceStamps)); RL_HIP(hipMemset(c.trace, 0, (size_t)64 * 3 * kTraceBlocks * kTraceStamps * sizeof(long long)));
    }
    RL_HIP(t->pool.alloc(&c.leaf_node, (size_t)c.MAXN + 1)); RL_HIP(t->pool.alloc(&c.leaf_start, (size_t)c.MAXN + 2));
    RL_HIP(t->pool.alloc(&c.leaf_of, (size_t)c.Npad + 64));
    RL_HIP(t->pool.alloc(&c.round_metric, (size_t)2 * t->p.n_trees));
    RL_HIP(hipMemset(c.round_metric, 0, (size_t)2 * t->p.n_trees * sizeof(float)));
    RL_HIP(hipMemset(c.lw, 0, N * sizeof(double2)));
    // ensemble
    const size_t en = (size_t)t->p.n_trees * c.MAXN;
    RL_HIP(t->pool.alloc(&t->ens.feat_idx, en)); RL_HIP(t->pool.alloc(&t->ens.thr, en));
    RL_HIP(t->pool.alloc(&t->ens.left, en)); RL_HIP(t->pool.alloc(&t->ens.right, en));
    RL_HIP(t->pool.alloc(&t->ens.out, en)); RL_HIP(t->pool.alloc(&t->ens.count, en)); RL_HIP(t->pool.alloc(&t->ens.deviance, en));
    RL_HIP(t->pool.alloc(&t->ens.n_nodes, (size_t)t->p.n_trees));
    RL_HIP(hipMemset(t->ens.n_nodes, 0, t->p.n_trees * sizeof(int32_t)));
    RL_HIP(t->pool.alloc(&t->d_mean, (size_t)2));
    return RL_OK;
}

// ---- float chains; sharded runs: sizes of every rank, exchange buffers ------------------------------------
static int init_dist_state(rl_trainer *t, InitWork &w)
{
    Ctx &c = t->ctx; hipStream_t s = t->stream; const Knobs &kn = t->knobs;
    const int N = c.N, F = w.F, TS = w.TS;
    int64_t Nmax = N;
    t->Qglobal = t->tr.Q; t->Qmax = t->tr.Q; t->Nglobal = N; c.Nglobal = N;
    if (t->dist) {      // sizes of every rank
        // every rank either has a validation shard or none has (checked below through the gathered sizes)
        int32_t *d_sz = nullptr, *d_all = nullptr;
        RL_HIP(t->pool.alloc(&d_sz, (size_t)4)); RL_HIP(t->pool.alloc(&d_all, (size_t)4 * t->n_ranks));
        const int32_t mine[4] = {N, t->tr.Q, t->has_valid ? t->va.Q : 0, t->has_valid ? 1 : 0};
        RL_HIP(hipMemcpy(d_sz, mine, sizeof(mine), hipMemcpyHostToDevice));
        int rcd = t->dist->allgather(d_sz, d_all, sizeof(mine), s); if (rcd) return rcd;
        std::vector<int32_t> all((size_t)4 * t->n_ranks), all_vQ;
        RL_HIP(hipStreamSynchronize(s));
        RL_HIP(hipMemcpy(all.data(), d_all, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        t->all_N.clear(); t->all_Q.clear(); t->Nglobal = 0; t->Qglobal = 0; t->Qmax = 0; t->vQglobal = 0; t->vQmax = 0;
        for (int r = 0; r < t->n_ranks; r++) {
            t->all_N.push_back(all[4 * r]); t->all_Q.push_back(all[4 * r + 1]); all_vQ.push_back(all[4 * r + 2]);
            t->Nglobal += all[4 * r]; t->Qglobal += all[4 * r + 1]; t->vQglobal += all[4 * r + 2];
            Nmax = std::max<int64_t>(Nmax, all[4 * r]); t->Qmax = std::max(t->Qmax, all[4 * r + 1]); t->vQmax = std::max(t->vQmax, all[4 * r + 2]);
            if ((all[4 * r + 3] != 0) != t->has_valid) return fail(RL_ERR_INVALID, "multi-GPU training: either every rank sets a validation shard or none does");
        }
        if (t->has_valid) {
            RL_HIP(t->pool.alloc(&t->d_vqsend, (size_t)t->vQmax)); RL_HIP(t->pool.alloc(&t->d_vqgath, (size_t)t->n_ranks * t->vQmax));
            RL_HIP(t->pool.alloc(&t->d_vqcat, (size_t)t->vQglobal)); RL_HIP(t->pool.alloc(&t->d_vallQ, (size_t)t->n_ranks));
            RL_HIP(hipMemcpy(t->d_vallQ, all_vQ.data(), t->n_ranks * sizeof(int32_t), hipMemcpyHostToDevice));
            RL_HIP(hipMemset(t->d_vqsend, 0, (size_t)t->vQmax * sizeof(double)));
        }
        if (t->Nglobal >= (int64_t)2147483647 - 4096) return fail(RL_ERR_UNSUPPORTED, "more than 2^31 documents in total");
        c.Nglobal = (int32_t)t->Nglobal;
    }
    int rc = alloc_chain(t, t->leaf_chain, c.MAXN + 1, 2, Nmax, true);
    if (rc) return rc;
    rc = alloc_chain(t, t->metric_chain, 1, 1, std::max(t->Qglobal, t->has_valid ? std::max(t->va.Q, t->vQglobal) : 0));
    if (rc) return rc;
    RL_HIP(t->pool.alloc(&t->d_seg_buf, (size_t)c.MAXN + 2));
    if (t->p.flags & RL_FLAG_FAST_LEAF) {       // rl_fast_leaf.inc: one partial per tile slot, one pair of sums per leaf (one GPU: rl_dist_init* refuses the flag)
        t->fast_slots = fast_leaf_slots(N, c.MAXN + 1);
        RL_HIP(t->pool.alloc(&t->d_fast_part, (size_t)t->fast_slots)); RL_HIP(t->pool.alloc(&t->d_fast_sums, (size_t)c.MAXN + 1));
    }
    if (t->dist) {
        t->lsstride = c.MAXN + 2;
        // piece mode (rl_dist.inc): the leaves' float chains from every rank's own pieces; the leaf-owner exchange for what it does not cover
        // (more than 256 leaves: the gathered tables grow with leaves x ranks; RL_FLAG_SERIAL_CHAIN) or on request (knobs.dist_owner_chains)
        // pinned mailbox: the transfer sizes of k_plan_exchange / the pending pieces of k_chain_cross reach the host without a stream synchronisation
        if (!t->h_xmail && hipHostMalloc((void **)&t->h_xmail, (size_t)(4 * 64 + 1) * sizeof(long long), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            memset(t->h_xmail, 0, (size_t)(4 * 64 + 1) * sizeof(long long));
            if (hipHostGetDevicePointer((void **)&t->d_xmail, t->h_xmail, 0) != hipSuccess) { t->d_xmail = nullptr; (void)hipGetLastError(); }
        } else (void)hipGetLastError();
        t->piece_chains = t->d_xmail != nullptr && !kn.dist_owner_chains && c.MAXN + 1 <= 256 && t->n_ranks <= 64 && !(t->p.flags & RL_FLAG_SERIAL_CHAIN);
        const bool owner_bufs = !t->piece_chains;
        if (owner_bufs) { rc = alloc_chain(t, t->gchain, c.MAXN + 1, 2, t->Nglobal, true); if (rc) return rc; }
        else { rc = alloc_chain(t, t->gchain, c.MAXN + 1, 2, 1024, true); if (rc) return rc; }       // (a stub: rl_get_array's statistics read leaf_chain in piece mode)
        RL_HIP(t->pool.alloc(&t->d_gx, owner_bufs ? (size_t)2 * t->Nglobal + 2 : (size_t)2));              // at worst one rank owns every leaf
        RL_HIP(t->pool.alloc(&t->d_send, owner_bufs ? (size_t)2 * N + 2 : (size_t)2));
        if (t->piece_chains) {
            const size_t n2 = (size_t)2 * (c.MAXN + 1), Rn = (size_t)t->n_ranks;
            RL_HIP(t->pool.alloc(&t->d_pc_loc, n2)); RL_HIP(t->pool.alloc(&t->d_pc_all, Rn * n2)); RL_HIP(t->pool.alloc(&t->d_pc_base, n2));
            RL_HIP(t->pool.alloc(&t->d_ptab, n2 * (kChainW + 1))); RL_HIP(t->pool.alloc(&t->d_gtab, Rn * n2 * (kChainW + 1)));
            RL_HIP(t->pool.alloc(&t->d_res_loc, n2)); RL_HIP(t->pool.alloc(&t->d_res_all, Rn * n2));
            RL_HIP(t->pool.alloc(&t->xstate.key, n2)); RL_HIP(t->pool.alloc(&t->xstate.rank, n2)); RL_HIP(t->pool.alloc(&t->xstate.pending, n2));
            RL_HIP(hipMemset(t->xstate.key, 0, n2 * 4)); RL_HIP(hipMemset(t->xstate.rank, 0, n2 * 4)); RL_HIP(hipMemset(t->xstate.pending, 0, n2 * 4));
            RL_HIP(hipMemset(t->d_res_all, 0, Rn * n2 * 4)); RL_HIP(hipMemset(t->d_ptab, 0, n2 * (kChainW + 1) * 4));
        }
        RL_HIP(t->pool.alloc(&t->d_own, (size_t)c.MAXN + 1)); RL_HIP(t->pool.alloc(&t->d_xtab, (size_t)(c.MAXN + 1) * (t->n_ranks + 1)));
        RL_HIP(t->pool.alloc(&t->d_gls, (size_t)t->n_ranks * t->lsstride));
        RL_HIP(t->pool.alloc(&t->d_gres, (size_t)t->n_ranks * 2 * (c.MAXN + 1) + 8));
        RL_HIP(t->pool.alloc(&t->d_qsend, (size_t)t->Qmax)); RL_HIP(t->pool.alloc(&t->d_qgath, (size_t)t->n_ranks * t->Qmax));
        RL_HIP(t->pool.alloc(&t->d_qcat, (size_t)t->Qglobal)); RL_HIP(t->pool.alloc(&t->d_allQ, (size_t)t->n_ranks));
        RL_HIP(hipMemcpy(t->d_allQ, t->all_Q.data(), t->n_ranks * sizeof(int32_t), hipMemcpyHostToDevice));
        RL_HIP(hipMemset(t->d_qsend, 0, (size_t)t->Qmax * sizeof(double)));
        c.limb_words = t->Nglobal < (1ll << 25) ? 2 : 3;
        RL_HIP(t->pool.alloc(&c.dist_buf, ((size_t)F * TS * 3 + 4) * kSpec));
        RL_HIP(hipMemset(c.dist_buf, 0, ((size_t)F * TS * 3 + 4) * kSpec * sizeof(long long)));
    }
    return RL_OK;
}

// ---- ranked-order arrays + pair-term matrix of the lambda kernels ----------------------------------------
static int init_lambda_state(rl_trainer *t)
{
    Ctx &c = t->ctx; const Knobs &kn = t->knobs;
    const int N = c.N;
    DataSet &d = t->tr;
    RL_HIP(t->pool.alloc(&d.d_ss, (size_t)N)); RL_HIP(t->pool.alloc(&d.d_sl, (size_t)N));
    RL_HIP(t->pool.alloc(&d.d_srel, (size_t)N)); RL_HIP(t->pool.alloc(&d.d_sidx, (size_t)N)); RL_HIP(t->pool.alloc(&d.d_docq, (size_t)N));
    std::vector<int32_t> docq((size_t)N);
    for (int q = 0; q < d.Q; q++) for (int i = d.qoff[q]; i < d.qoff[q + 1]; i++) docq[i] = q;
    RL_HIP(hipMemcpy(d.d_docq, docq.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    // the LDS-resident fused kernel serves every metric with few rows (k <= kLambdaFusedMaxK); longer cutoffs go through the pair-term matrix
    const bool fused = !c.mart && c.k <= kLambdaFusedMaxK && !kn.lambda_unfused;
    if (!c.mart && !fused) {
        if ((size_t)N * c.k * sizeof(double2) > ((size_t)16 << 30)) return fail(RL_ERR_UNSUPPORTED, "this metric cutoff needs more than 16 GiB of pair terms");
        RL_HIP(t->pool.alloc(&t->d_T, (size_t)N * c.k));
    }
    RL_HIP(t->pool.alloc(&t->d_wmax, (size_t)std::max(std::max(d.Q, (N + kThreads - 1) / kThreads), 2048) + 1));
    if (c.metric == RL_METRIC_MAP) RL_HIP(t->pool.alloc(&d.d_aux_i, (size_t)N));
    if (c.metric == RL_METRIC_RR) RL_HIP(t->pool.alloc(&d.d_aux_i, (size_t)2 * d.Q));      // firstRank, secondRank of every list (written by the rank kernels)
    if (c.metric == RL_METRIC_ERR) {     // R[] / np[]: the rank kernels only ever write the top min(k, n) positions of a list, the rest stays 0
        RL_HIP(t->pool.alloc(&d.d_aux_a, (size_t)N)); RL_HIP(t->pool.alloc(&d.d_aux_b, (size_t)N));
        RL_HIP(hipMemset(d.d_aux_a, 0, (size_t)N * sizeof(double))); RL_HIP(hipMemset(d.d_aux_b, 0, (size_t)N * sizeof(double)));
    }
    RL_HIP(hipDeviceSynchronize());
    int rc = launch_rank(t, d, c.scores, d.d_ndcg, true);      // ranking of the all-zero start scores (file order)
    if (rc) return rc;
    return RL_OK;
}

}  // namespace rl
