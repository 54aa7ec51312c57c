// rl_debug_abi.inc -- the rl_debug_* entry points: probes of single device routines for the tests and tools, no trainer handle.
// Included inside the extern "C" block of rl_trainer.hip.
int rl_debug_exp(const double *x, int32_t n, double *out_fast, double *out_ref)
{
    if (!x || !out_fast || !out_ref || n < 0) return fail(RL_ERR_INVALID, "bad argument");
    if (n == 0) return RL_OK;
    double *d = nullptr;
    RL_HIP(hipMalloc((void **)&d, (size_t)n * 3 * sizeof(double)));
    RL_HIP(hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_exp_probe, dim3((n + 255) / 256), dim3(256), 0, 0, (const double *)d, n, d + n, d + 2 * (size_t)n);
    RL_HIP(hipGetLastError());
    RL_HIP(hipDeviceSynchronize());
    RL_HIP(hipMemcpy(out_fast, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(out_ref, d + 2 * (size_t)n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return RL_OK;
}

int rl_debug_rho(const double *x, const double *den, int32_t n, double *out_fast, double *out_ref)
{
    if (!x || !out_fast || !out_ref || n < 0) return fail(RL_ERR_INVALID, "bad argument");
    if (n == 0) return RL_OK;
    double *d = nullptr;
    RL_HIP(hipMalloc((void **)&d, (size_t)n * 4 * sizeof(double)));
    RL_HIP(hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    if (den) {
        RL_HIP(hipMemcpy(d + 3 * (size_t)n, den, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_div_probe, dim3((n + 255) / 256), dim3(256), 0, 0, (const double *)d, (const double *)(d + 3 * (size_t)n), n, d + n, d + 2 * (size_t)n);
    } else
        hipLaunchKernelGGL(k_rho_probe, dim3((n + 255) / 256), dim3(256), 0, 0, (const double *)d, n, d + n, d + 2 * (size_t)n);
    RL_HIP(hipGetLastError());
    RL_HIP(hipDeviceSynchronize());
    RL_HIP(hipMemcpy(out_fast, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(out_ref, d + 2 * (size_t)n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return RL_OK;
}

int rl_debug_float_chain(int32_t device, const double *x, int64_t n, const int64_t *seg_start, int32_t n_seg, float *out, int32_t *stats)
{
    if (!x || !seg_start || !out || n < 0 || n_seg < 1 || n > 2147483647 / 2) return fail(RL_ERR_INVALID, "bad argument");
    for (int i = 0; i < n_seg; i++) if (seg_start[i] > seg_start[i + 1]) return fail(RL_ERR_INVALID, "segments must be ascending");
    if (seg_start[0] != 0 || seg_start[n_seg] != n) return fail(RL_ERR_INVALID, "segments must cover [0, n)");
    RL_HIP(hipSetDevice(device));
    std::unique_ptr<rl_trainer> t(new rl_trainer());      // only the pool, the stream and the chain bookkeeping are used
    memset(&t->ctx, 0, sizeof(t->ctx)); memset(&t->ens, 0, sizeof(t->ens)); memset(&t->p, 0, sizeof(t->p));
    t->p.device = device;
    RL_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    RL_HIP(hipFuncSetAttribute((const void *)k_chain_stitch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    RL_HIP(hipFuncSetAttribute((const void *)k_tie_finish, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    struct Guard { rl_trainer *t; ~Guard() { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); for (void *q : t->pinned) (void)hipHostFree(q); } } guard{t.get()};
    ChainBufs b;
    int rc = alloc_chain(t.get(), b, n_seg, 1, n, true);
    if (rc) return rc;
    std::vector<int32_t> ss(n_seg + 1), st0(n_seg + 1);
    int32_t tiles = 0;
    for (int i = 0; i <= n_seg; i++) {
        ss[i] = (int32_t)seg_start[i]; st0[i] = tiles;
        if (i < n_seg) tiles += (int32_t)((seg_start[i + 1] - seg_start[i] + kChainTile - 1) / kChainTile);
    }
    ChainPlan plan{n_seg, tiles, tiles + n_seg, (int32_t)n};
    double *dx = nullptr;
    RL_HIP(t->pool.alloc(&dx, (size_t)std::max<int64_t>(n, 1)));
    RL_HIP(hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(b.seg_start, ss.data(), ss.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(b.seg_tile0, st0.data(), st0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(b.plan, &plan, sizeof(plan), hipMemcpyHostToDevice));
    ChainSource src{dx, nullptr, nullptr, nullptr, nullptr, nullptr};
    enqueue_chain(t.get(), b, src);
    RL_HIP(hipGetLastError());
    RL_HIP(hipStreamSynchronize(t->stream));
    RL_HIP(hipMemcpy(out, b.result, (size_t)n_seg * sizeof(float), hipMemcpyDeviceToHost));
    if (stats) RL_HIP(hipMemcpy(stats, b.stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RL_OK;
}

int rl_debug_fast_sum(int32_t device, const double *x, int64_t n, const int64_t *seg_start, int32_t n_seg, double *out_f64, float *out_f32)
{
    if ((!x && n > 0) || !seg_start || n < 0 || n_seg < 1 || n > 2147483647 / 2) return fail(RL_ERR_INVALID, "bad argument");
    for (int i = 0; i < n_seg; i++) if (seg_start[i] > seg_start[i + 1]) return fail(RL_ERR_INVALID, "segments must be ascending");
    if (seg_start[0] != 0 || seg_start[n_seg] != n) return fail(RL_ERR_INVALID, "segments must cover [0, n)");
    RL_HIP(hipSetDevice(device));
    DevPool pool;
    // both value arrays carry x: the two sums of a leaf go through the same instructions side by side, and must come out equal
    std::vector<double2> pair((size_t)n);
    for (int64_t i = 0; i < n; i++) pair[(size_t)i] = make_double2(x[i], x[i]);
    std::vector<int32_t> ss((size_t)n_seg + 1);
    for (int i = 0; i <= n_seg; i++) ss[i] = (int32_t)seg_start[i];
    double2 *d_pair = nullptr, *d_part = nullptr, *d_sums = nullptr; int32_t *d_ss = nullptr;
    const int64_t slots = fast_leaf_slots(n, n_seg);
    RL_HIP(pool.alloc(&d_pair, (size_t)n)); RL_HIP(pool.alloc(&d_part, (size_t)slots)); RL_HIP(pool.alloc(&d_sums, (size_t)n_seg)); RL_HIP(pool.alloc(&d_ss, ss.size()));
    if (n > 0) RL_HIP(hipMemcpy(d_pair, pair.data(), (size_t)n * sizeof(double2), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_ss, ss.data(), ss.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    const FastLeafArgs fa{d_pair, nullptr, nullptr, nullptr, d_ss, nullptr, n_seg, nullptr, d_part, (int32_t)slots, d_sums, nullptr, nullptr, 0};
    hipLaunchKernelGGL(k_fast_leaf_tiles, dim3((unsigned)slots), dim3(kFastTile), 0, 0, fa);
    hipLaunchKernelGGL(k_fast_leaf_finish, dim3((unsigned)n_seg), dim3(kFastTile), 0, 0, fa);
    RL_HIP(hipGetLastError());
    RL_HIP(hipDeviceSynchronize());
    std::vector<double2> sums((size_t)n_seg);
    RL_HIP(hipMemcpy(sums.data(), d_sums, (size_t)n_seg * sizeof(double2), hipMemcpyDeviceToHost));
    for (int i = 0; i < n_seg; i++) {
        if (memcmp(&sums[i].x, &sums[i].y, sizeof(double)) != 0) return fail(RL_ERR_HIP, "rl_debug_fast_sum: the two sums of segment " + std::to_string(i) + " differ (internal error)");
        if (out_f64) out_f64[i] = sums[i].x;
        if (out_f32) out_f32[i] = (float)sums[i].x;
    }
    return RL_OK;
}

int rl_debug_membench(int32_t device, int32_t mode, int64_t bytes, int32_t stride, int32_t iters, double *avg_ms, double *alg_bytes)
{
    if (!avg_ms || bytes < 4096 || iters < 1 || mode < 0 || mode > 9 || (mode == 3 && stride < 1)) return fail(RL_ERR_INVALID, "bad argument");
    RL_HIP(hipSetDevice(device));
    if (mode >= 4) {
        // LDS atomics (k_mb_lds_atomic): `bytes` = atomics per thread (rounded to 16), `stride` unused; alg_bytes returns the 64-bit atomics of one launch
        hipDeviceProp_t prop;
        RL_HIP(hipGetDeviceProperties(&prop, device));
        const int reps = (int)std::max<int64_t>(1, bytes / 16);
        const unsigned gridl = (unsigned)prop.multiProcessorCount * 3u;
        unsigned long long *sinkl = nullptr;
        RL_HIP(hipMalloc((void **)&sinkl, gridl * sizeof(unsigned long long)));
        struct G2 { unsigned long long *p; ~G2() { (void)hipFree(p); } } g2{sinkl};
        hipEvent_t e0, e1;
        RL_HIP(hipEventCreate(&e0)); RL_HIP(hipEventCreate(&e1));
        const size_t ldsb = (size_t)16 * kHistLdsStride * 12;
        for (int it = -1; it < iters; it++) {
            if (it == 0) RL_HIP(hipEventRecord(e0, nullptr));
            hipLaunchKernelGGL(k_mb_lds_atomic, dim3(gridl), dim3(kThreads), ldsb, nullptr, mode - 4, reps, sinkl);
        }
        RL_HIP(hipEventRecord(e1, nullptr));
        RL_HIP(hipEventSynchronize(e1));
        RL_HIP(hipGetLastError());
        float ms = 0;
        RL_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        *avg_ms = (double)ms / iters;
        if (alg_bytes) *alg_bytes = (double)gridl * kThreads * (double)reps * 16.0;
        return RL_OK;
    }
    const size_t n16 = (size_t)bytes / 16;
    uint4 *a = nullptr, *b = nullptr; int *idx = nullptr; unsigned *sink = nullptr;
    struct Guard { void **p[4]; ~Guard() { for (auto q : p) if (*q) (void)hipFree(*q); } } guard{{(void **)&a, (void **)&b, (void **)&idx, (void **)&sink}};
    hipStream_t s = nullptr;
    RL_HIP(hipMalloc((void **)&a, n16 * 16));
    RL_HIP(hipMemset(a, 1, n16 * 16));
    if (mode == 0) { RL_HIP(hipMalloc((void **)&b, n16 * 16)); RL_HIP(hipMemset(b, 0, n16 * 16)); }
    const unsigned grid = 256 * 16;
    RL_HIP(hipMalloc((void **)&sink, grid * sizeof(unsigned)));
    size_t n_idx = 0;
    if (mode == 3) {
        n_idx = (n16 / 2) / (size_t)stride;
        if (n_idx == 0) return fail(RL_ERR_INVALID, "buffer too small for this stride");
        RL_HIP(hipMalloc((void **)&idx, n_idx * sizeof(int)));
        hipLaunchKernelGGL(k_mb_fill_idx, dim3(1024), dim3(kThreads), 0, s, idx, n_idx, stride, stride);
    }
    hipEvent_t e0, e1;
    RL_HIP(hipEventCreate(&e0)); RL_HIP(hipEventCreate(&e1));
    double bytes_per = 0;
    for (int it = -1; it < iters; it++) {       // it == -1: warm-up
        if (it == 0) RL_HIP(hipEventRecord(e0, s));
        switch (mode) {
        case 0: hipLaunchKernelGGL(k_mb_copy, dim3(grid), dim3(kThreads), 0, s, (const uint4 *)a, b, n16); bytes_per = 2.0 * n16 * 16; break;
        case 1: hipLaunchKernelGGL(k_mb_read, dim3(grid), dim3(kThreads), 0, s, (const uint4 *)a, n16, sink); bytes_per = 1.0 * n16 * 16; break;
        case 2: hipLaunchKernelGGL(k_mb_write, dim3(grid), dim3(kThreads), 0, s, a, n16); bytes_per = 1.0 * n16 * 16; break;
        default: hipLaunchKernelGGL(k_mb_gather32, dim3(grid), dim3(kThreads), 0, s, (const uint4 *)a, (const int *)idx, n_idx, sink); bytes_per = 36.0 * n_idx; break;
        }
    }
    RL_HIP(hipEventRecord(e1, s));
    RL_HIP(hipEventSynchronize(e1));
    RL_HIP(hipGetLastError());
    float ms = 0;
    RL_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_ms = (double)ms / iters;
    if (alg_bytes) *alg_bytes = bytes_per;
    return RL_OK;
}