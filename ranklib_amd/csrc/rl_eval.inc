// rl_eval.inc -- test-time evaluation: rank every list of a file by its scores and take each list's metric, one pass on gfx950.
// DESIGN.md 19.  Included by rl_ca.hip's unit (it shares ca_pow2m1 and ca_sync); k_ca_trials is not touched.
//
//   k_eval_lists<G, CAP>  a group of G threads owns one list.  Its scores go into LDS (CAP > 0) or stay in global memory (CAP == 0), every
//                         document counts its position p = #{j : s[j] > s[i] or (s[j] == s[i] and j < i)} -- stable and descending,
//                         MergeSorter.sort(double[], false); -0.0 == 0.0 is a tie, +-Infinity are ordinary values, NaN never arrives
//                         (eval_prepare refuses it) -- writes its label to slot p of the ranked labels and, when asked, p itself.  Then
//                         the group's first lane takes the metric as the Java's serial f64 chain over the ranked labels, the scorers of
//                         ranklib_amd/metric.py statement for statement (ev_metric).  Length classes, this kernel's own:
//                           <= kEvTiny  (16)    G = 16, 16 lists per block
//                           <= kEvWave  (256)   one wavefront per list, 4 lists per block
//                           <= kEvBlock (6144)  one block per list: 6144 x (8 B score + 4 B label) = 72 KiB of LDS, two blocks per CU
//                           longer              one block per list, scores read from global memory, ranked labels in global scratch
//                         Nothing is summed on the device: MetricScorer.score(List) and Evaluator.test add the lists' values serially on
//                         the host.
//
// The host half (rl_eval_host.h: validation, ideal DCGs) is plain C++.  Built with -ffp-contract=off like the rest.  No CPU fallback.
#include "rl_eval_host.h"
#include "rl_eval_dev.h"

namespace rl {

// kEvTiny / kEvWave / kEvBlock, EvArgs and ev_metric (the scorers): rl_eval_dev.h, shared with k_stage_eval (rl_stage.inc)

// one list by one group of G threads; s_sc / s_lab: the group's LDS (CAP > 0 entries each)
template <int G, int CAP>
__device__ void ev_group(const EvArgs &a, int slot, int tid, double *s_sc, float *s_lab)
{
    const int q = a.qlist[slot];
    const int cur = a.qoff[q], n = a.qoff[q + 1] - cur;
    const double *sc = a.sc + cur;
    float *lab = s_lab;
    if (CAP > 0) {
        for (int i = tid; i < n; i += G) s_sc[i] = sc[i];
        ca_sync<G>();
        sc = s_sc;
    } else {
        lab = a.glab + cur;
    }
    for (int i = tid; i < n; i += G) {
        const double v = sc[i];
        int p = 0;
        for (int j = 0; j < n; j++) { const double y = sc[j]; p += ((y > v) || (y == v && j < i)) ? 1 : 0; }
        lab[p] = a.labels[cur + i];
        if (a.pos) a.pos[cur + i] = p;
    }
    ca_sync<G>();
    if (tid == 0) a.out[q] = ev_metric(a, q, n, lab);
}

template <int G, int CAP>
__global__ __launch_bounds__(kThreads) void k_eval_lists(const EvArgs a)
{
    constexpr int GPB = kThreads / G;                 // groups per block
    constexpr int LDS = CAP > 0 ? CAP : 1;
    __shared__ double s_sc[GPB * LDS];
    __shared__ float s_lab[GPB * LDS];
    const int grp = threadIdx.x / G, tid = threadIdx.x % G;
    const int64_t g = (int64_t)blockIdx.x * GPB + grp;
    if (g < (int64_t)a.nq) ev_group<G, CAP>(a, (int)g, tid, s_sc + grp * LDS, s_lab + grp * LDS);   // G == kThreads: the whole block or none
}

static thread_local double g_ev_kernel_ms = 0.0;     // the last rl_eval_lists call of this thread: its launches between two device events

}  // namespace rl

extern "C" {

int rl_eval_lists(int32_t device, int32_t metric, int32_t k, double err_max, const double *scores, const float *labels, int64_t n_docs,
                  const int32_t *qoff, int32_t n_lists, const int32_t *qkey, const double *ideal_dcg, const int32_t *rel_doc_count,
                  double *out_metric, int32_t *out_pos, double *out_ideal)
{
    std::vector<double> ideal, disc;
    std::string err;
    int rc = eval_prepare(metric, k, err_max, scores, labels, n_docs, qoff, n_lists, qkey, ideal_dcg, rel_doc_count, out_metric, ideal, disc,
                          err);
    if (rc) return fail(rc, err);
    if ((rc = open_device(device, true))) return rc;
    std::vector<int32_t> lists[4];
    for (int32_t q = 0; q < n_lists; q++) {
        const int n = qoff[q + 1] - qoff[q];
        lists[n <= kEvTiny ? 0 : n <= kEvWave ? 1 : n <= kEvBlock ? 2 : 3].push_back(q);
    }
    DevPool buf;
    EvArgs a;
    memset(&a, 0, sizeof(a));
    double *d_sc = nullptr, *d_ideal = nullptr, *d_disc = nullptr, *d_out = nullptr; float *d_lab = nullptr;
    int32_t *d_qoff = nullptr, *d_rd = nullptr, *d_pos = nullptr, *d_qlist[4] = {nullptr, nullptr, nullptr, nullptr};
    RL_HIP(buf.alloc(&d_sc, (size_t)n_docs));
    RL_HIP(buf.alloc(&d_lab, (size_t)n_docs));
    RL_HIP(buf.alloc(&d_qoff, (size_t)n_lists + 1));
    RL_HIP(buf.alloc(&d_ideal, (size_t)n_lists));
    RL_HIP(buf.alloc(&d_disc, disc.size()));
    RL_HIP(buf.alloc(&d_out, (size_t)n_lists));
    RL_HIP(hipMemcpy(d_sc, scores, (size_t)n_docs * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_lab, labels, (size_t)n_docs * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_qoff, qoff, ((size_t)n_lists + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_ideal, ideal.data(), (size_t)n_lists * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_disc, disc.data(), disc.size() * sizeof(double), hipMemcpyHostToDevice));
    if (rel_doc_count) {
        RL_HIP(buf.alloc(&d_rd, (size_t)n_lists));
        RL_HIP(hipMemcpy(d_rd, rel_doc_count, (size_t)n_lists * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (out_pos) RL_HIP(buf.alloc(&d_pos, (size_t)n_docs));
    if (!lists[3].empty()) RL_HIP(buf.alloc(&a.glab, (size_t)n_docs));
    for (int c = 0; c < 4; c++) {
        if (lists[c].empty()) continue;
        RL_HIP(buf.alloc(&d_qlist[c], lists[c].size()));
        RL_HIP(hipMemcpy(d_qlist[c], lists[c].data(), lists[c].size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    a.sc = d_sc; a.labels = d_lab; a.qoff = d_qoff; a.ideal = d_ideal; a.rd_ext = d_rd; a.disc = d_disc; a.out = d_out; a.pos = d_pos;
    a.metric = metric; a.k = k; a.err_max = err_max;
    static const int G[4] = {kEvTiny, kWave, kThreads, kThreads};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } guard{e0, e1};
    RL_HIP(hipEventCreate(&e0));
    RL_HIP(hipEventCreate(&e1));
    RL_HIP(hipEventRecord(e0, 0));
    for (int c = 0; c < 4; c++) {
        if (lists[c].empty()) continue;
        a.qlist = d_qlist[c]; a.nq = (int32_t)lists[c].size();
        const int gpb = kThreads / G[c];
        const dim3 grid((unsigned)((a.nq + gpb - 1) / gpb)), block(kThreads);
        if (c == 0) hipLaunchKernelGGL((k_eval_lists<kEvTiny, kEvTiny>), grid, block, 0, 0, a);
        else if (c == 1) hipLaunchKernelGGL((k_eval_lists<kWave, kEvWave>), grid, block, 0, 0, a);
        else if (c == 2) hipLaunchKernelGGL((k_eval_lists<kThreads, kEvBlock>), grid, block, 0, 0, a);
        else hipLaunchKernelGGL((k_eval_lists<kThreads, 0>), grid, block, 0, 0, a);
        RL_HIP(hipGetLastError());
    }
    RL_HIP(hipEventRecord(e1, 0));
    RL_HIP(hipMemcpy(out_metric, d_out, (size_t)n_lists * sizeof(double), hipMemcpyDeviceToHost));
    if (out_pos) RL_HIP(hipMemcpy(out_pos, d_pos, (size_t)n_docs * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_ideal) std::copy(ideal.begin(), ideal.end(), out_ideal);
    float ms = 0.f;
    RL_HIP(hipEventElapsedTime(&ms, e0, e1));
    g_ev_kernel_ms = (double)ms;
    return RL_OK;
}

int rl_debug_eval_times(double *kernel_ms)
{
    if (!kernel_ms) return fail(RL_ERR_INVALID, "rl_debug_eval_times: null argument");
    *kernel_ms = g_ev_kernel_ms;
    return RL_OK;
}

}  // extern "C"
