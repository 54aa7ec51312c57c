// rl_net.inc -- the forward pass of the neural-net rankers (RankNet -ranker 1, LambdaRank 5, ListNet 7: learning/neuralnet/RankNet.java
// eval :336-349, which the other two inherit) on gfx950; included at the end of rl_ca.hip.  Scoring only: a handle (rl_net) holds one
// loaded network on the device.  Training is not built.
//
// The network (RankNet.java setInputOutput / addHiddenLayer / wire :67-110): layer 0 = the F inputs and a bias neuron of output 1.0,
// layers 1 .. L-1 hidden, layer L one output neuron.  Neuron j of layer l sums its inLinks in order (Neuron.computeOutput :68-76):
//     wsum = 0.0;  wsum += out(l-1, i) * w  for i = 0 .. n_{l-1} - 1;  wsum += 1.0 * w_bias   (wire() connects the bias last)
//     out(l, j) = 1.0 / (1.0 + exp(-wsum))                                                   (LogiFunction.compute :18-20)
// an f64 multiply, then an f64 add (never fused: -ffp-contract=off), then rho_fdlibm(-wsum) of rl_device.h, which is 1.0 / (1 + exp(x)) with
// fdlibm's exp bit for bit.  The weights arrive in that order: for l = 1 .. L a row-major matrix [n_l][n_{l-1} + 1], row j = neuron j's
// inLinks, the bias weight last.
//
//   k_net_forward<NACC>    one document per lane, 256 documents a block.  The whole network lives in LDS, staged once per block: layer 1
//                          transposed to [F + 1][NACC] (the NACC weights of one input are adjacent; columns beyond n_1 repeat the last
//                          neuron and are never stored), the later layers as given.  Every lane reads the same weight at the same time: a
//                          broadcast.  The rows of X are brought in coalesced, 32 inputs of the block's 256 rows at a time, through an LDS
//                          tile of pitch 33 floats (lane d reads bank (d + kk) % 32: no conflict); the feature list's indirection and the
//                          "beyond row_stride reads 0" rule are applied while staging.  A lane carries the n_1 chains of layer 1 as NACC
//                          register accumulators and takes each input once for all of them: those independent chains hide the latency of
//                          a dependent f64 add.  The outputs of a hidden layer go to the lane's own column of an LDS scratch (which
//                          reuses the tile), the later layers run through net_layer.
//   k_net_forward_global   the same arithmetic with the weights read from global memory (uniform addresses), the row read by its lane and
//                          the hidden outputs in a global scratch of the handle: for networks whose first layer is wider than kNetMaxAcc or
//                          that do not fit kNetLdsBytes.  A bounded grid strides over the documents.
//   net_layer              one layer for one lane: kNetJB neurons at a time, each a serial chain in the Java's order.
//
// Why an LDS tile and not wide per-lane loads: a row starts at i * row_stride floats and row_stride is usually F + 1 (column 0 unused), so a
// lane's 16-byte loads would be misaligned on three rows of four, and the feature list is an indirection a lane would resolve per value.

#include "rl_device.h"

namespace rl {

constexpr int kNetChunk = 32;                    // inputs staged per tile
constexpr int kNetPitch = kNetChunk + 1;         // floats per tile row
constexpr int kNetTileDoubles = kThreads * kNetPitch / 2;
constexpr int kNetMaxAcc = 32;                   // widest first layer k_net_forward keeps in registers
constexpr int kNetLdsBytes = 64 * 1024;          // LDS budget of a block: weights + feature list + tile / scratch
constexpr int kNetJB = 4;                        // neurons net_layer carries at a time
constexpr int kNetGlobalBlocks = 256;            // grid bound of k_net_forward_global (sizes the handle's scratch)
static_assert(kThreads % kNetChunk == 0 && (kThreads * kNetPitch) % 2 == 0, "tile geometry");

struct NetArgs {
    const float *X; double *out; int64_t n, stride;
    const int32_t *fid;          // [F] feature ids = columns of X
    const int32_t *dims;         // [L + 1]: F, the hidden sizes, 1
    const double *w;             // the matrices of layers 1 .. L, one after another
    int32_t F, L, nw;
    int32_t off_fid, off_a, off_b;   // k_net_forward: LDS offsets in doubles (feature list, tile / scratch A, scratch B)
    int32_t maxw;                // widest hidden layer
    double *scratch;             // k_net_forward_global: [2][maxw][lanes]
};

// LogiFunction.compute of N sums: 1.0 / (1.0 + exp(-wsum)), up to four interleaved rho chains at a time
template <int N>
__device__ __forceinline__ void net_logistic(const double (&s)[N], double (&r)[N])
{
    constexpr int G = N % 4 == 0 ? 4 : N % 2 == 0 ? 2 : 1;
#pragma unroll
    for (int g = 0; g < N; g += G) {
        double x[G], y[G];
#pragma unroll
        for (int u = 0; u < G; u++) x[u] = -s[g + u];
        rho_fdlibm_n<G>(x, y);
#pragma unroll
        for (int u = 0; u < G; u++) r[g + u] = y[u];
    }
}

// Layer of nl neurons over np sources and the bias, for one document: W = [nl][np + 1], in(i) = the output of source i, put(j, v) takes
// neuron j's output.  Rows beyond nl repeat the last neuron (their result is dropped).
template <class In, class Put>
__device__ __forceinline__ void net_layer(const double *W, int np, int nl, In in, Put put)
{
    for (int j0 = 0; j0 < nl; j0 += kNetJB) {
        const double *row[kNetJB];
        double s[kNetJB], r[kNetJB];
#pragma unroll
        for (int u = 0; u < kNetJB; u++) { row[u] = W + (size_t)min(j0 + u, nl - 1) * (np + 1); s[u] = 0.0; }
        for (int i = 0; i < np; i++) {
            const double a = in(i);
#pragma unroll
            for (int u = 0; u < kNetJB; u++) s[u] += a * row[u][i];
        }
#pragma unroll
        for (int u = 0; u < kNetJB; u++) s[u] += 1.0 * row[u][np];
        net_logistic<kNetJB>(s, r);
#pragma unroll
        for (int u = 0; u < kNetJB; u++)
            if (j0 + u < nl) put(j0 + u, r[u]);
    }
}

template <int NACC>
__global__ __launch_bounds__(kThreads) void k_net_forward(const NetArgs a)
{
    extern __shared__ double s_net[];
    constexpr int ROWS = kThreads / kNetChunk, PER = kNetChunk;      // a thread stages input kk of rows dd, dd + 8, ...: 32 loads
    const int F = a.F, L = a.L, tid = threadIdx.x;
    const int n1 = a.dims[1], nwd = a.nw - n1 * (F + 1);
    double *w1t = s_net;                                             // [F + 1][NACC]
    double *wd = w1t + (size_t)(F + 1) * NACC;                       // layers 2 .. L as given
    int32_t *s_fid = (int32_t *)(s_net + a.off_fid);
    float *tile = (float *)(s_net + a.off_a);                        // [256][kNetPitch]
    double *act_a = s_net + a.off_a, *act_b = s_net + a.off_b;       // [maxw][256] each; A reuses the tile
    for (int e = tid; e < (F + 1) * NACC; e += kThreads) {
        const int k = e / NACC, u = e - k * NACC;
        w1t[e] = a.w[(size_t)min(u, n1 - 1) * (F + 1) + k];
    }
    for (int e = tid; e < nwd; e += kThreads) wd[e] = a.w[(size_t)n1 * (F + 1) + e];
    for (int e = tid; e < F; e += kThreads) s_fid[e] = a.fid[e];
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * kThreads, doc = base + tid;
    const int kk = tid % kNetChunk, dd = tid / kNetChunk;
    double acc[NACC];
#pragma unroll
    for (int u = 0; u < NACC; u++) acc[u] = 0.0;
    for (int k0 = 0; k0 < F; k0 += kNetChunk) {
        // no range check around a load: what is out of range reads element 0 and becomes 0 afterwards, so all 32 loads are in flight
        const int c = k0 + kk < F ? s_fid[k0 + kk] : -1;
        const bool cin = c >= 0 && c < a.stride;
        float v[PER];
#pragma unroll
        for (int t = 0; t < PER; t++) {
            const int64_t i = base + dd + t * ROWS;
            v[t] = a.X[cin && i < a.n ? i * a.stride + c : (int64_t)0];
        }
        if (k0) __syncthreads();                                     // the previous chunk has been consumed
#pragma unroll
        for (int t = 0; t < PER; t++) tile[(dd + t * ROWS) * kNetPitch + kk] = cin && base + dd + t * ROWS < a.n ? v[t] : 0.f;
        __syncthreads();
        const int kc = min(kNetChunk, F - k0);
        const float *xr = tile + tid * kNetPitch;
        const double *wr = w1t + (size_t)k0 * NACC;
#pragma unroll 4
        for (int q = 0; q < kc; q++) {
            const double x = (double)xr[q];
#pragma unroll
            for (int u = 0; u < NACC; u++) acc[u] += x * wr[q * NACC + u];
        }
    }
#pragma unroll
    for (int u = 0; u < NACC; u++) acc[u] += 1.0 * w1t[(size_t)F * NACC + u];
    double r[NACC];
    net_logistic<NACC>(acc, r);
    if (L == 1) {                                                    // no hidden layer: layer 1 is the output neuron
        if (doc < a.n) a.out[doc] = r[0];
        return;
    }
    __syncthreads();                                                 // the tile is scratch A from here on
#pragma unroll
    for (int u = 0; u < NACC; u++)
        if (u < n1) act_a[u * kThreads + tid] = r[u];
    double *in = act_a, *ob = act_b;                                 // a lane reads and writes its own column only: no barrier
    const double *W = wd;
    for (int l = 2; l <= L; l++) {
        const int np = a.dims[l - 1], nl = a.dims[l];
        net_layer(W, np, nl, [&](int i) { return in[i * kThreads + tid]; },
                  [&](int j, double val) {
                      if (l < L) ob[j * kThreads + tid] = val;
                      else if (doc < a.n) a.out[doc] = val;
                  });
        W += (size_t)nl * (np + 1);
        double *t = in; in = ob; ob = t;
    }
}

__global__ __launch_bounds__(kThreads) void k_net_forward_global(const NetArgs a)
{
    const int64_t lanes = (int64_t)gridDim.x * kThreads, lane = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double *act_a = a.scratch + lane, *act_b = act_a + (size_t)a.maxw * lanes;      // element j of a lane: [j * lanes]
    for (int64_t doc = lane; doc < a.n; doc += lanes) {
        const float *row = a.X + doc * a.stride;
        const double *W = a.w;
        double *in = act_b, *ob = act_a;
        for (int l = 1; l <= a.L; l++) {
            const int np = a.dims[l - 1], nl = a.dims[l];
            auto put = [&](int j, double val) {
                if (l < a.L) ob[(size_t)j * lanes] = val;
                else a.out[doc] = val;
            };
            if (l == 1)
                net_layer(W, np, nl, [&](int k) { const int c = a.fid[k]; return (double)(c >= 0 && c < a.stride ? row[c] : 0.f); }, put);
            else
                net_layer(W, np, nl, [&](int i) { return in[(size_t)i * lanes]; }, put);
            W += (size_t)nl * (np + 1);
            double *t = in; in = ob; ob = t;
        }
    }
}

}  // namespace rl

struct rl_net {
    int32_t device = 0, F = 0, L = 0, nw = 0, maxw = 0;
    int32_t nacc = 0;                  // k_net_forward's instantiation; 0: k_net_forward_global
    int32_t off_fid = 0, off_a = 0, off_b = 0; size_t lds_bytes = 0;
    rl::DevPool buf;
    int32_t *d_fid = nullptr, *d_dims = nullptr; double *d_w = nullptr, *d_scratch = nullptr;
    int32_t last_path = RL_NET_PATH_NONE;
};

namespace rl {

// the instantiations of k_net_forward: the smallest one that holds n_1 is taken (RankNet's default is 10 hidden neurons; 1: no hidden layer)
#define RL_NET_ACCS(X) X(1) X(2) X(4) X(6) X(8) X(10) X(12) X(16) X(24) X(32)

static int net_pick_acc(int n1)
{
#define X(N) if (n1 <= N) return N;
    RL_NET_ACCS(X)
#undef X
    return 0;
}

// decides the variant and lays out k_net_forward's LDS
static void net_plan(rl_net *h, const std::vector<int32_t> &dims)
{
    const int F = h->F, L = h->L, n1 = dims[1];
    h->nacc = net_pick_acc(n1);
    if (!h->nacc) return;
    int64_t off = (int64_t)(F + 1) * h->nacc + (h->nw - (int64_t)n1 * (F + 1));
    h->off_fid = (int32_t)off; off += (F + 1) / 2;
    h->off_a = (int32_t)off; off += std::max<int64_t>(kNetTileDoubles, L > 1 ? (int64_t)h->maxw * kThreads : 0);
    h->off_b = (int32_t)off; off += L > 2 ? (int64_t)h->maxw * kThreads : 0;
    if (off * (int64_t)sizeof(double) > kNetLdsBytes) { h->nacc = 0; return; }
    h->lds_bytes = (size_t)off * sizeof(double);
}

}  // namespace rl

extern "C" {

int rl_net_create(int32_t device, const int32_t *feature_ids, int32_t n_features, const int32_t *hidden_sizes, int32_t n_hidden,
                  const double *weights, int32_t n_weights, rl_net **out)
{
    if (!out) return fail(RL_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!feature_ids || !weights || (n_hidden > 0 && !hidden_sizes)) return fail(RL_ERR_INVALID, "null argument");
    if (n_features < 1) return fail(RL_ERR_INVALID, "a network needs at least one input feature");
    if (n_hidden < 0) return fail(RL_ERR_INVALID, "negative number of hidden layers");
    std::vector<int32_t> dims;
    dims.push_back(n_features);
    int64_t need = 0; int32_t maxw = 0;
    for (int32_t l = 0; l < n_hidden; l++) {
        if (hidden_sizes[l] < 1) return fail(RL_ERR_INVALID, "hidden layer " + std::to_string(l + 1) + " has no neuron");
        dims.push_back(hidden_sizes[l]);
        maxw = std::max(maxw, hidden_sizes[l]);
    }
    dims.push_back(1);
    for (size_t l = 1; l < dims.size(); l++) need += (int64_t)dims[l] * ((int64_t)dims[l - 1] + 1);
    if (need != (int64_t)n_weights)
        return fail(RL_ERR_INVALID, "n_weights is " + std::to_string(n_weights) + ", the network has " + std::to_string(need) +
                                    " (for every layer n_l * (n_{l-1} + 1))");
    const int gate = open_device(device, true);
    if (gate) return gate;
    std::unique_ptr<rl_net> h(new rl_net());
    h->device = device; h->F = n_features; h->L = n_hidden + 1; h->nw = n_weights; h->maxw = maxw;
    net_plan(h.get(), dims);
    RL_HIP(h->buf.alloc(&h->d_fid, (size_t)n_features));
    RL_HIP(h->buf.alloc(&h->d_dims, dims.size()));
    RL_HIP(h->buf.alloc(&h->d_w, (size_t)n_weights));
    RL_HIP(hipMemcpy(h->d_fid, feature_ids, (size_t)n_features * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->d_dims, dims.data(), dims.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->d_w, weights, (size_t)n_weights * sizeof(double), hipMemcpyHostToDevice));
    if (!h->nacc) RL_HIP(h->buf.alloc(&h->d_scratch, (size_t)2 * maxw * kNetGlobalBlocks * kThreads));
    *out = h.release();
    return RL_OK;
}

void rl_net_destroy(rl_net *net)
{
    if (!net) return;
    (void)hipSetDevice(net->device);
    delete net;                        // hipFree waits for the device
}

int rl_net_predict_device(rl_net *net, const float *dX, int64_t n_docs, int32_t row_stride, double *dOut, void *stream)
{
    if (!net) return fail(RL_ERR_INVALID, "null handle");
    if (n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad sizes");
    if (n_docs >= (int64_t)2147483647 * kThreads) return fail(RL_ERR_UNSUPPORTED, "too many documents for one launch");
    if (n_docs == 0) return RL_OK;
    if (!dX || !dOut) return fail(RL_ERR_INVALID, "null argument");
    RL_HIP(hipSetDevice(net->device));
    NetArgs a;
    a.X = dX; a.out = dOut; a.n = n_docs; a.stride = row_stride;
    a.fid = net->d_fid; a.dims = net->d_dims; a.w = net->d_w;
    a.F = net->F; a.L = net->L; a.nw = net->nw;
    a.off_fid = net->off_fid; a.off_a = net->off_a; a.off_b = net->off_b;
    a.maxw = net->maxw; a.scratch = net->d_scratch;
    const int64_t blocks = (n_docs + kThreads - 1) / kThreads;
    hipStream_t s = (hipStream_t)stream;
    switch (net->nacc) {
#define X(N) case N: hipLaunchKernelGGL(k_net_forward<N>, dim3((unsigned)blocks), dim3(kThreads), net->lds_bytes, s, a); break;
        RL_NET_ACCS(X)
#undef X
    default:
        hipLaunchKernelGGL(k_net_forward_global, dim3((unsigned)std::min<int64_t>(blocks, kNetGlobalBlocks)), dim3(kThreads), 0, s, a);
    }
    RL_HIP(hipGetLastError());
    net->last_path = net->nacc ? RL_NET_PATH_LDS : RL_NET_PATH_GLOBAL;
    return RL_OK;
}

int rl_net_predict(rl_net *net, const float *X, int64_t n_docs, int32_t row_stride, double *out)
{
    if (!net) return fail(RL_ERR_INVALID, "null handle");
    if (n_docs < 0 || row_stride < 1) return fail(RL_ERR_INVALID, "bad sizes");
    if (n_docs == 0) return RL_OK;
    if (!X || !out) return fail(RL_ERR_INVALID, "null argument");
    RL_HIP(hipSetDevice(net->device));
    DevPool buf;
    float *dX = nullptr; double *dO = nullptr;
    RL_HIP(buf.alloc(&dX, (size_t)n_docs * row_stride));
    RL_HIP(buf.alloc(&dO, (size_t)n_docs));
    RL_HIP(hipMemcpy(dX, X, (size_t)n_docs * row_stride * sizeof(float), hipMemcpyHostToDevice));
    int rc = rl_net_predict_device(net, dX, n_docs, row_stride, dO, nullptr);
    if (rc) return rc;
    RL_HIP(hipMemcpy(out, dO, (size_t)n_docs * sizeof(double), hipMemcpyDeviceToHost));
    return RL_OK;
}

int rl_net_debug_path(const rl_net *net, int32_t *path)
{
    if (!net || !path) return fail(RL_ERR_INVALID, "null argument");
    *path = net->last_path;
    return RL_OK;
}

}  // extern "C"
