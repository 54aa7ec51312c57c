// rl_norm.inc -- feature normalisation (-norm sum | zscore | linear) of every ranked list of a file in one pass on gfx950.  DESIGN.md 20.
// Included by rl_ca.hip's unit.  Built with -ffp-contract=off like the rest.  No CPU fallback.
//
//   k_normalize_lists   one lane owns one (list, requested column) pair and walks the list's documents in order, as the Java's loops over
//                       rl.get(i) do (features/SumNormalizor.java, ZScoreNormalizor.java, LinearNormalizer.java): two passes for sum and
//                       linear, three for zscore.  The f64 sums are the Java's serial chains -- never split, reordered or reduced over
//                       lanes; only the loads of the next documents are issued ahead (nm_walk).  The pairs are numbered list-major,
//                       pair = list * n_cols + j, and lane t of the grid owns pair t: neighbouring lanes read neighbouring requested
//                       columns of one row, and with 136 columns no lane idles -- a wavefront that straddles two lists reads two row
//                       segments a step and runs to the longer list.  A list of any length is walked; nothing is staged in LDS.  `times`
//                       applications run back to back inside the lane: a column of a list is read and written by its own lane only.
//
// Three operations must be correctly rounded: the f64 and f32 divisions (hipcc's IEEE expansions) and the f64 square root, which
// nm_sqrt corrects with an exact fma residual whatever the expansion gives.
namespace rl {

struct NmArgs {
    float *X; const int32_t *qoff; const int32_t *cols;
    int64_t n_pairs;                                           // n_lists * n_cols
    int32_t n_cols, stride, kind, times;
};

__device__ __forceinline__ float nm_val(float v) { return v != v ? 0.0f : v; }   // DataPoint.getFeatureValue: NaN (unknown) reads as 0

// Math.min / Math.max (float): -0.0f orders below +0.0f.  a is the running value (never NaN here), b a cell as nm_val reads it
__device__ __forceinline__ float nm_java_min(float a, float b)
{
    if (a == 0.0f && b == 0.0f && (__float_as_uint(b) >> 31)) return b;
    return (a <= b) ? a : b;
}
__device__ __forceinline__ float nm_java_max(float a, float b)
{
    if (a == 0.0f && b == 0.0f && (__float_as_uint(a) >> 31)) return b;
    return (a >= b) ? a : b;
}

// Math.sqrt: the correctly rounded root.  The device expansion's result c is moved by at most two steps either way while the exact
// residual r = x - c * c (one fma) says the neighbour is nearer: with u the gap to the next double, sqrt(x) lies above the midpoint
// c + u / 2 exactly when r > c * u (x, c * c and c * u are whole multiples of u * u, the midpoint's square is not), and below the
// midpoint c - u' / 2 exactly when r <= -c * u'.  0, Infinity and NaN need nothing.
__device__ double nm_sqrt(double x)
{
    double c = sqrt(x);
    if (!(x > 0.0) || !(x < HUGE_VAL) || !(c > 0.0)) return c;
    for (int it = 0; it < 2; it++) {
        const double up = __longlong_as_double(__double_as_longlong(c) + 1);
        if (fma(-c, c, x) > c * (up - c)) c = up; else break;
    }
    for (int it = 0; it < 2; it++) {
        const double dn = __longlong_as_double(__double_as_longlong(c) - 1);
        if (fma(-c, c, x) <= -(c * (c - dn))) c = dn; else break;
    }
    return c;
}

// f(value) for the n documents of a column in order; the loads of four documents are issued before the first is used
template <class F>
__device__ __forceinline__ void nm_walk(const float *p, int n, int64_t stride, F f)
{
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const float a = p[0], b = p[stride], c = p[2 * stride], d = p[3 * stride];
        p += 4 * stride;
        f(nm_val(a)); f(nm_val(b)); f(nm_val(c)); f(nm_val(d));
    }
    for (; i < n; i++) { f(nm_val(*p)); p += stride; }
}

// p[i] = g(value) for the n documents of a column
template <class G>
__device__ __forceinline__ void nm_write(float *p, int n, int64_t stride, G g)
{
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const float a = p[0], b = p[stride], c = p[2 * stride], d = p[3 * stride];
        p[0] = g(nm_val(a)); p[stride] = g(nm_val(b)); p[2 * stride] = g(nm_val(c)); p[3 * stride] = g(nm_val(d));
        p += 4 * stride;
    }
    for (; i < n; i++) { *p = g(nm_val(*p)); p += stride; }
}

__global__ __launch_bounds__(kThreads) void k_normalize_lists(const NmArgs a)
{
    const int64_t pair = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (pair >= a.n_pairs) return;
    const int q = (int)(pair / a.n_cols), j = (int)(pair % a.n_cols);
    const int row0 = a.qoff[q], n = a.qoff[q + 1] - row0;
    const int64_t stride = a.stride;
    float *p = a.X + ((int64_t)row0 * stride + a.cols[j]);      // 64-bit: 40 M rows x 137 columns is past 2^31 elements
    for (int t = 0; t < a.times; t++) {
        if (a.kind == RL_NORM_SUM) {                            // SumNormalizor.java:55-70
            double norm = 0;
            nm_walk(p, n, stride, [&](float v) { norm += (double)fabsf(v); });
            if (norm > 0) nm_write(p, n, stride, [&](float v) { return (float)((double)v / norm); });
        } else if (a.kind == RL_NORM_ZSCORE) {                  // ZScoreNormalizor.java:66-92
            double mean = 0;
            nm_walk(p, n, stride, [&](float v) { mean += (double)v; });
            mean = mean / n;
            double std = 0;
            nm_walk(p, n, stride, [&](float v) { const double x = (double)v - mean; std += x * x; });
            std = nm_sqrt(std / (n - 1));                       // one document: 0 / 0 = NaN, `std > 0` is false
            if (std > 0.0) nm_write(p, n, stride, [&](float v) { return (float)(((double)v - mean) / std); });
        } else {                                                // LinearNormalizer.java:44-66
            float mn = 3.40282347e+38f, mx = __uint_as_float(1u);   // Float.MAX_VALUE, Float.MIN_VALUE (the smallest positive subnormal)
            nm_walk(p, n, stride, [&](float v) { mn = nm_java_min(mn, v); mx = nm_java_max(mx, v); });
            if (mx > mn) {
                const float span = mx - mn;
                nm_write(p, n, stride, [&](float v) { return (v - mn) / span; });
            } else {
                nm_write(p, n, stride, [&](float) { return 0.0f; });
            }
        }
    }
}

// Everything rl_normalize_lists checks before it looks for a device
static int nm_check(int32_t kind, const float *X, int64_t n_docs, int32_t stride, const int32_t *row_len, const int32_t *qoff, int32_t n_lists,
                    const int32_t *cols, int32_t n_cols, int32_t times, std::string &err)
{
    auto bad = [&](const std::string &m) { err = "rl_normalize_lists: " + m; return (int)RL_ERR_INVALID; };
    if (!X || !qoff || !cols) return bad("null argument");
    if (kind < RL_NORM_SUM || kind > RL_NORM_LINEAR) return bad("unknown normaliser " + std::to_string(kind));
    if (n_docs < 1 || n_lists < 1 || n_cols < 1 || times < 1) return bad("n_docs, n_lists, n_cols and times must be >= 1");
    if (stride < 2) return bad("stride must be >= 2 (column 0 is never a feature)");
    if (const int rc = check_lists("rl_normalize_lists", nullptr, n_docs, qoff, n_lists, err)) return rc;      // no labels here: the qoff rules alone
    std::vector<char> seen((size_t)stride, 0);
    int32_t maxcol = 0;
    for (int32_t j = 0; j < n_cols; j++) {
        const int32_t c = cols[j];
        if (c < 1 || c >= stride) return bad("feature id " + std::to_string(c) + " is not a column of a row (1 .. stride - 1)");
        if (seen[(size_t)c]) return bad("duplicate feature id " + std::to_string(c));
        seen[(size_t)c] = 1;
        maxcol = std::max(maxcol, c);
    }
    if (row_len) {
        for (int64_t d = 0; d < n_docs; d++)
            if (row_len[d] < 1 || row_len[d] > stride)
                return bad("row_len of row " + std::to_string(d) + " is " + std::to_string(row_len[d]) + " (1 .. stride)");
        for (int64_t d = 0; d < n_docs; d++) {
            if (row_len[d] > maxcol) continue;
            for (int32_t j = 0; j < n_cols; j++)
                if (cols[j] >= row_len[d])
                    return bad("row " + std::to_string(d) + " does not hold feature " + std::to_string(cols[j]) + " (its row_len is "
                               + std::to_string(row_len[d]) + "): unspecified features are the caller's");
        }
    }
    return RL_OK;
}

static thread_local double g_nm_kernel_ms = 0.0;     // the last rl_normalize_lists call of this thread: its launch between two device events

}  // namespace rl

extern "C" {

int rl_normalize_lists(int32_t device, int32_t kind, float *X, int64_t n_docs, int32_t stride, const int32_t *row_len, const int32_t *qoff,
                       int32_t n_lists, const int32_t *cols, int32_t n_cols, int32_t times)
{
    std::string err;
    int rc = nm_check(kind, X, n_docs, stride, row_len, qoff, n_lists, cols, n_cols, times, err);
    if (rc) return fail(rc, err);
    if ((rc = open_device(device, true))) return rc;
    const int64_t n_pairs = (int64_t)n_lists * n_cols;
    const int64_t n_blocks = (n_pairs + kThreads - 1) / kThreads;
    if (n_blocks > (int64_t)2147483647) return fail(RL_ERR_UNSUPPORTED, "rl_normalize_lists: more than 2^31 blocks of (list, column) pairs");
    const size_t cells = (size_t)n_docs * (size_t)stride;
    DevPool buf;
    NmArgs a;
    memset(&a, 0, sizeof(a));
    int32_t *d_qoff = nullptr, *d_cols = nullptr;
    RL_HIP(buf.alloc(&a.X, cells));
    RL_HIP(buf.alloc(&d_qoff, (size_t)n_lists + 1));
    RL_HIP(buf.alloc(&d_cols, (size_t)n_cols));
    RL_HIP(hipMemcpy(a.X, X, cells * sizeof(float), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_qoff, qoff, ((size_t)n_lists + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d_cols, cols, (size_t)n_cols * sizeof(int32_t), hipMemcpyHostToDevice));
    a.qoff = d_qoff; a.cols = d_cols; a.n_pairs = n_pairs; a.n_cols = n_cols; a.stride = stride; a.kind = kind; a.times = times;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } guard{e0, e1};
    RL_HIP(hipEventCreate(&e0));
    RL_HIP(hipEventCreate(&e1));
    RL_HIP(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_normalize_lists, dim3((unsigned)n_blocks), dim3(kThreads), 0, 0, a);
    RL_HIP(hipGetLastError());
    RL_HIP(hipEventRecord(e1, 0));
    RL_HIP(hipMemcpy(X, a.X, cells * sizeof(float), hipMemcpyDeviceToHost));
    float ms = 0.f;
    RL_HIP(hipEventElapsedTime(&ms, e0, e1));
    g_nm_kernel_ms = (double)ms;
    return RL_OK;
}

int rl_debug_normalize_times(double *kernel_ms)
{
    if (!kernel_ms) return fail(RL_ERR_INVALID, "rl_debug_normalize_times: null argument");
    *kernel_ms = g_nm_kernel_ms;
    return RL_OK;
}

}  // extern "C"
