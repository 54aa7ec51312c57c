// rl_fast_leaf.inc -- RL_FLAG_FAST_LEAF: the leaves' two sums as a FIXED f64 reduction instead of the Java's float running sums (rl_chain.inc).
//
// The definition is pure arithmetic and does not depend on a grid or a launch shape (DESIGN.md 14; tests/fast_leaf_restatement.py restates it).
// For the values x_0 .. x_{n-1} (f64) of a leaf's samples in ascending order (the leaf's sample list; the identity for a root-only tree):
//
//   B(v), at most 256 values: pad to 256 with +0.0; for s = 128, 64, .., 1: a[i] = a[i] + a[i + s] for all i < s; the result is a[0]
//   R(x): n == 0 -> 0.0; else replace the sequence by [B(x[256 j : 256 j + 256]) for j] until one value is left (n == 1 still passes through
//         one B); finally add +0.0 (an all -0.0 leaf gives +0.0, as the Java's `0F +=` does)
//
// Every add is a plain f64 add (this translation unit is built with -ffp-contract=off and without fast-math; there is no multiply near them).
// LambdaMART: s1 = (float) R(pseudoResponses), s2 = (float) R(weights), output = (s2 == 0) ? 0 : s1 / s2 (learning/tree/LambdaMART.java:409-413);
// MART: output = s1 / (float) count (learning/tree/MART.java:64), as k_leaf_output.
//
// Two launches, both sized by capacities known at rl_init, no device value read back by the host:
//   k_fast_leaf_tiles   level 0: one block per 256-sample tile of every segment, one double2 partial (both sums) per tile
//   k_fast_leaf_finish  one block per segment: the upper levels by the same rule (at most three more: 256^4 > 2^31), then the output
//
// Tile slots.  Segment l = [seg_start[l], seg_start[l + 1]) of the position space [0, n) owns the slots slot0(l) .. slot0(l) + ceil(len / 256) - 1 with
// slot0(l) = seg_start[l] / 256 + l: a closed form of the table k_leaf_table already writes (no scan, no launch of its own).  The ranges do not
// overlap, because ceil((e - s) / 256) <= e / 256 - s / 256 + 1 for integers s <= e, and the last one ends below n / 256 + n_seg + 1.  A slot between
// two ranges is empty: its block exits, nothing reads its partial.

namespace rl {

constexpr int kFastTile = 256;          // values per B() = threads per block of both kernels

struct FastLeafArgs {
    const double2 *pair;                // (lambda, weight) by document
    const int32_t *idx0, *idx1;         // the two ping-pong sample-list buffers
    const int32_t *seg_buf;             // [n_seg] which buffer a segment's list lives in, -1 = the identity; null = the identity for every segment
    const int32_t *seg_start;           // [n_seg + 1] ascending, seg_start[n_seg] = n
    const int32_t *n_seg_dev;           // the segment count on the device (TreeState::n_leaves); null = n_seg
    int32_t n_seg;                      // segments at most (the blocks of k_fast_leaf_finish): every table below has this many entries
    uint16_t *seg_of;                   // optional [by document]: the segment a document sits in (k_score_stream)
    double2 *part;                      // [cap_slots] partial sums
    int32_t cap_slots;                  // >= n / 256 + n_seg + 1
    double2 *sums;                      // [n_seg] out: R of both value arrays
    // the leaves' outputs (null: only `sums` is written)
    NodeRec *nodes;
    const int32_t *leaf_node;           // [n_seg] node of every segment
    int32_t mart;
};

__host__ __device__ __forceinline__ int fast_slot0(int start, int l) { return start / kFastTile + l; }
static int64_t fast_leaf_slots(int64_t n, int64_t max_seg) { return n / kFastTile + max_seg + 2; }

// lane i receives the value of lane i + S of its 16-lane row (S < 16); lanes without a source keep their own value, which no later step reads
template <int S> __device__ __forceinline__ double row_down_f64(double v) { return bits2d(dpp_u64<0x100 + S>(d2bits(v), d2bits(v))); }

// B() of the block's 256 values, v = a[threadIdx.x]; the result is valid in thread 0.  After step s the entries a[0 .. s) are the definition's; the
// other threads go on computing values nobody reads.  Steps 128 and 64 go through LDS, the steps inside wavefront 0 through ds_bpermute (32, 16:
// they cross the 16-lane rows) and DPP row shifts (8 .. 1).
__device__ __forceinline__ double2 fast_block_B(double2 v, double2 *sh /* [128] */)
{
    const int i = threadIdx.x;
    if (i >= 128) sh[i - 128] = v;
    __syncthreads();
    if (i < 128) { const double2 o = sh[i]; v.x = v.x + o.x; v.y = v.y + o.y; }
    __syncthreads();
    if (i >= 64 && i < 128) sh[i - 64] = v;
    __syncthreads();
    if (i >= 64) return v;          // (whole wavefronts)
    { const double2 o = sh[i]; v.x = v.x + o.x; v.y = v.y + o.y; }
    v.x = v.x + __shfl_down(v.x, 32); v.y = v.y + __shfl_down(v.y, 32);
    v.x = v.x + __shfl_down(v.x, 16); v.y = v.y + __shfl_down(v.y, 16);
    v.x = v.x + row_down_f64<8>(v.x); v.y = v.y + row_down_f64<8>(v.y);
    v.x = v.x + row_down_f64<4>(v.x); v.y = v.y + row_down_f64<4>(v.y);
    v.x = v.x + row_down_f64<2>(v.x); v.y = v.y + row_down_f64<2>(v.y);
    v.x = v.x + row_down_f64<1>(v.x); v.y = v.y + row_down_f64<1>(v.y);
    return v;
}

// Level 0.  Index bounds: slot = blockIdx.x < cap_slots (the grid IS cap_slots; the guard keeps a larger grid harmless); the segment l < n_seg is
// the last one with slot0(l) <= slot, j = slot - slot0(l) its tile; a tile at or beyond the segment's end is an empty slot.  Position
// base + p0 + i is read only under i < len - p0, so it stays below seg_start[l + 1] <= n, the length of idx0 / idx1; the document ids in the lists
// are below n, the length of pair / seg_of.  One partial is written, at part[slot].
__global__ __launch_bounds__(kFastTile) void k_fast_leaf_tiles(const FastLeafArgs a)
{
    __shared__ double2 sh[128];
    const int slot = blockIdx.x;
    if (slot >= a.cap_slots) return;
    const int ns = a.n_seg_dev ? min(*a.n_seg_dev, a.n_seg) : a.n_seg;
    if (ns <= 0) return;
    int lo = 0, hi = ns - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (fast_slot0(a.seg_start[mid], mid) <= slot) lo = mid; else hi = mid - 1; }
    const int l = lo;
    const int base = a.seg_start[l], len = a.seg_start[l + 1] - base;
    const int j = slot - fast_slot0(base, l);
    if (j < 0 || (long long)j * kFastTile >= len) return;
    const int p0 = j * kFastTile, i = p0 + (int)threadIdx.x;
    const int sb = a.seg_buf ? a.seg_buf[l] : -1;
    const int32_t *idx = sb < 0 ? nullptr : (sb == 0 ? a.idx0 : a.idx1);
    double2 v = make_double2(0.0, 0.0);
    if (i < len) {
        const int doc = idx ? idx[base + i] : base + i;
        v = a.pair[doc];
        if (a.seg_of) a.seg_of[doc] = (uint16_t)l;
    }
    v = fast_block_B(v, sh);
    if (threadIdx.x == 0) a.part[slot] = v;
}

// Upper levels and the output.  Index bounds: l = blockIdx.x < n_seg (the device count, at most the table size the grid was sized by); the
// segment's partials are part[s0 .. s0 + cnt) with s0 = slot0(l) and cnt = ceil(len / 256) at level 1, so s0 + cnt <= cap_slots as for level 0;
// group g of a level reads part[s0 + 256 g + i] under 256 g + i < cnt and writes part[s0 + g], g <= 256 g: in place, behind a barrier, never
// ahead of a group still to be read.  sums[l], leaf_node[l] and nodes[leaf_node[l]] are the tables of k_leaf_table.
__global__ __launch_bounds__(kFastTile) void k_fast_leaf_finish(const FastLeafArgs a)
{
    __shared__ double2 sh[128];
    const int l = blockIdx.x;
    const int ns = a.n_seg_dev ? min(*a.n_seg_dev, a.n_seg) : a.n_seg;
    if (l >= ns) return;
    const int base = a.seg_start[l], len = a.seg_start[l + 1] - base;
    double2 *part = a.part + fast_slot0(base, l);
    int cnt = (int)(((long long)len + kFastTile - 1) / kFastTile);
    while (cnt > 1) {
        const int groups = (cnt + kFastTile - 1) / kFastTile;
        for (int g = 0; g < groups; g++) {
            const int i = g * kFastTile + (int)threadIdx.x;
            double2 v = make_double2(0.0, 0.0);
            if (i < cnt) v = part[i];
            v = fast_block_B(v, sh);
            __syncthreads();            // every read of the group is done (part[g] may be one of its inputs)
            if (threadIdx.x == 0) part[g] = v;
        }
        __threadfence_block();
        __syncthreads();                // the level's results are visible to the block
        cnt = groups;
    }
    if (threadIdx.x != 0) return;
    double2 r = make_double2(0.0, 0.0);
    if (len > 0) r = part[0];
    r.x = r.x + 0.0; r.y = r.y + 0.0;
    a.sums[l] = r;
    if (!a.nodes) return;
    const float s1 = (float)r.x, s2 = (float)r.y;
    NodeRec &X = a.nodes[a.leaf_node[l]];
    if (a.mart) X.output = s1 / (float)X.gcount;                  // MART.updateTreeOutput (MART.java:54-65)
    else X.output = (s2 == 0.f) ? 0.f : s1 / s2;                  // LambdaMART.java:409-413
}

}  // namespace rl
