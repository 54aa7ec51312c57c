// rl_ale2_host.h -- the host side of second-order accumulated local effects (rl_ale2.inc): the argument checks and the
// integer bookkeeping of a call -- the pairs cut into chunks, a chunk into batches of up to P consecutive pairs, and uses[batch][tree],
// two bits per pair of the batch, exact: bit 2u "a node of the tree tests pair u's column a", bit 2u + 1 "... its column b".
// Plain C++, no device.
#pragma once
#include "rl_ale_host.h"

namespace rl {

constexpr int kAle2MaxCells = 4096;                          // of one pair: RL_ALE2_MAX_CELLS (rl_ale2.inc asserts it)
constexpr int kAle2Super = 64;                               // partials of a super-partial: RL_ALE2_SUM_SUPER

// what rl_model_predict_ale2 checks before it looks at the model, so a machine without a device reaches every one of them
inline int ale2_check(const std::string &w, const void *X, int64_t n_docs, int32_t row_stride, const int32_t *pairs, int32_t n_pairs,
                      const int32_t *edge_off, const float *edges, int64_t scratch_bytes, const void *out_count, const void *out_sum,
                      std::string &err)
{
    if (!X) { err = w + "null X"; return RLP_INVALID; }
    if (!pairs) { err = w + "null pairs"; return RLP_INVALID; }
    if (!edge_off) { err = w + "null edge_off"; return RLP_INVALID; }
    if (!edges) { err = w + "null edges"; return RLP_INVALID; }
    if (!out_count) { err = w + "null out_count"; return RLP_INVALID; }
    if (!out_sum) { err = w + "null out_sum"; return RLP_INVALID; }
    if (n_docs < 1) { err = w + "n_docs must be >= 1"; return RLP_INVALID; }
    if (n_docs > (int64_t)INT32_MAX) { err = w + "more than 2^31 documents per call"; return RLP_UNSUPPORTED; }
    if (row_stride < 1) { err = w + "row_stride must be >= 1"; return RLP_INVALID; }
    if (n_pairs < 1) { err = w + "n_pairs must be >= 1"; return RLP_INVALID; }
    if (n_pairs > INT32_MAX / 2 - 1) { err = w + "more than 2^30 pairs per call"; return RLP_UNSUPPORTED; }
    for (int32_t p = 0; p < n_pairs; p++) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        const std::string at = "pairs[" + std::to_string(p) + "] = (" + std::to_string(a) + ", " + std::to_string(b) + ")";
        if (a < 0 || b < 0) { err = w + at + " has a negative column"; return RLP_INVALID; }
        if (a == b) { err = w + at + " names one column twice"; return RLP_INVALID; }
    }
    const int32_t n_slices = 2 * n_pairs;
    if (edge_off[0] != 0) { err = w + "edge_off[0] = " + std::to_string(edge_off[0]) + " must be 0"; return RLP_INVALID; }
    for (int32_t c = 0; c < n_slices; c++) {
        const int64_t ne = (int64_t)edge_off[c + 1] - (int64_t)edge_off[c];
        if (ne < 2 || ne > kAleMaxEdges) {
            err = w + "edge_off[" + std::to_string(c + 1) + "] - edge_off[" + std::to_string(c) + "] = " + std::to_string(ne) +
                  ": a slice has 2 .. " + std::to_string(kAleMaxEdges) + " edges";
            return RLP_INVALID;
        }
    }
    for (int32_t c = 0; c < n_slices; c++)
        for (int32_t j = edge_off[c]; j < edge_off[c + 1]; j++) {
            const std::string at = "edges[" + std::to_string(c) + "][" + std::to_string(j - edge_off[c]) + "] = " + partial_float(edges[j]);
            if (edges[j] != edges[j]) { err = w + at + " is NaN"; return RLP_INVALID; }
            if (j > edge_off[c] && !(edges[j - 1] < edges[j])) {
                err = w + at + " is not greater than its predecessor " + partial_float(edges[j - 1]) + ": a slice's edges ascend strictly";
                return RLP_INVALID;
            }
        }
    int64_t cells = 0;
    for (int32_t p = 0; p < n_pairs; p++) {
        const int32_t ka = edge_off[2 * p + 1] - edge_off[2 * p] - 1, kb = edge_off[2 * p + 2] - edge_off[2 * p + 1] - 1;
        if (ka * kb > kAle2MaxCells) {
            err = w + "pairs[" + std::to_string(p) + "] has " + std::to_string(ka) + " x " + std::to_string(kb) + " = " + std::to_string(ka * kb) +
                  " cells: a pair has at most " + std::to_string(kAle2MaxCells);
            return RLP_INVALID;
        }
        cells += ka * kb;
        if (cells >= (int64_t)INT32_MAX - 1) { err = w + "more than 2^31 cells per call"; return RLP_UNSUPPORTED; }
    }
    if (scratch_bytes < 0) { err = w + "scratch_bytes must be >= 0"; return RLP_INVALID; }
    return RLP_OK;
}

// The device scratch of a chunk is 12 bytes per document and pair (d as f64, the cell), 16 more where the four corners are asked for,
// plus the base: the pairs a chunk holds, at least one and at most max_chunk (a launch's gridDim.y: every pair may be a batch of its own)
inline int32_t ale2_chunk_pairs(int64_t scratch_bytes, int64_t default_bytes, int64_t n_docs, int32_t n_pairs, bool corners, int32_t max_chunk)
{
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : default_bytes;
    const int64_t fit = (budget - n_docs * (int64_t)sizeof(float)) / (n_docs * (corners ? 28 : 12));
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_pairs, max_chunk), fit));
}

// the super-blocks of RL_ALE2_SUM_SUPER * RL_PARTIAL_SUM_BLOCK documents a call's reduction is spread over
inline int32_t ale2_supers(int64_t n_docs, int32_t sum_block) { return (int32_t)((n_docs + (int64_t)kAle2Super * sum_block - 1) / ((int64_t)kAle2Super * sum_block)); }

// Chunk ci holds the pairs [ci * chunk, min(n_pairs, ci * chunk + chunk)); its batch j the up to P pairs from ci * chunk + j * P on.
struct Ale2Plan {
    int32_t n_pairs = 0, chunk = 1, P = 1, n_trees = 0, max_cells = 0;      // max_cells: of the widest chunk, all its pairs together
    std::vector<int32_t> cell_off;          // [pairs + 1] the running sum of Ka * Kb
    std::vector<int32_t> first;             // [chunks + 1] the chunks' first batches
    std::vector<uint32_t> uses;             // [batches][n_trees]
    int32_t chunks() const { return (int32_t)first.size() - 1; }
    int32_t pair0(int32_t ci) const { return ci * chunk; }
    int32_t pair1(int32_t ci) const { return std::min<int64_t>(n_pairs, (int64_t)ci * chunk + chunk); }
};

inline Ale2Plan ale2_plan(const std::vector<HostTree> &trees, const int32_t *pairs, int32_t n_pairs, const int32_t *edge_off, int32_t chunk, int32_t P)
{
    Ale2Plan p;
    p.n_pairs = n_pairs; p.chunk = std::max<int32_t>(1, chunk); p.P = P; p.n_trees = (int32_t)trees.size();
    const size_t T = trees.size();
    std::map<int32_t, std::vector<int32_t>> trees_of;      // column -> the trees that test it, ascending, each once
    for (int32_t t = 0; t < p.n_trees; t++)
        for (int32_t f : trees[(size_t)t].feature)
            if (f != -1) { auto &v = trees_of[f]; if (v.empty() || v.back() != t) v.push_back(t); }
    p.cell_off.push_back(0);
    for (int32_t q = 0; q < n_pairs; q++)
        p.cell_off.push_back(p.cell_off.back() + (edge_off[2 * q + 1] - edge_off[2 * q] - 1) * (edge_off[2 * q + 2] - edge_off[2 * q + 1] - 1));
    int32_t nb = 0;
    for (int32_t c0 = 0; c0 < n_pairs; c0 += p.chunk) {
        p.first.push_back(nb);
        const int32_t c1 = std::min<int64_t>(n_pairs, (int64_t)c0 + p.chunk);
        p.max_cells = std::max(p.max_cells, p.cell_off[(size_t)c1] - p.cell_off[(size_t)c0]);
        for (int32_t b0 = c0; b0 < c1; b0 += P, nb++) {
            p.uses.resize(p.uses.size() + T, 0u);
            for (int32_t u = 0; u < P && b0 + u < c1; u++)
                for (int32_t side = 0; side < 2; side++) {
                    auto it = trees_of.find(pairs[2 * (b0 + u) + side]);
                    if (it != trees_of.end())
                        for (int32_t t : it->second) p.uses[(size_t)nb * T + (size_t)t] |= 1u << (2 * u + side);
                }
        }
    }
    p.first.push_back(nb);
    return p;
}

}  // namespace rl
