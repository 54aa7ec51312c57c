// rl_ale_host.h -- the host side of accumulated local effects (rl_ale.inc): the argument checks and the integer
// bookkeeping of a call -- the columns cut into chunks, a chunk into batches of up to B consecutive columns, and uses[batch][tree], a
// bit per column of the batch, exact.  Plain C++, no device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "rl_partial_host.h"

namespace rl {

constexpr int kAleMaxEdges = 256;                            // of one column: RL_ALE_MAX_INTERVALS + 1 (rl_ale.inc asserts it)

// what rl_model_predict_ale checks before it looks at the model, so a machine without a device reaches every one of them
inline int ale_check(const std::string &w, const void *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                     const int32_t *edge_off, const float *edges, int64_t scratch_bytes, const void *out_count, const void *out_sum,
                     std::string &err)
{
    if (!X) { err = w + "null X"; return RLP_INVALID; }
    if (!columns) { err = w + "null columns"; return RLP_INVALID; }
    if (!edge_off) { err = w + "null edge_off"; return RLP_INVALID; }
    if (!edges) { err = w + "null edges"; return RLP_INVALID; }
    if (!out_count) { err = w + "null out_count"; return RLP_INVALID; }
    if (!out_sum) { err = w + "null out_sum"; return RLP_INVALID; }
    if (n_docs < 1) { err = w + "n_docs must be >= 1"; return RLP_INVALID; }
    if (n_docs > (int64_t)INT32_MAX) { err = w + "more than 2^31 documents per call"; return RLP_UNSUPPORTED; }
    if (row_stride < 1) { err = w + "row_stride must be >= 1"; return RLP_INVALID; }
    if (n_columns < 1) { err = w + "n_columns must be >= 1"; return RLP_INVALID; }
    for (int32_t c = 0; c < n_columns; c++)
        if (columns[c] < 0) { err = w + "columns[" + std::to_string(c) + "] = " + std::to_string(columns[c]) + " is negative"; return RLP_INVALID; }
    if (edge_off[0] != 0) { err = w + "edge_off[0] = " + std::to_string(edge_off[0]) + " must be 0"; return RLP_INVALID; }
    for (int32_t c = 0; c < n_columns; c++) {
        const int64_t ne = (int64_t)edge_off[c + 1] - (int64_t)edge_off[c];
        if (ne < 2 || ne > kAleMaxEdges) {
            err = w + "edge_off[" + std::to_string(c + 1) + "] - edge_off[" + std::to_string(c) + "] = " + std::to_string(ne) +
                  ": a column has 2 .. " + std::to_string(kAleMaxEdges) + " edges";
            return RLP_INVALID;
        }
    }
    for (int32_t c = 0; c < n_columns; c++)
        for (int32_t j = edge_off[c]; j < edge_off[c + 1]; j++) {
            const std::string at = "edges[" + std::to_string(c) + "][" + std::to_string(j - edge_off[c]) + "] = " + partial_float(edges[j]);
            if (edges[j] != edges[j]) { err = w + at + " is NaN"; return RLP_INVALID; }
            if (j > edge_off[c] && !(edges[j - 1] < edges[j])) {
                err = w + at + " is not greater than its predecessor " + partial_float(edges[j - 1]) + ": a column's edges ascend strictly";
                return RLP_INVALID;
            }
        }
    if (scratch_bytes < 0) { err = w + "scratch_bytes must be >= 0"; return RLP_INVALID; }
    return RLP_OK;
}

// The device scratch of a chunk is 12 bytes per document and column (lo, hi, interval), plus the base: the columns a chunk holds,
// at least one and at most max_chunk (a launch's gridDim.y: every column may be a batch of its own)
inline int32_t ale_chunk_columns(int64_t scratch_bytes, int64_t default_bytes, int64_t n_docs, int32_t n_columns, int32_t max_chunk)
{
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : default_bytes;
    const int64_t fit = (budget - n_docs * (int64_t)sizeof(float)) / (n_docs * 12);
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_columns, max_chunk), fit));
}

// Chunk ci holds the columns [ci * chunk, min(C, ci * chunk + chunk)); its batch j the up to B columns from ci * chunk + j * B on.
struct AlePlan {
    int32_t n_columns = 0, chunk = 1, B = 1, n_trees = 0;
    std::vector<int32_t> first;             // [chunks + 1] the chunks' first batches
    std::vector<uint32_t> uses;             // [batches][n_trees]: bit u set where a node of the tree tests the batch's column u
    int32_t chunks() const { return (int32_t)first.size() - 1; }
    int32_t col0(int32_t ci) const { return ci * chunk; }
    int32_t col1(int32_t ci) const { return std::min<int64_t>(n_columns, (int64_t)ci * chunk + chunk); }
};

inline AlePlan ale_plan(const std::vector<HostTree> &trees, const int32_t *columns, int32_t n_columns, int32_t chunk, int32_t B)
{
    AlePlan p;
    p.n_columns = n_columns; p.chunk = std::max<int32_t>(1, chunk); p.B = B; p.n_trees = (int32_t)trees.size();
    const size_t T = trees.size();
    std::map<int32_t, std::vector<int32_t>> trees_of;      // column -> the trees that test it, ascending, each once
    for (int32_t t = 0; t < p.n_trees; t++)
        for (int32_t f : trees[(size_t)t].feature)
            if (f != -1) { auto &v = trees_of[f]; if (v.empty() || v.back() != t) v.push_back(t); }
    int32_t nb = 0;
    for (int32_t c0 = 0; c0 < n_columns; c0 += p.chunk) {
        p.first.push_back(nb);
        const int32_t c1 = std::min<int64_t>(n_columns, (int64_t)c0 + p.chunk);
        for (int32_t b0 = c0; b0 < c1; b0 += B, nb++) {
            p.uses.resize(p.uses.size() + T, 0u);
            for (int32_t u = 0; u < B && b0 + u < c1; u++) {
                auto it = trees_of.find(columns[b0 + u]);
                if (it != trees_of.end())
                    for (int32_t t : it->second) p.uses[(size_t)nb * T + (size_t)t] |= 1u << u;
            }
        }
    }
    p.first.push_back(nb);
    return p;
}

}  // namespace rl
