// rl_partial_host.h -- the host side of partial dependence (rl_partial.inc): the argument checks and the integer
// bookkeeping of a call -- the cells cut into chunks, a chunk into batches that never straddle a column (the last batch of a column in a
// chunk is padded; a chunk ends early before it would cut a batch), and uses[batch][tree], exact per column.  Plain C++, no device: it
// is also compiled into tools/partial_host_check.cpp, a stand-alone program that runs under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "rl_model.h"

namespace rl {

constexpr int RLP_OK = 0, RLP_INVALID = -1, RLP_UNSUPPORTED = -4;      // RL_OK, RL_ERR_INVALID, RL_ERR_UNSUPPORTED

inline std::string partial_float(float v)
{
    char buf[32];
    snprintf(buf, sizeof buf, "%.9g", (double)v);
    return buf;
}

// what rl_model_predict_partial checks before it looks at the model, so a machine without a device reaches every one of them
inline int partial_check(const std::string &w, const void *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                         const int32_t *grid_off, const float *grid, int64_t scratch_bytes, const void *out_mean, const void *out_shift2,
                         std::string &err)
{
    if (!X) { err = w + "null X"; return RLP_INVALID; }
    if (!columns) { err = w + "null columns"; return RLP_INVALID; }
    if (!grid_off) { err = w + "null grid_off"; return RLP_INVALID; }
    if (!grid) { err = w + "null grid"; return RLP_INVALID; }
    if (!out_mean) { err = w + "null out_mean"; return RLP_INVALID; }
    if (!out_shift2) { err = w + "null out_shift2"; return RLP_INVALID; }
    if (n_docs < 1) { err = w + "n_docs must be >= 1"; return RLP_INVALID; }
    if (n_docs > (int64_t)INT32_MAX) { err = w + "more than 2^31 documents per call"; return RLP_UNSUPPORTED; }
    if (row_stride < 1) { err = w + "row_stride must be >= 1"; return RLP_INVALID; }
    if (n_columns < 1) { err = w + "n_columns must be >= 1"; return RLP_INVALID; }
    for (int32_t c = 0; c < n_columns; c++)
        if (columns[c] < 0) { err = w + "columns[" + std::to_string(c) + "] = " + std::to_string(columns[c]) + " is negative"; return RLP_INVALID; }
    if (grid_off[0] != 0) { err = w + "grid_off[0] = " + std::to_string(grid_off[0]) + " must be 0"; return RLP_INVALID; }
    for (int32_t c = 0; c < n_columns; c++)
        if (grid_off[c + 1] <= grid_off[c]) {
            err = w + "grid_off[" + std::to_string(c + 1) + "] = " + std::to_string(grid_off[c + 1]) + " is not greater than grid_off[" +
                  std::to_string(c) + "] = " + std::to_string(grid_off[c]) + ": a column's grid is empty or grid_off descends";
            return RLP_INVALID;
        }
    for (int32_t c = 0; c < n_columns; c++)
        for (int32_t j = grid_off[c]; j < grid_off[c + 1]; j++) {
            const std::string at = "grid[" + std::to_string(c) + "][" + std::to_string(j - grid_off[c]) + "] = " + partial_float(grid[j]);
            if (grid[j] != grid[j]) { err = w + at + " is NaN"; return RLP_INVALID; }
            if (j > grid_off[c] && !(grid[j - 1] < grid[j])) {
                err = w + at + " is not greater than its predecessor " + partial_float(grid[j - 1]) + ": a column's grid ascends strictly";
                return RLP_INVALID;
            }
        }
    if (scratch_bytes < 0) { err = w + "scratch_bytes must be >= 0"; return RLP_INVALID; }
    if (grid_off[n_columns] >= INT32_MAX - 1) { err = w + "more than 2^31 cells per call"; return RLP_UNSUPPORTED; }      // (the base is one more)
    return RLP_OK;
}

// The device scratch of a chunk is 4 bytes per document and cell, plus the base: what is left for the cells of `budget` bytes
inline int64_t partial_cell_budget(int64_t scratch_bytes, int64_t default_bytes, int64_t n_docs)
{
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : default_bytes;
    return std::max<int64_t>(1, budget - n_docs * (int64_t)sizeof(float));
}

// A batch: `cnt` (1 .. B) consecutive cells of ONE column, rows cell0 .. cell0 + cnt - 1 of the chunk's scores.  The base is the first
// batch of the first chunk: column -1, place -1, one cell that goes to the base buffer instead.
struct PartialBatch { int32_t col, cell0, cnt, place; };      // place: the column's index in columns[]

struct PartialPlan {
    int32_t n_cells = 0, chunk = 1, B = 1, n_trees = 0;
    std::vector<int32_t> first;             // [chunks + 1] the chunks' first batches
    std::vector<int32_t> cell0;             // [chunks + 1] the chunks' first cells: a chunk holds at most `chunk` cells
    std::vector<PartialBatch> batches;
    std::vector<float> values;              // [batches][B]: the cells' grid values; the slots past cnt repeat the last one (never stored)
    std::vector<uint8_t> uses;              // [batches][n_trees]: 1 where a node of the tree tests the batch's column
    int32_t chunks() const { return (int32_t)first.size() - 1; }
    int32_t cells_of(int32_t ci) const { return cell0[(size_t)ci + 1] - cell0[(size_t)ci]; }
};

inline PartialPlan partial_plan(const std::vector<HostTree> &trees, const int32_t *columns, int32_t n_columns, const int32_t *grid_off,
                                const float *grid, int32_t chunk, int32_t B)
{
    PartialPlan p;
    p.n_cells = grid_off[n_columns]; p.chunk = std::max<int32_t>(1, chunk); p.B = B; p.n_trees = (int32_t)trees.size();
    const size_t T = trees.size();
    std::map<int32_t, std::vector<int32_t>> trees_of;      // column -> the trees that test it, ascending, each once
    for (int32_t t = 0; t < p.n_trees; t++)
        for (int32_t f : trees[(size_t)t].feature)
            if (f != -1) { auto &v = trees_of[f]; if (v.empty() || v.back() != t) v.push_back(t); }
    auto add = [&](int32_t col, int32_t cell0, int32_t cnt, int32_t place, const float *vals) {
        p.batches.push_back({col, cell0, cnt, place});
        for (int32_t u = 0; u < B; u++) p.values.push_back(vals ? vals[std::min(u, cnt - 1)] : 0.f);
        p.uses.resize(p.uses.size() + T, 0);
        auto it = trees_of.find(col);
        if (it != trees_of.end())
            for (int32_t t : it->second) p.uses[p.uses.size() - T + (size_t)t] = 1;
    };
    // A chunk ends where the next batch -- up to B cells, as many as its column has left -- would not fit whole, so that a cut costs no
    // batch (a batch is a whole walk); only a batch larger than a whole chunk is cut.
    int32_t j = 0, c = 0;                                  // the cell at hand and its column
    while (j < p.n_cells) {
        p.first.push_back((int32_t)p.batches.size());
        p.cell0.push_back(j);
        if (j == 0) add(-1, 0, 1, -1, nullptr);
        int32_t used = 0;
        while (j < p.n_cells) {
            while (grid_off[c + 1] <= j) c++;
            const int32_t want = std::min<int32_t>(B, grid_off[c + 1] - j), left = p.chunk - used;
            if (left == 0 || (want > left && used > 0 && want <= p.chunk)) break;
            const int32_t cnt = std::min(want, left);
            add(columns[c], used, cnt, c, grid + j);
            j += cnt; used += cnt;
        }
    }
    p.cell0.push_back(p.n_cells);
    p.first.push_back((int32_t)p.batches.size());
    return p;
}

}  // namespace rl
