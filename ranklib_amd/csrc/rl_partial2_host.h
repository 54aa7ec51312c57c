// rl_partial2_host.h -- the host side of two-feature partial dependence (rl_partial2.inc): the argument checks and the
// integer bookkeeping of a call -- every pair's ga x gb cells cut into tiles of up to TA x TB cells that never straddle a pair (an edge
// tile is padded by repeating its last value on either axis), the tiles packed into chunks that hold whole tiles (a chunk ends early
// before a tile it cannot hold; only where a whole chunk is smaller than TA x TB cells are the tiles cut smaller, to fit one), and
// uses[tile][tree], exact per pair: 1 where a node of the tree tests either column.  Plain C++, no device: it is also compiled into
// tools/partial2_host_check.cpp, a stand-alone program that runs under the host sanitizers.
//
// The kernel's pending stack (rl_partial2.inc) holds two 32-bit words per entry: the node id as int32 (so trees of up to 2^31 - 1 nodes)
// and the index rectangle u0 | u1 << 8 | v0 << 16 | v1 << 24 (so tiles of up to 255 x 255 cells).
#pragma once
#include "rl_partial_host.h"

namespace rl {

constexpr int kPartial2MaxSide = 255;                         // what the rectangle's packing allows

// what rl_model_predict_partial2 checks before it looks at the model; the grids are the 2 n_pairs CSR slices of `grid`
inline int partial2_check(const std::string &w, const void *X, int64_t n_docs, int32_t row_stride, const int32_t *pairs, int32_t n_pairs,
                          const int32_t *grid_off, const float *grid, int64_t scratch_bytes, const void *out_mean, const void *out_shift2,
                          std::string &err)
{
    if (!X) { err = w + "null X"; return RLP_INVALID; }
    if (!pairs) { err = w + "null pairs"; return RLP_INVALID; }
    if (!grid_off) { err = w + "null grid_off"; return RLP_INVALID; }
    if (!grid) { err = w + "null grid"; return RLP_INVALID; }
    if (!out_mean) { err = w + "null out_mean"; return RLP_INVALID; }
    if (!out_shift2) { err = w + "null out_shift2"; return RLP_INVALID; }
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
    const int32_t n_grids = 2 * n_pairs;
    if (grid_off[0] != 0) { err = w + "grid_off[0] = " + std::to_string(grid_off[0]) + " must be 0"; return RLP_INVALID; }
    for (int32_t c = 0; c < n_grids; c++)
        if (grid_off[c + 1] <= grid_off[c]) {
            err = w + "grid_off[" + std::to_string(c + 1) + "] = " + std::to_string(grid_off[c + 1]) + " is not greater than grid_off[" +
                  std::to_string(c) + "] = " + std::to_string(grid_off[c]) + ": a grid is empty or grid_off descends";
            return RLP_INVALID;
        }
    for (int32_t c = 0; c < n_grids; c++)
        for (int32_t j = grid_off[c]; j < grid_off[c + 1]; j++) {
            const std::string at = "grid[" + std::to_string(c) + "][" + std::to_string(j - grid_off[c]) + "] = " + partial_float(grid[j]);
            if (grid[j] != grid[j]) { err = w + at + " is NaN"; return RLP_INVALID; }
            if (j > grid_off[c] && !(grid[j - 1] < grid[j])) {
                err = w + at + " is not greater than its predecessor " + partial_float(grid[j - 1]) + ": a grid ascends strictly";
                return RLP_INVALID;
            }
        }
    if (scratch_bytes < 0) { err = w + "scratch_bytes must be >= 0"; return RLP_INVALID; }
    int64_t cells = 0;
    for (int32_t p = 0; p < n_pairs; p++) {
        cells += (int64_t)(grid_off[2 * p + 1] - grid_off[2 * p]) * (int64_t)(grid_off[2 * p + 2] - grid_off[2 * p + 1]);
        if (cells >= (int64_t)INT32_MAX - 1) { err = w + "more than 2^31 cells per call"; return RLP_UNSUPPORTED; }
    }
    return RLP_OK;
}

// A tile: cnt_a x cnt_b cells of ONE pair, the values u0 .. u0 + cnt_a - 1 of column col_a's grid and v0 .. of col_b's.  Its scores are
// the rows slot0 + uu * cnt_b + vv of the chunk's scores (only the cells that exist take a slot); the call's cell of slot (uu, vv) is
// cell + uu * gb + vv.  The base is tile 0, outside every chunk: columns -1, one cell that goes to the base buffer instead.
struct Partial2Tile { int32_t col_a, col_b, slot0, cnt_a, cnt_b, cell, gb, pair; };

struct Partial2Plan {
    int32_t n_cells = 0, chunk = 1, TA = 1, TB = 1, n_trees = 0;
    std::vector<int32_t> cell_off;          // [pairs + 1] the running sum of ga * gb
    std::vector<int32_t> first;             // [chunks + 1] the chunks' first tiles (the first chunk's is 1)
    std::vector<int32_t> slots;             // [chunks] the cells a chunk holds: at most `chunk`
    std::vector<Partial2Tile> tiles;
    std::vector<float> values;              // [tiles][TA + TB]: TA values of a, then TB of b; the slots past cnt repeat the last one
    std::vector<uint8_t> uses;              // [tiles][n_trees]
    int32_t chunks() const { return (int32_t)first.size() - 1; }
};

inline Partial2Plan partial2_plan(const std::vector<HostTree> &trees, const int32_t *pairs, int32_t n_pairs, const int32_t *grid_off,
                                  const float *grid, int32_t chunk, int32_t TA, int32_t TB)
{
    Partial2Plan p;
    p.chunk = std::max<int32_t>(1, chunk); p.TA = TA; p.TB = TB; p.n_trees = (int32_t)trees.size();
    const size_t T = trees.size();
    std::map<int32_t, std::vector<int32_t>> trees_of;      // column -> the trees that test it, ascending, each once
    for (int32_t t = 0; t < p.n_trees; t++)
        for (int32_t f : trees[(size_t)t].feature)
            if (f != -1) { auto &v = trees_of[f]; if (v.empty() || v.back() != t) v.push_back(t); }
    auto add = [&](Partial2Tile td, const float *ga, const float *gb) {
        p.tiles.push_back(td);
        for (int32_t u = 0; u < TA; u++) p.values.push_back(ga ? ga[std::min(u, td.cnt_a - 1)] : 0.f);
        for (int32_t v = 0; v < TB; v++) p.values.push_back(gb ? gb[std::min(v, td.cnt_b - 1)] : 0.f);
        p.uses.resize(p.uses.size() + T, 0);
        for (int32_t col : {td.col_a, td.col_b}) {
            auto it = trees_of.find(col);
            if (it != trees_of.end())
                for (int32_t t : it->second) p.uses[p.uses.size() - T + (size_t)t] = 1;
        }
    };
    add({-1, -1, 0, 1, 1, -1, 1, -1}, nullptr, nullptr);
    // the sides a tile may have: TA x TB, cut down only where a whole chunk holds fewer cells than that
    const int32_t sb = std::min(TB, p.chunk), sa = std::max<int32_t>(1, std::min(TA, p.chunk / sb));
    p.cell_off.push_back(0);
    int32_t used = p.chunk;                                 // (so that the first tile opens the first chunk)
    for (int32_t q = 0; q < n_pairs; q++) {
        const float *ga = grid + grid_off[2 * q], *gb = grid + grid_off[2 * q + 1];
        const int32_t na = grid_off[2 * q + 1] - grid_off[2 * q], nb = grid_off[2 * q + 2] - grid_off[2 * q + 1], c0 = p.cell_off.back();
        for (int32_t u0 = 0; u0 < na; u0 += sa)
            for (int32_t v0 = 0; v0 < nb; v0 += sb) {
                const int32_t ca = std::min(sa, na - u0), cb = std::min(sb, nb - v0);
                if (used + ca * cb > p.chunk) {             // a chunk ends before a tile it cannot hold
                    p.first.push_back((int32_t)p.tiles.size());
                    p.slots.push_back(0);
                    used = 0;
                }
                add({pairs[2 * q], pairs[2 * q + 1], used, ca, cb, c0 + u0 * nb + v0, nb, q}, ga + u0, gb + v0);
                used += ca * cb;
                p.slots.back() = used;
            }
        p.cell_off.push_back(c0 + na * nb);
    }
    p.n_cells = p.cell_off.back();
    p.first.push_back((int32_t)p.tiles.size());
    return p;
}

}  // namespace rl
