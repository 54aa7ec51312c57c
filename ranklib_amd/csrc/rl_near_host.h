// rl_near_host.h -- the host side of the leaf-space neighbour search (rl_near.inc): the shape of k_near_match's tiles, the
// 64-bit key that orders references, how a call is cut into query chunks, reference bands and splits, and the argument checks of
// rl_model_predict_neighbours.  Plain C++, no device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "rl_leaves_host.h"

namespace rl {

constexpr int kNearThreads = 256;                  // four wavefronts: a 16 x 16 grid of lanes over the (query, reference) tile
constexpr int kNearMQ = 4, kNearMR = 8;            // a lane's register tile: 4 queries x 8 references, 32 packed counters
constexpr int kNearQT = 16 * kNearMQ;              // queries of a block (_native.NEAR_QUERY_TILE)
constexpr int kNearRT = 16 * kNearMR;              // references of one step of its sweep (_native.NEAR_REF_TILE)
constexpr int kNearTC = 64;                        // trees staged at a time (_native.NEAR_TREE_CHUNK): 32 words of two leaf numbers each
constexpr int kNearCW = kNearTC / 2;
// words of a staged row: the chunk and four more, so that the 16 rows a wavefront's 128-bit reads touch start 4 banks apart
constexpr int kNearRowW = kNearCW + 4;
constexpr int kNearCntRow = kNearRT + 2;           // u16 of a row of the tile's counts in LDS: 65 words, the owners' reads fall into different banks
constexpr int kNearMaxK = 64;                      // RL_NEAR_MAX_K
constexpr int kNearMaxSplits = 63;                 // lists one wavefront of k_near_merge merges beside the running one
constexpr int kNearBlocks = 1024;                  // blocks a launch aims at: four a CU (_native.NEAR_BLOCKS; tests/test_neighbours_cpu.py holds the four mirrors to these)
constexpr int kNearMaxTrees = 65535;               // a 16-bit half of a packed counter counts every other tree of the window
static_assert(kNearQT * kNearCntRow * 2 <= (kNearQT + kNearRT) * kNearRowW * 4, "the tile's counts take the place of the staged leaf numbers");
static_assert(kNearCW % 4 == 0 && kNearThreads == 256, "128-bit LDS reads; tid = 16 * (query lane) + (reference lane)");

// References are ordered by shared descending, then index ascending: the larger key is the better neighbour.  No reference has key 0
// (index < 2^31), which marks an empty slot: index -1, shared 0.
inline uint64_t near_key(uint32_t shared, uint32_t index) { return ((uint64_t)shared << 32) | (uint32_t)~index; }
inline int32_t near_key_index(uint64_t key) { return key ? (int32_t)~(uint32_t)key : -1; }
inline int32_t near_key_shared(uint64_t key) { return (int32_t)(key >> 32); }

// u16 of a row of leaf numbers as the match reads it: a multiple of 4, so a row starts on 8 bytes (the walk's 64-bit stores, the
// staging's 64-bit loads)
inline int64_t near_ld(int32_t n_trees) { return ((int64_t)n_trees + 3) & ~(int64_t)3; }

// dynamic LDS of k_near_match: the staged chunk (the tile's counts afterwards) and the block's lists
inline size_t near_lds(int k) { return (size_t)(kNearQT + kNearRT) * kNearRowW * 4 + (size_t)kNearQT * k * 8; }

struct NearPlan {
    int64_t q_chunk = 0, r_band = 0;               // rows of a query chunk (whole query tiles unless it is all) and of a reference band (whole reference tiles unless it is all)
    int64_t part_rows = 0;                         // (splits x queries) of the largest launch: the lists of the partial results
};

// ref tiles -> (tiles per split, splits): enough blocks to fill the chip when the queries are few, every split with at least one tile
inline int64_t near_split_cap(int64_t q_tiles, int64_t r_tiles)      // never falls as r_tiles grows
{
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kNearMaxSplits, r_tiles), (kNearBlocks + q_tiles - 1) / q_tiles));
}
inline void near_splits(int64_t q_tiles, int64_t r_tiles, int64_t *per, int64_t *splits)
{
    const int64_t s = near_split_cap(q_tiles, r_tiles);
    *per = (r_tiles + s - 1) / s;
    *splits = (r_tiles + *per - 1) / *per;
}

// A quarter of the budget to the query chunk, the rest to the reference band; bytes_per_row: a row and its leaf numbers.
inline NearPlan near_plan(int64_t nq, int64_t nr, int64_t bytes_per_row, int64_t scratch_bytes)
{
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : ((int64_t)256 << 20);
    NearPlan p;
    p.q_chunk = std::min<int64_t>(nq, std::max<int64_t>(kNearQT, (budget / 4 / bytes_per_row) / kNearQT * kNearQT));
    const int64_t left = budget - std::min<int64_t>(budget / 4, p.q_chunk * bytes_per_row);
    p.r_band = std::min<int64_t>(nr, std::max<int64_t>(kNearRT, (left / bytes_per_row) / kNearRT * kNearRT));
    const int64_t last = nq % p.q_chunk;                                       // the call's last chunk may have fewer query tiles and so more splits
    for (int64_t nqc : {p.q_chunk, last ? last : p.q_chunk})                   // (no band has more splits than the cap of the longest)
        p.part_rows = std::max(p.part_rows, near_split_cap((nqc + kNearQT - 1) / kNearQT, (p.r_band + kNearRT - 1) / kNearRT) * nqc);
    return p;
}

// The checks of rl_model_predict_neighbours that need no device, in the header's order; n_model_trees < 0: a null model.  *n_trees == 0
// becomes "through the last tree".  0, or the status (-1 invalid, -4 unsupported: RL_ERR_*) and the message.
inline int near_check(const std::string &w, int64_t n_model_trees, const void *Xq, int64_t nq, const void *Xr, int64_t nr, int32_t row_stride,
                      int32_t first_tree, int32_t *n_trees, int32_t k, int32_t flags, int64_t scratch_bytes, const void *out_index,
                      const void *out_shared, std::string &err)
{
    if (!Xq) { err = w + "null Xq"; return -1; }
    if (!Xr) { err = w + "null Xr"; return -1; }
    if (!out_index) { err = w + "null out_index"; return -1; }
    if (!out_shared) { err = w + "null out_shared"; return -1; }
    if (nq < 1) { err = w + "nq must be >= 1"; return -1; }
    if (nr < 1) { err = w + "nr must be >= 1"; return -1; }
    if (row_stride < 1) { err = w + "row_stride must be >= 1"; return -1; }
    if (k < 1 || k > kNearMaxK) { err = w + "k = " + std::to_string(k) + " is outside [1, " + std::to_string(kNearMaxK) + "]"; return -1; }
    if (flags & ~1) { err = w + "unknown flags " + std::to_string(flags & ~1); return -1; }
    if (scratch_bytes < 0) { err = w + "scratch_bytes must be >= 0"; return -1; }
    std::string lerr;                                                          // first_tree, n_trees, the model and the window: leaves_check's words
    const int rc = leaves_check(w, n_model_trees, Xq, 0, row_stride, first_tree, n_trees, 0, out_index, lerr);
    if (rc) { err = lerr; return rc; }
    if (nq > (int64_t)INT32_MAX || nr > (int64_t)INT32_MAX) { err = w + "more than 2^31 rows per call"; return -4; }
    if (*n_trees > kNearMaxTrees) { err = w + "a window of " + std::to_string(*n_trees) + " trees: 65535 at most"; return -4; }
    return 0;
}

}  // namespace rl
