// rl_contrib_host.h -- the host side of per-document feature contributions (rl_contrib.inc): the argument checks, the
// inner nodes' covers from the leaves', the node values from the covers and the slot of every node.  Plain C++, no device: it is also
// compiled into tools/contrib_host_check.cpp, a stand-alone program that runs under the host sanitizers.
// Built with -ffp-contract=off like the rest: the node value is two products, one sum and one quotient, each rounded.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "rl_model.h"

namespace rl {

constexpr int RLC_OK = 0, RLC_INVALID = -1, RLC_STATE = -3, RLC_UNSUPPORTED = -4;      // RL_OK, RL_ERR_INVALID, RL_ERR_STATE, RL_ERR_UNSUPPORTED

// what rl_model_cover and rl_model_predict_contribs check before the device is touched (n_trees < 0: a null model)
inline int contrib_check_rows(const std::string &w, int64_t n_trees, const void *X, int64_t n_docs, int32_t row_stride, std::string &err)
{
    if (n_trees < 0) { err = w + "null model"; return RLC_INVALID; }
    if (!X) { err = w + "null X"; return RLC_INVALID; }
    if (n_docs < 0) { err = w + "n_docs must be >= 0"; return RLC_INVALID; }
    if (n_docs > (int64_t)INT32_MAX) { err = w + "more than 2^31 documents per call"; return RLC_UNSUPPORTED; }
    if (row_stride < 1) { err = w + "row_stride must be >= 1"; return RLC_INVALID; }
    if (n_trees < 1) { err = w + "the model has no trees"; return RLC_INVALID; }
    return RLC_OK;
}

inline int contrib_check_columns(const std::string &w, const int32_t *columns, int32_t n_columns, int64_t scratch_bytes, const void *out,
                                 std::string &err)
{
    if (!out) { err = w + "null output"; return RLC_INVALID; }
    if (n_columns < 0) { err = w + "n_columns must be >= 0"; return RLC_INVALID; }
    if (columns && n_columns < 1) { err = w + "n_columns must be >= 1 with columns given"; return RLC_INVALID; }
    if (scratch_bytes < 0) { err = w + "scratch_bytes must be >= 0"; return RLC_INVALID; }
    if (columns) {
        for (int32_t c = 0; c < n_columns; c++)
            if (columns[c] < 0) { err = w + "columns[" + std::to_string(c) + "] = " + std::to_string(columns[c]) + " is negative"; return RLC_INVALID; }
        std::vector<std::pair<int32_t, int32_t>> s((size_t)n_columns);
        for (int32_t c = 0; c < n_columns; c++) s[(size_t)c] = {columns[c], c};
        std::sort(s.begin(), s.end());
        for (size_t i = 1; i < s.size(); i++)
            if (s[i].first == s[i - 1].first) {
                err = w + "columns[" + std::to_string(s[i].second) + "] = " + std::to_string(s[i].first) + " is listed twice";
                return RLC_INVALID;
            }
    }
    return RLC_OK;
}

// cover [n_nodes] holds the leaves' counts; the inner nodes become c[l] + c[r].  The nodes are in the pre-order of the model text, a
// parent before its children, so one pass from the last node to the first has both children ready.
inline void contrib_fill_inner(const HostTree &t, uint64_t *cover)
{
    for (int j = t.n_nodes - 1; j >= 0; j--)
        if (t.feature[(size_t)j] != -1) cover[j] = cover[t.left[(size_t)j]] + cover[t.right[(size_t)j]];
}

// val [n_nodes], children first: a leaf's is (double)out; a split's the cover-weighted mean of its children's, both weights 1 where the
// background never reached the node
inline void contrib_node_values(const HostTree &t, const uint64_t *cover, double *val)
{
    for (int j = t.n_nodes - 1; j >= 0; j--) {
        if (t.feature[(size_t)j] == -1) { val[j] = (double)t.output[(size_t)j]; continue; }
        const int l = t.left[(size_t)j], r = t.right[(size_t)j];
        uint64_t a = cover[l], b = cover[r];
        if (a + b == 0) a = b = 1;
        const double pa = (double)a * val[l];
        const double pb = (double)b * val[r];
        val[j] = (pa + pb) / (double)(a + b);
    }
}

// slot [n_nodes]: of a split, the place of its feature in columns (sorted pairs (id, place)), or `rest`; of a leaf, -1
inline void contrib_node_slots(const HostTree &t, const std::vector<std::pair<int32_t, int32_t>> &sorted_columns, int32_t rest, int32_t *slot)
{
    for (int j = 0; j < t.n_nodes; j++) {
        const int32_t f = t.feature[(size_t)j];
        if (f == -1) { slot[j] = -1; continue; }
        auto it = std::lower_bound(sorted_columns.begin(), sorted_columns.end(), std::make_pair(f, (int32_t)INT32_MIN));
        slot[j] = (it != sorted_columns.end() && it->first == f) ? it->second : rest;
    }
}

// The LDS of k_model_contribs: nodes of a tile of trees, 32 bytes each, and the accumulators [slots of the pass][docs + 1] f64 (the + 1
// keeps the transposed read of the store phase off one bank).  kContribTile trees at most, fewer while the tile would pass a fifth of
// the budget.
constexpr int kContribLds = 160 * 1024, kContribTile = 8, kContribNodeBytes = 32, kContribDocsMin = 64, kContribDocsMax = 256;

inline int contrib_tree_tile(int maxn)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(kContribTile, (int64_t)(kContribLds / 5) / ((int64_t)kContribNodeBytes * maxn)));
}

// the most slots a block of `docs` documents holds beside its tree tile (0: not even one)
inline int64_t contrib_slot_limit(int maxn, int docs)
{
    const int64_t left = (int64_t)kContribLds - (int64_t)contrib_tree_tile(maxn) * maxn * kContribNodeBytes;
    return left <= 0 ? 0 : left / ((int64_t)(docs + 1) * 8);
}

// docs of a block and slots of a pass for `slots` slots in all: the widest block of 256, 128 or 64 documents that holds every slot in
// one pass (a wider block stages the tree tile less often per document); else blocks of 64 and several passes
inline bool contrib_plan(int maxn, int64_t slots, int &docs, int64_t &per_pass)
{
    for (docs = kContribDocsMax; docs >= kContribDocsMin; docs /= 2)
        if (contrib_slot_limit(maxn, docs) >= slots) { per_pass = slots; return true; }
    docs = kContribDocsMin;
    per_pass = contrib_slot_limit(maxn, docs);
    return per_pass >= 1;
}

}  // namespace rl
