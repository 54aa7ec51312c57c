// rl_interact_host.h -- the host side of SHAP interaction values (rl_interact.inc): per conditioned slot the list of the
// leaves a block has to walk, the LDS plan of k_model_interact and the rule that cuts a call's rows into chunks.  Plain C++, no device:
// it is also compiled into tools/interact_host_check.cpp, a stand-alone program that runs under the host sanitizers.  The path tables
// (ShapPaths, shap_tree_paths, shap_check_paths, shap_tables) are rl_shap_host.h's, the argument checks rl_contrib_host.h's.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "rl_shap_host.h"

namespace rl {

constexpr int64_t kInteractMaxSlots = 65535;                           // conditioned slots of a call at most: they are the grid's second dimension

struct alignas(8) InteractLeaf { int32_t leaf, tree; };                // a leaf of ShapPaths::leaves and the tree it belongs to
static_assert(sizeof(InteractLeaf) == 8, "the device reads these as they are");

struct InteractLists {
    std::vector<int32_t> list0;                                        // [C + 2]: the leaves of conditioned slot s are [list0[s], list0[s + 1]), s = 0 .. C
    std::vector<InteractLeaf> list;                                    // ascending by leaf, so in tree order, then the pre-order of the model text
};

// Per slot 0 .. C (the columns and rest; the bias conditions nothing) the leaves that have an element in that slot and at least two
// elements: a block conditioned on the slot walks these only, every other leaf contributes exactly zero to its cells.
inline InteractLists interact_lists(const ShapPaths &p, int32_t C)
{
    InteractLists il;
    std::vector<std::vector<InteractLeaf>> per((size_t)C + 1);
    const int32_t nt = p.leaf0.empty() ? 0 : (int32_t)p.leaf0.size() - 1;
    for (int32_t t = 0; t < nt; t++)
        for (int32_t lf = p.leaf0[(size_t)t]; lf < p.leaf0[(size_t)t + 1]; lf++) {
            const ShapLeaf &leaf = p.leaves[(size_t)lf];
            if (leaf.d < 2) continue;
            for (int32_t e = 0; e < leaf.d; e++) {
                const int32_t s = p.elems[(size_t)leaf.el0 + e].slot;
                if (s < 0 || s > C) continue;
                if (per[(size_t)s].empty() || per[(size_t)s].back().leaf != lf) per[(size_t)s].push_back(InteractLeaf{lf, t});
            }
        }
    il.list0.push_back(0);
    for (const auto &v : per) {
        il.list.insert(il.list.end(), v.begin(), v.end());
        il.list0.push_back((int32_t)il.list.size());
    }
    return il;
}

// RLC_UNSUPPORTED when the call has more conditioned slots (C + 1) than the grid's second dimension takes
inline int interact_check_slots(const std::string &w, int64_t C, std::string &err)
{
    if (C + 1 > kInteractMaxSlots) {
        err = w + std::to_string(C + 1) + " conditioned slots, more than " + std::to_string(kInteractMaxSlots);
        return RLC_UNSUPPORTED;
    }
    return RLC_OK;
}

// The LDS of k_model_interact: the accumulators [attributed slots of the pass][docs + 1] f64 -- the slots 0 .. C; the bias needs none --
// and the per-lane w[] array [wr][docs] f64.  The recurrence runs on a leaf's elements without the conditioned one, so wr is the
// model's longest element list: one row less than k_model_shap's (and 1 at least, so that the block always has its column).
inline int interact_w_rows(int32_t longest) { return std::max<int32_t>(1, longest); }

inline int64_t interact_slot_limit(int wr, int docs) { return shap_slot_limit(wr, docs); }

// docs of a block and attributed slots of a pass: the widest block of 256, 128 or 64 documents that holds all C + 1 in one pass, else
// blocks of 64 and several column passes
inline bool interact_plan(int wr, int64_t slots, int &docs, int64_t &per_pass) { return shap_plan(wr, slots, docs, per_pass); }

// The rows of a chunk: per row its device buffers are the row itself, 8 (C + 2)^2 bytes of result and 8 (C + 2) bytes of SHAP values,
// all within scratch_bytes (0: 256 MiB).  A chunk holds at least one row.
inline int64_t interact_row_bytes(int32_t row_stride, int64_t C) { return (int64_t)row_stride * 4 + 8 * (C + 2) * (C + 2) + 8 * (C + 2); }

inline int64_t interact_chunk_rows(int64_t n_docs, int32_t row_stride, int64_t C, int64_t scratch_bytes)
{
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : ((int64_t)256 << 20);
    return std::max<int64_t>(1, std::min<int64_t>(n_docs, budget / interact_row_bytes(row_stride, C)));
}

}  // namespace rl
