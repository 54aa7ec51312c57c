// rl_leaves_host.h -- the host side of the leaf-index kernels (rl_leaves.inc): how a tree's leaves are numbered, the
// trees as eval_pack takes them for k_model_leaves_tiled (leaf numbers where the scorer's pack holds leaf outputs), the deal of a
// window of trees to the walkers, and the argument checks of rl_model_predict_leaves.  Plain C++, no device.
#pragma once
#include <string>

#include "rl_eval_pack_host.h"

namespace rl {

constexpr int kLeavesMax = 65536;                  // leaves of one tree: a leaf number is a uint16_t
// u16 per tree of a walked tile in LDS: the documents and one 32-bit word of padding, so the writer's lanes, which read down the trees
// of one document, fall into different banks (a row of 33 words moves a tree's row on by one bank)
constexpr int kLeavesRow = kEvalDocs + 2;
static_assert(kEvalTreeTile % 4 == 0 && kEvalTreeTile <= 64, "the writer packs four leaf numbers a lane and gives a tile's trees to the lanes of one wavefront");

// no[j] = the number of leaf j among the tree's leaves in pre-order (Split.leaves() order: left first, depth first); 0 at inner nodes.
// Returns the number of leaves.
inline int leaves_number(const HostTree &t, uint16_t *no)
{
    int n = 0;
    for (int j = 0; j < t.n_nodes; j++) {
        const bool leaf = t.feature[j] == -1;
        no[j] = leaf ? (uint16_t)n : (uint16_t)0;
        n += leaf ? 1 : 0;
    }
    return n;
}

inline int leaves_count(const HostTree &t)
{
    int n = 0;
    for (int j = 0; j < t.n_nodes; j++) n += t.feature[j] == -1 ? 1 : 0;
    return n;
}

// The trees with a leaf's NUMBER in the bits of its output: what eval_pack packs into the 32 value bits of a leaf node.  A number below
// 2^16 is +0.0 or a positive subnormal as a float, never NaN, and `-infinity <= value` holds for it whether or not the compare flushes
// subnormals (it would compare -infinity with 0): the leaf stays the walk's fixed point, and the walk ends with the number in a register.
inline std::vector<HostTree> leaves_as_outputs(const std::vector<HostTree> &trees)
{
    std::vector<HostTree> out(trees);
    for (HostTree &t : out) {
        uint32_t n = 0;
        for (int j = 0; j < t.n_nodes; j++)
            if (t.feature[j] == -1) { memcpy(&t.output[j], &n, 4); n++; }
    }
    return out;
}

// the levels below the root of a tree eval_pack has accepted (children in range, no node reached twice)
inline int leaves_tree_depth(const HostTree &t)
{
    std::vector<int> todo(1, 0), lvl(1, 0);
    int depth = 0;
    for (size_t h = 0; h < todo.size(); h++) {
        const int j = todo[h];
        if (t.feature[j] == -1) continue;
        todo.push_back(t.left[j]); lvl.push_back(lvl[h] + 1);
        todo.push_back(t.right[j]); lvl.push_back(lvl[h] + 1);
        depth = std::max(depth, lvl[h] + 1);
    }
    return depth;
}

// The window [first, first + nt) of the model as tiles of its own: tile k holds the trees first + k * kEvalTreeTile .. of the model,
// dealt to the walkers as eval_pack deals a model's tiles.  perm [tiles][kEvalTreeTile], meta [tiles][kEvalMetaDepths].
inline void leaves_deal_window(const int *depth, int nt, bool deal, bool phased, std::vector<unsigned char> &perm, std::vector<unsigned char> &meta)
{
    const size_t ntl = ((size_t)nt + kEvalTreeTile - 1) / kEvalTreeTile;
    perm.assign(ntl * kEvalTreeTile, 255);
    meta.assign(ntl * kEvalMetaDepths, 0);
    for (size_t tl = 0; tl < ntl; tl++) {
        const size_t t0 = tl * kEvalTreeTile, tt = std::min<size_t>(kEvalTreeTile, (size_t)nt - t0);
        unsigned char *p = perm.data() + tl * kEvalTreeTile, *steps = meta.data() + tl * kEvalMetaDepths;
        eval_deal_tile(depth + t0, tt, deal, p, steps);
        eval_phase_ends(depth + t0, tt, phased, p, steps, steps + kEvalParts);
    }
}

// the dynamic LDS of k_model_leaves_tiled: the staged rows, a tile of trees, two tiles of leaf numbers, one tile's deal
inline size_t leaves_tiled_lds(int cols, int maxn)
{
    return (size_t)cols * kEvalDocs * 4 + (size_t)kEvalTreeTile * maxn * 8 + (size_t)2 * kEvalTreeTile * kLeavesRow * 2 + (kEvalTreeTile + kEvalMetaDepths);
}

// The checks of rl_model_predict_leaves that need no device; n_model_trees < 0: a null model, which is looked at after the arguments
// that need none.  *n_trees == 0 becomes "through the last tree".  0, or the status (-1 invalid, -4 unsupported: RL_ERR_*) and the message.
inline int leaves_check(const std::string &w, int64_t n_model_trees, const void *X, int64_t n_docs, int32_t row_stride, int32_t first_tree,
                        int32_t *n_trees, int32_t layout, const void *out, std::string &err)
{
    if (!X) { err = w + "null X"; return -1; }
    if (!out) { err = w + "null output"; return -1; }
    if (n_docs < 0) { err = w + "n_docs must be >= 0"; return -1; }
    if (n_docs > (int64_t)INT32_MAX) { err = w + "more than 2^31 documents per call"; return -4; }
    if (row_stride < 1) { err = w + "row_stride must be >= 1"; return -1; }
    if (layout != 0 && layout != 1) { err = w + "layout = " + std::to_string(layout) + " is neither RL_LEAVES_BY_ROW nor RL_LEAVES_BY_TREE"; return -1; }
    if (first_tree < 0) { err = w + "first_tree must be >= 0"; return -1; }
    if (*n_trees < 0) { err = w + "n_trees must be >= 0"; return -1; }
    if (n_model_trees < 0) { err = w + "null model"; return -1; }
    if (n_model_trees < 1) { err = w + "the model has no trees"; return -1; }
    if (first_tree >= n_model_trees) {
        err = w + "first_tree = " + std::to_string(first_tree) + " is outside [0, " + std::to_string(n_model_trees) + ")";
        return -1;
    }
    if ((int64_t)first_tree + *n_trees > n_model_trees) {
        err = w + "n_trees = " + std::to_string(*n_trees) + " from tree " + std::to_string(first_tree) + " leaves the model's " + std::to_string(n_model_trees) + " trees";
        return -1;
    }
    if (*n_trees == 0) *n_trees = (int32_t)(n_model_trees - first_tree);
    return 0;
}

}  // namespace rl
