// rl_shap_host.h -- the host side of exact TreeSHAP contributions (rl_shap.inc): the path tables of every leaf (the
// elements of its root-to-leaf path with their slots, cover products z and split conditions), the limit on a path's distinct features,
// the factor tables A / B / U / R and the LDS plan of k_model_shap.  Plain C++, no device: it is also compiled into
// tools/shap_host_check.cpp, a stand-alone program that runs under the host sanitizers.  The argument checks are rl_contrib_host.h's.
// Built with -ffp-contract=off like the rest: a ratio is one quotient, z one product per further split of the feature, each rounded.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "rl_contrib_host.h"

namespace rl {

constexpr int kShapP = 32;                                             // distinct features on one path at most: every tree of up to 33 leaves
constexpr int kShapT = kShapP + 1;                                     // the tables are [kShapT][kShapT], indexed [l][i], 0 <= i < l <= P

struct alignas(16) ShapLeaf { double out; int32_t el0, d; };          // (double)out of the leaf, its elements [el0, el0 + d)
struct alignas(8) ShapElem { double z; int32_t feat, slot, c0, nc; }; // its conditions [c0, c0 + nc)
struct alignas(8) ShapCond { float thr; int32_t left; };              // the path goes left (1) or right (0) at a split with this threshold
static_assert(sizeof(ShapLeaf) == 16 && sizeof(ShapElem) == 24 && sizeof(ShapCond) == 8, "the device reads these as they are");

struct ShapPaths {
    std::vector<int32_t> leaf0;                                        // [trees + 1]: the leaves of tree t are [leaf0[t], leaf0[t + 1])
    std::vector<ShapLeaf> leaves;                                      // in tree order, then the pre-order of the model text
    std::vector<ShapElem> elems;
    std::vector<ShapCond> conds;
};

// the splits from the root to `node`, the root's first: (split, 1 if the path goes left there)
inline void shap_path_to(const std::vector<int32_t> &parent, const HostTree &t, int node, std::vector<std::pair<int32_t, int32_t>> &steps)
{
    steps.clear();
    for (int j = node; parent[(size_t)j] >= 0; j = parent[(size_t)j]) steps.push_back({parent[(size_t)j], t.left[(size_t)parent[(size_t)j]] == j ? 1 : 0});
    std::reverse(steps.begin(), steps.end());
}

inline std::vector<int32_t> shap_parents(const HostTree &t)
{
    std::vector<int32_t> parent((size_t)t.n_nodes, -1);
    for (int j = 0; j < t.n_nodes; j++)
        if (t.feature[(size_t)j] != -1) parent[(size_t)t.left[(size_t)j]] = parent[(size_t)t.right[(size_t)j]] = j;
    return parent;
}

// the longest element list of a tree -- the most distinct features on one root-to-leaf path -- and the leaf that has it (its place
// among the tree's leaves, and its node).  Needs no cover.
inline int32_t shap_tree_max_path(const HostTree &t, int32_t *leaf_at, int32_t *node_at)
{
    const std::vector<int32_t> parent = shap_parents(t);
    std::vector<std::pair<int32_t, int32_t>> steps;
    std::vector<int32_t> seen;
    int32_t best = -1, leaf = 0;
    for (int j = 0; j < t.n_nodes; j++) {
        if (t.feature[(size_t)j] != -1) continue;
        shap_path_to(parent, t, j, steps);
        seen.clear();
        for (const auto &s : steps) {
            const int32_t f = t.feature[(size_t)s.first];
            if (std::find(seen.begin(), seen.end(), f) == seen.end()) seen.push_back(f);
        }
        if ((int32_t)seen.size() > best) {
            best = (int32_t)seen.size();
            if (leaf_at) *leaf_at = leaf;
            if (node_at) *node_at = j;
        }
        leaf++;
    }
    return std::max<int32_t>(best, 0);
}

// RLC_UNSUPPORTED, naming tree and leaf, when a path of the model holds more than kShapP distinct features; *max_path is the model's longest
inline int shap_check_paths(const std::string &w, const std::vector<HostTree> &trees, int32_t *max_path, std::string &err)
{
    int32_t longest = 0;
    for (size_t t = 0; t < trees.size(); t++) {
        int32_t leaf = 0, node = 0;
        const int32_t d = shap_tree_max_path(trees[t], &leaf, &node);
        longest = std::max(longest, d);
        if (d > kShapP && err.empty())
            err = w + "the path to leaf " + std::to_string(leaf) + " (node " + std::to_string(node) + ") of tree " + std::to_string(t) + " holds " +
                  std::to_string(d) + " distinct features, more than " + std::to_string(kShapP);
    }
    if (max_path) *max_path = longest;
    return err.empty() ? RLC_OK : RLC_UNSUPPORTED;
}

// appends the tables of one tree: per leaf the distinct features of its path in order of first appearance, each with its slot
// (slot [n_nodes] as contrib_node_slots made it), z -- the f64 product, in root-to-leaf order, of c[child on the path] / (a + b) over the
// path's splits on the feature, a = b = 1 where a + b == 0 -- and those splits' conditions
inline void shap_tree_paths(const HostTree &t, const uint64_t *cover, const int32_t *slot, ShapPaths &p)
{
    if (p.leaf0.empty()) p.leaf0.push_back(0);
    const std::vector<int32_t> parent = shap_parents(t);
    std::vector<std::pair<int32_t, int32_t>> steps;
    std::vector<ShapElem> els;
    std::vector<std::vector<ShapCond>> cds;
    for (int j = 0; j < t.n_nodes; j++) {
        if (t.feature[(size_t)j] != -1) continue;
        shap_path_to(parent, t, j, steps);
        els.clear(); cds.clear();
        for (const auto &s : steps) {
            const int32_t nd = s.first, f = t.feature[(size_t)nd];
            uint64_t a = cover[t.left[(size_t)nd]], b = cover[t.right[(size_t)nd]];
            if (a + b == 0) a = b = 1;
            const double r = (double)(s.second ? a : b) / (double)(a + b);
            size_t e = 0;
            while (e < els.size() && els[e].feat != f) e++;
            if (e == els.size()) { els.push_back(ShapElem{r, f, slot[nd], 0, 0}); cds.emplace_back(); }
            else els[e].z = els[e].z * r;
            cds[e].push_back(ShapCond{t.threshold[(size_t)nd], s.second});
        }
        p.leaves.push_back(ShapLeaf{(double)t.output[(size_t)j], (int32_t)p.elems.size(), (int32_t)els.size()});
        for (size_t e = 0; e < els.size(); e++) {
            els[e].c0 = (int32_t)p.conds.size(); els[e].nc = (int32_t)cds[e].size();
            p.conds.insert(p.conds.end(), cds[e].begin(), cds[e].end());
            p.elems.push_back(els[e]);
        }
    }
    p.leaf0.push_back((int32_t)p.leaves.size());
}

// A[l][i] = (i+1)/(l+1), B[l][i] = (l-i)/(l+1), U[l][i] = (l+1)/(i+1), R[l][i] = (l+1)/(l-i) for 0 <= i < l <= P, one f64 quotient each;
// four tables of kShapT * kShapT, one behind the other
inline std::vector<double> shap_tables()
{
    std::vector<double> tb((size_t)4 * kShapT * kShapT, 0.0);
    for (int l = 1; l < kShapT; l++)
        for (int i = 0; i < l; i++) {
            const size_t at = (size_t)l * kShapT + i, n = (size_t)kShapT * kShapT;
            tb[at] = (double)(i + 1) / (double)(l + 1);
            tb[n + at] = (double)(l - i) / (double)(l + 1);
            tb[2 * n + at] = (double)(l + 1) / (double)(i + 1);
            tb[3 * n + at] = (double)(l + 1) / (double)(l - i);
        }
    return tb;
}

// The LDS of k_model_shap: the accumulators [slots of the pass][docs + 1] f64 as k_model_contribs has them, and the per-lane w[] array
// [wd][docs] f64 with wd = the model's longest element list + 1 (not P + 1: the rows a model cannot use would cost the block width).
// The path tables are not staged: they are wave-uniform and read through the scalar cache.
constexpr int kShapLds = kContribLds, kShapDocsMin = kContribDocsMin, kShapDocsMax = kContribDocsMax;

inline int64_t shap_slot_limit(int wd, int docs)
{
    const int64_t left = (int64_t)kShapLds - (int64_t)wd * docs * 8;
    return left <= 0 ? 0 : left / ((int64_t)(docs + 1) * 8);
}

// docs of a block and slots of a pass: the widest block of 256, 128 or 64 documents that holds every slot in one pass, else blocks of
// 64 and several column passes
inline bool shap_plan(int wd, int64_t slots, int &docs, int64_t &per_pass)
{
    for (docs = kShapDocsMax; docs >= kShapDocsMin; docs /= 2)
        if (shap_slot_limit(wd, docs) >= slots) { per_pass = slots; return true; }
    docs = kShapDocsMin;
    per_pass = shap_slot_limit(wd, docs);
    return per_pass >= 1;
}

}  // namespace rl
