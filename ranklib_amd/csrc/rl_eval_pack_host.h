// rl_eval_pack_host.h -- the host side of k_model_eval_tiled (rl_model_eval.inc): the kernel's tile constants, its LDS
// budget and the packed format it walks -- which models the packing takes, the 64-bit nodes, a tile's deal to the walkers and their
// walk lengths.  Plain C++, no device: it is also compiled into tools/eval_pack_host_check.cpp, a stand-alone program that runs under
// the host sanitizers (tests/test_eval_pack_cpu.py replays the kernel's walk on what it prints).
//
// The format, per model of nt trees and maxn = the largest tree's nodes:
//   nodes [nt][maxn]               a tree's nodes renumbered breadth-first, so siblings are adjacent (right = left + 1):
//                                    bits 0..31 threshold (a leaf: its output) float bits | 32..47 byte offset of the column in the staged
//                                    tile, feature * kEvalDocs * 4 | 48..63 byte offset of the left child in the tree
//                                  A leaf loops onto itself: it "reads" column 0, where the staged tile holds -infinity, so `x <= value`
//                                  is always true, and its left-child offset is its own.  Padding words are 0: such a leaf with value +0.0.
//   perm  [tiles][kEvalTreeTile]   chain u of walker p walks tree perm[p * kEvalPer + u] of the tile (255: none, in the last, partial tile).
//                                  The trees of a tile, stably sorted by descending depth, are dealt round the walkers (walker p: ranks p,
//                                  p + kEvalParts, ..), deepest first inside a walker; deal = false or a partial tile: kEvalPer consecutive
//                                  ranks each.
//   meta  [tiles][kEvalMetaDepths] the walkers' steps [kEvalParts] = max(depth, 1) of a walker's deepest tree (0: it has no tree), then per
//                                  walker the steps at which its kEvalPhases phases end.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rl_model.h"

namespace rl {

#ifndef RL_EVAL_PARTS
#define RL_EVAL_PARTS 4
#endif
#ifndef RL_EVAL_PER
#define RL_EVAL_PER 8
#endif
constexpr int kEvalDocs = 64, kEvalParts = RL_EVAL_PARTS, kEvalPer = RL_EVAL_PER, kEvalTreeTile = kEvalParts * kEvalPer;
constexpr int kEvalThreads = kEvalDocs * (kEvalParts + 1), kEvalPrefetch = 8;     // 8-byte words each thread prefetches per tile
// Phases of a walker's walk (round 6; see the loop): chains still walking after the first phase, the second, .. and in the last one.  Same box,
// alternating libraries, 30 M rows x 10 000 trees (profiles/r06w_ab_infer_phased_walk.txt): one loop of eight chains 26.8 M docs/s | 8 -> 4: 27.9 |
// 8 -> 4 -> 2: 27.5 | 8 -> 6 -> 4 -> 2: 28.3 - 28.5 | a staircase 8 -> 7 -> .. -> 1: 23.3.
#ifndef RL_EVAL_PHASES
#define RL_EVAL_PHASES 3
#endif
#if RL_EVAL_PHASES == 1
constexpr int kEvalPhases = 1, kEvalPh1 = 4, kEvalPh2 = 2, kEvalPhLast = 4;
#elif RL_EVAL_PHASES == 2
constexpr int kEvalPhases = 2, kEvalPh1 = 4, kEvalPh2 = 2, kEvalPhLast = 2;
#else
constexpr int kEvalPhases = 3, kEvalPh1 = 6, kEvalPh2 = 4, kEvalPhLast = 2;
#endif
static_assert(kEvalPer >= kEvalPh1 && kEvalPh1 >= kEvalPh2 && kEvalPh2 >= kEvalPhLast && kEvalPhLast >= 1, "a phase walks the deepest chains of the phase before it");
constexpr int kEvalMetaDepths = kEvalParts * (1 + kEvalPhases);      // per tile: every walker's steps, then the steps at which its phases end

constexpr size_t kEvalLdsBudget = (size_t)160 * 1024;                // the dynamic LDS k_model_eval_tiled may ask for

// cols = max(row_stride, largest column any node reads + 1)
inline size_t eval_tiled_lds(int cols, int maxn)
{
    return (size_t)cols * kEvalDocs * 4 + (size_t)kEvalTreeTile * maxn * 8 + (size_t)2 * kEvalTreeTile * kEvalDocs * 4 + 2 * kEvalTreeTile * 4 + 2 * (kEvalTreeTile + kEvalMetaDepths);
}

constexpr int kEvalMaxDepth = 250;                                   // walk lengths are bytes

struct EvalPack {
    bool ok = false;
    const char *why = nullptr;                                       // !ok: the rule that refused the model
    std::vector<unsigned long long> nodes;
    std::vector<unsigned char> perm, meta;
    int32_t maxcol = 0;                                              // largest column any node reads (set whether ok or not)
};

// One tree, renumbered breadth-first and packed into out[0, n_nodes).  Returns its depth, or -1 and the rule it breaks.
inline int eval_pack_tree(const HostTree &t, unsigned long long *out, const char *&why)
{
    std::vector<int> order(1, 0), newid((size_t)t.n_nodes, -1), lvl(1, 0);
    int depth = 0;
    newid[0] = 0;
    for (size_t h = 0; h < order.size(); h++) {
        const int j = order[h];
        if (t.feature[j] == -1) continue;
        if (t.left[j] < 0 || t.right[j] < 0 || t.left[j] >= t.n_nodes || t.right[j] >= t.n_nodes || (int)order.size() + 2 > t.n_nodes) {
            why = "a child index lies outside the tree";
            return -1;
        }
        newid[t.left[j]] = (int)order.size(); order.push_back(t.left[j]); lvl.push_back(lvl[h] + 1);
        newid[t.right[j]] = (int)order.size(); order.push_back(t.right[j]); lvl.push_back(lvl[h] + 1);
        depth = std::max(depth, lvl[h] + 1);
    }
    for (size_t h = 0; h < order.size(); h++) {
        const int j = order[h];
        const bool leaf = t.feature[j] == -1;
        uint32_t bits; const float fv = leaf ? t.output[j] : t.threshold[j];
        memcpy(&bits, &fv, 4);
        if (leaf && std::isnan(fv)) { why = "a leaf output is NaN"; return -1; }      // a leaf loops through `-inf <= value`: NaN outputs take the generic kernel
        // leaf: reads column 0 (-infinity in the staged tile) and its left child is itself
        const unsigned long long co = leaf ? 0ull : (unsigned long long)t.feature[j] * kEvalDocs * 4;
        const unsigned long long lo = leaf ? (unsigned long long)h * 8 : (unsigned long long)newid[t.left[j]] * 8;
        out[h] = (unsigned long long)bits | (co << 32) | (lo << 48);
    }
    if (depth > kEvalMaxDepth) { why = "a tree is deeper than 250"; return -1; }
    return depth;
}

// One tile of tt trees with depths depth[0, tt): perm [kEvalTreeTile] (preset to 255) and the walkers' steps [kEvalParts] (preset to 0).
// The sorted trees are dealt ROUND the walkers (walker p: ranks p, p + 4, p + 8, ..; deepest first inside a walker as the phases need it): every
// walker spans the tile's whole range of depths, so its chains drop out early and the four walkers reach the tile's barrier together.
// With eight consecutive ranks each (rounds 4 - 5, RLHIP_EVAL_DEAL=0) walker 0 held the eight deepest trees -- little to drop, and the others
// waited for it: 28.2 against 28.8 M docs/s (profiles/r06w_ab_infer_phased_walk.txt).
inline void eval_deal_tile(const int *depth, size_t tt, bool deal, unsigned char *perm, unsigned char *steps)
{
    std::vector<int> idx(tt);
    for (size_t q = 0; q < tt; q++) idx[q] = (int)q;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return depth[a] > depth[b]; });
    if (deal && tt == (size_t)kEvalTreeTile) {
        std::vector<int> rr(tt);
        for (size_t q = 0; q < tt; q++) rr[(q % kEvalParts) * kEvalPer + q / kEvalParts] = idx[q];
        idx = rr;
    }
    for (size_t q = 0; q < tt; q++) {
        perm[q] = (unsigned char)idx[q];
        unsigned char &g = steps[q / kEvalPer];
        g = std::max<unsigned char>(g, (unsigned char)std::max(depth[idx[q]], 1));      // (a single-leaf tree still stores its output: one step)
    }
}

// The phase ends of one tile, ends [kEvalParts][kEvalPhases].  A phase of n chains ends when the walker's (n' + 1)-th tree (n' = the next
// phase's chains) is done: that tree's depth.  A walker with fewer trees: 0 (the phase is skipped).  phased = false (RLHIP_EVAL_PHASED=0):
// every phase runs to the walker's full depth (one loop, rounds 4 - 5).
inline void eval_phase_ends(const int *depth, size_t tt, bool phased, const unsigned char *perm, const unsigned char *steps, unsigned char *ends)
{
    const int next_ch[3] = {kEvalPhases >= 2 ? kEvalPh1 : kEvalPhLast, kEvalPhases >= 3 ? kEvalPh2 : kEvalPhLast, kEvalPhLast};
    for (int p = 0; p < kEvalParts; p++)
        for (int ph = 0; ph < kEvalPhases; ph++) {
            const size_t q = (size_t)p * kEvalPer + next_ch[ph];
            ends[p * kEvalPhases + ph] = !phased ? steps[p] : (q < tt ? (unsigned char)std::max(depth[perm[q]], 1) : 0);
        }
}

// The packing of a model, or which rule refuses it (the generic kernel then scores it).  maxn: the largest tree's nodes, at least 1.
inline EvalPack eval_pack(const std::vector<HostTree> &trees, int maxn, bool deal, bool phased)
{
    EvalPack pk;
    const size_t nt = trees.size();
    bool fid_ok = true;                  // column 0 is what a packed leaf reads (no RankLib feature has id 0: learning/DataPoint.java:33)
    for (const HostTree &t : trees)
        for (int32_t f : t.feature) if (f != -1) { pk.maxcol = std::max(pk.maxcol, f); fid_ok = fid_ok && f >= 1; }
    if (nt == 0) pk.why = "there are no trees";
    else if (!fid_ok) pk.why = "a feature id is below 1";
    else if ((size_t)maxn * 8 >= 0x10000) pk.why = "a child offset does not fit 16 bits";
    else if (((size_t)pk.maxcol + 1) * kEvalDocs * 4 >= 0xffff) pk.why = "a column offset does not fit 16 bits";
    else if ((size_t)kEvalTreeTile * maxn > (size_t)kEvalThreads * kEvalPrefetch) pk.why = "a tile of trees is more than a block prefetches";
    if (pk.why) return pk;
    pk.nodes.assign(nt * maxn, 0ull);                                 // (padding: a leaf at offset 0 with value +0.0)
    std::vector<int> depth(nt, 0);
    for (size_t i = 0; i < nt && !pk.why; i++) depth[i] = eval_pack_tree(trees[i], pk.nodes.data() + i * maxn, pk.why);
    if (pk.why) { pk.nodes.clear(); return pk; }
    const size_t ntl = (nt + kEvalTreeTile - 1) / kEvalTreeTile;
    pk.perm.assign(ntl * kEvalTreeTile, 255);
    pk.meta.assign(ntl * kEvalMetaDepths, 0);
    for (size_t tl = 0; tl < ntl; tl++) {
        const size_t t0 = tl * kEvalTreeTile, tt = std::min<size_t>(kEvalTreeTile, nt - t0);
        unsigned char *perm = pk.perm.data() + tl * kEvalTreeTile, *steps = pk.meta.data() + tl * kEvalMetaDepths;
        eval_deal_tile(depth.data() + t0, tt, deal, perm, steps);
        eval_phase_ends(depth.data() + t0, tt, phased, perm, steps, steps + kEvalParts);
    }
    pk.ok = true;
    return pk;
}

}  // namespace rl
