// rl_interv_host.h -- the host side of interventional TreeSHAP against background rows (rl_interv.inc): the checks of the
// background's arguments, the table T, the LDS plan of k_model_interv and the tree chunks of the background's mask buffer.  Plain C++,
// no device: it is also compiled into tools/interv_host_check.cpp, a stand-alone program that runs under the host sanitizers.  The path
// tables (ShapPaths, shap_tree_paths with null covers, shap_check_paths) are rl_shap_host.h's, the other argument checks
// rl_contrib_host.h's.  Built with -ffp-contract=off like the rest: an entry of T is one quotient.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "rl_shap_host.h"

namespace rl {

constexpr int32_t kIntervMaxBg = 16384;                                // background rows of a call at most

// what rl_model_predict_shap_background checks of its background before the device is touched
inline int interv_check_background(const std::string &w, const void *BG, int32_t n_background, int32_t bg_stride, std::string &err)
{
    if (!BG) { err = w + "null BG"; return RLC_INVALID; }
    if (n_background < 1) { err = w + "n_background must be >= 1"; return RLC_INVALID; }
    if (bg_stride < 1) { err = w + "bg_stride must be >= 1"; return RLC_INVALID; }
    if (n_background > kIntervMaxBg) { err = w + "more than " + std::to_string(kIntervMaxBg) + " background rows"; return RLC_UNSUPPORTED; }
    return RLC_OK;
}

// T[p][q] = 1.0 / (double)(p * C(p + q, p)) for 1 <= p, 0 <= q, p + q <= P, as [kShapT][kShapT] indexed [p][q]: the Shapley weight
// (p - 1)! q! / (p + q)! of a feature among p that have to be in the set while q have to stay out.  The denominator is an exact integer
// (below 2^34) and the entry one rounded division; row 0 and the cells with p + q > P stay 0.0 and are never used.
inline std::vector<double> interv_table()
{
    std::vector<double> tb((size_t)kShapT * kShapT, 0.0);
    for (int p = 1; p <= kShapP; p++)
        for (int q = 0; p + q <= kShapP; q++) {
            uint64_t c = 1;                                            // C(p + q, p) = prod_{i = 1 .. p} (q + i) / i, exact at every step
            for (int i = 1; i <= p; i++) c = c * (uint64_t)(q + i) / (uint64_t)i;
            tb[(size_t)p * kShapT + q] = 1.0 / (double)((uint64_t)p * c);
        }
    return tb;
}

// The LDS of k_model_interv: the table T, the accumulators [slots of the pass][docs + 1] f64 as k_model_contribs has them, and the
// per-lane sums s[wd][docs] f64, wd = the model's longest element list.
constexpr int kIntervTableBytes = kShapT * kShapT * 8;

inline int64_t interv_slot_limit(int wd, int docs)
{
    const int64_t left = (int64_t)kShapLds - kIntervTableBytes - (int64_t)wd * docs * 8;
    return left <= 0 ? 0 : left / ((int64_t)(docs + 1) * 8);
}

inline size_t interv_lds_bytes(int wd, int docs, int ns) { return (size_t)kIntervTableBytes + ((size_t)ns * (docs + 1) + (size_t)wd * docs) * 8; }

// docs of a block and slots of a pass: the widest block of 256, 128 or 64 documents that holds every slot in one pass, else blocks of
// 64 and several column passes
inline bool interv_plan(int wd, int64_t slots, int &docs, int64_t &per_pass)
{
    for (docs = kShapDocsMax; docs >= kShapDocsMin; docs /= 2)
        if (interv_slot_limit(wd, docs) >= slots) { per_pass = slots; return true; }
    docs = kShapDocsMin;
    per_pass = interv_slot_limit(wd, docs);
    return per_pass >= 1;
}

// The mask buffer zm[leaf][mask stride] uint32 holds the background's masks of a chunk of trees; a row of it is padded to a multiple of
// four words so that the walk reads four masks with one 16-byte uniform load.  Beside it goes zleaf[tree][B] int32, the leaf each
// background row ends in.
inline int32_t interv_mask_stride(int32_t n_background) { return (n_background + 3) & ~3; }

inline int64_t interv_tree_bytes(int32_t leaves, int32_t n_background)
{
    return 4 * ((int64_t)leaves * interv_mask_stride(n_background) + n_background);
}

// The tree chunks of a call, [chunks + 1] ascending from 0 to the tree count: as many trees in order as fit scratch_bytes (0: 256 MiB)
// with their masks and leaf indices, one tree at least.
inline std::vector<int32_t> interv_tree_chunks(const std::vector<int32_t> &leaf0, int32_t n_background, int64_t scratch_bytes)
{
    const int64_t budget = scratch_bytes > 0 ? scratch_bytes : ((int64_t)256 << 20);
    const int32_t T = leaf0.empty() ? 0 : (int32_t)leaf0.size() - 1;
    std::vector<int32_t> cut{0};
    int64_t used = 0;
    for (int32_t t = 0; t < T; t++) {
        const int64_t b = interv_tree_bytes(leaf0[(size_t)t + 1] - leaf0[(size_t)t], n_background);
        if (t > cut.back() && used + b > budget) { cut.push_back(t); used = 0; }
        used += b;
    }
    if (T > 0) cut.push_back(T);
    return cut;
}

}  // namespace rl
