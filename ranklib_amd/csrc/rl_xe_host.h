// rl_xe_host.h -- the host side of the XE-NDCG objective (rl_xe.inc): the tile size and the block table of k_lambda_xe.
// Plain C++, no device: it is also compiled into tools/xe_host_check.cpp, a stand-alone program that runs under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace rl {

constexpr uint64_t kXeSeedTag = 0x58454E44ull;                // "XEND": gamma's hash chain starts apart from the feature sampling's and DART's
constexpr int kXeTile = 512;                                  // documents of a tile: 44 bytes of LDS each (rl_xe.inc), 23 KB a block -- six blocks fit a CU's LDS, five its registers
constexpr int kXeMaxLabel = 30;                               // phi = 2^(int)label - gamma as a double built from its exponent; RankLib's own gain wraps above 30

// the tile size in force: the build constant, or the knob's value (RLHIP_XE_TILE, rl_debug_xe_lambdas' argument) where that is smaller; <= 0: unset
inline int xe_tile(int knob) { return knob > 0 ? std::min(knob, kXeTile) : kXeTile; }

// one block of k_lambda_xe: the lists q0 .. q0 + nq - 1.  nq > 1 or a list of at most `tile` documents: the tile path; else the long path
struct XeBlock { int32_t q0, nq; };

// Consecutive whole lists packed greedily into tiles of at most `tile` documents; every list longer than `tile` gets a block of its own
inline void xe_pack(const int32_t *qoff, int32_t n_lists, int32_t tile, std::vector<XeBlock> &blocks)
{
    blocks.clear();
    XeBlock cur{0, 0};
    int32_t docs = 0;
    auto flush = [&]() { if (cur.nq > 0) blocks.push_back(cur); cur.nq = 0; docs = 0; };
    for (int32_t q = 0; q < n_lists; q++) {
        const int32_t n = qoff[q + 1] - qoff[q];
        if (n > tile) { flush(); blocks.push_back(XeBlock{q, 1}); continue; }
        if (docs + n > tile) flush();
        if (cur.nq == 0) cur.q0 = q;
        cur.nq++; docs += n;
    }
    flush();
}

}  // namespace rl
