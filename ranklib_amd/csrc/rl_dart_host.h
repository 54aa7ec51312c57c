// rl_dart_host.h -- the host side of DART (rl_dart.inc): which of the trees 0 .. m-1 round m drops, and the weights the round
// leaves behind.  Plain C++, no device: it is also compiled into tools/dart_host_check.cpp, a stand-alone program that runs under the host
// sanitizers.  The hash behind the draw is the caller's (the trainer passes feature_key(root_hash(seed ^ kDartSeedTag, m), i), rl_device.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace rl {

constexpr uint64_t kDartSeedTag = 0x44415254ull;              // "DART": the draw's hash chain starts apart from the feature sampling's

// Tree i < m is a candidate when its key's top 53 bits, as a fraction of 2^53, lie below rate_drop; of more than max_drop candidates the
// max_drop smallest keys stay (ties: the smaller index); max_drop <= 0: no cap.  -> the kept trees in ascending order
template <class Key>
inline void dart_draw(Key key, int32_t m, float rate_drop, int32_t max_drop, std::vector<int32_t> &dropped)
{
    dropped.clear();
    std::vector<std::pair<uint64_t, int32_t>> cand;
    for (int32_t i = 0; i < m; i++) {
        const uint64_t k = key(i);
        if ((double)(k >> 11) * 0x1.0p-53 < (double)rate_drop) cand.push_back({k, i});
    }
    if (max_drop > 0 && cand.size() > (size_t)max_drop) {
        std::sort(cand.begin(), cand.end());                  // (key, index): ties go to the smaller index
        cand.resize((size_t)max_drop);
    }
    for (const auto &c : cand) dropped.push_back(c.second);
    std::sort(dropped.begin(), dropped.end());
}

// XGBoost's "tree" normalisation: with k trees dropped the new tree gets lr / (k + lr), a dropped tree keeps k / (k + lr) of its weight
inline float dart_new_weight(int32_t k, float lr) { return k == 0 ? lr : (float)((double)lr / ((double)k + (double)lr)); }
inline float dart_factor(int32_t k, float lr) { return (float)((double)k / ((double)k + (double)lr)); }
inline float dart_scaled(float w, float f) { return (float)((double)w * (double)f); }

}  // namespace rl
