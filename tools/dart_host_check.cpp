// dart_host_check.cpp -- a stand-alone run of the host side of DART (ranklib_amd/csrc/rl_dart_host.h: the draw of a round's drop set and the
// weight arithmetic): host code only, no device, run on the CPU.
//
//   g++ -std=c++17 -ffp-contract=off tools/dart_host_check.cpp -o dart_host_check                 (tests/test_dart_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dart_host_check.cpp -o dart_host_check
//   ./dart_host_check seed rate_drop max_drop lr rounds
//
// The hash is the trainer's (rl_device.h: mix64, root_hash, feature_key; the oracle's ro_root_hash / ro_feature_key), restated here because that
// header is device code.  For every round m = 0 .. rounds - 1 it draws the drop set as the trainer does, rescales the weights, and prints
//   round <m> k <k> w_m <bits, hex> dropped <ids ...> weights <bits of w_0 .. w_m, hex>
// On its own -- no arguments -- it runs max_drop above, at and below the candidate count and m = 0, and fails loudly on a wrong set.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ranklib_amd/csrc/rl_dart_host.h"

using namespace rl;

static uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
static uint64_t root_hash(uint64_t seed, int tree) { return mix64(seed ^ mix64((uint64_t)(uint32_t)tree)); }
static uint64_t feature_key(uint64_t h, int f) { return mix64(h ^ ((uint64_t)(uint32_t)(f + 1) * 0xA24BAED4963EE407ULL)); }

static std::vector<int32_t> draw(uint64_t seed, int m, float rate, int max_drop)
{
    std::vector<int32_t> D;
    const uint64_t h = root_hash(seed ^ kDartSeedTag, m);
    dart_draw([&](int32_t i) { return feature_key(h, i); }, m, rate, max_drop, D);
    return D;
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int self_check()
{
    int bad = 0;
    if (!draw(1, 0, 1.0f, 0).empty()) { printf("round 0 dropped a tree\n"); bad++; }
    const int m = 40;
    const std::vector<int32_t> all = draw(1, m, 1.0f, 0);
    if ((int)all.size() != m) { printf("rate 1 kept %zu of %d\n", all.size(), m); bad++; }
    const std::vector<int32_t> cand = draw(1, m, 0.5f, 0);
    const int n = (int)cand.size();
    for (int cap : {n + 3, n, n - 1, 1}) {
        const std::vector<int32_t> D = draw(1, m, 0.5f, cap);
        const int want = cap < n ? cap : n;
        if ((int)D.size() != want) { printf("max_drop %d of %d candidates kept %zu\n", cap, n, D.size()); bad++; }
        for (size_t j = 0; j < D.size(); j++) {
            bool in = false;
            for (int32_t c : cand) in |= c == D[j];
            if (!in || (j > 0 && D[j - 1] >= D[j])) { printf("max_drop %d: entry %zu is no candidate or out of order\n", cap, j); bad++; }
        }
        if (cap < n) {      // the kept ones hold the smallest keys
            const uint64_t h = root_hash(1 ^ kDartSeedTag, m);
            uint64_t worst = 0;
            for (int32_t d : D) worst = std::max(worst, feature_key(h, d));
            for (int32_t c : cand) {
                bool kept = false;
                for (int32_t d : D) kept |= d == c;
                if (!kept && feature_key(h, c) < worst) { printf("max_drop %d: tree %d has a smaller key than a kept one\n", cap, c); bad++; }
            }
        }
    }
    if (bits(dart_new_weight(0, 0.1f)) != bits(0.1f)) { printf("k = 0 changes the learning rate\n"); bad++; }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return self_check();
    if (argc != 6) { fprintf(stderr, "usage: dart_host_check [seed rate_drop max_drop lr rounds]\n"); return 2; }
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    const float rate = strtof(argv[2], nullptr), lr = strtof(argv[4], nullptr);
    const int max_drop = atoi(argv[3]), rounds = atoi(argv[5]);
    std::vector<float> w;
    for (int m = 0; m < rounds; m++) {
        const std::vector<int32_t> D = draw(seed, m, rate, max_drop);
        const int k = (int)D.size();
        const float f = k ? dart_factor(k, lr) : 1.0f;
        for (int32_t d : D) w[(size_t)d] = dart_scaled(w[(size_t)d], f);
        w.push_back(dart_new_weight(k, lr));
        printf("round %d k %d w_m %08" PRIx32 " dropped", m, k, bits(w.back()));
        for (int32_t d : D) printf(" %d", d);
        printf(" weights");
        for (float x : w) printf(" %08" PRIx32, bits(x));
        printf("\n");
    }
    return 0;
}
