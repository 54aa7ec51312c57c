// near_host_check.cpp -- a stand-alone run of the host side of the leaf-space neighbour search (ranklib_amd/csrc/rl_near_host.h: the
// kernel's shape, the argument checks, the cut of a call into query chunks, reference bands and splits): host code only, no device.
//
//   g++ -std=c++17 tools/near_host_check.cpp -o near_host_check                        (tests/test_neighbours_cpu.py builds and reads it)
//   ./near_host_check shape                                    -> shape <query tile> <ref tile> <tree chunk> <blocks> <max k> <max splits> <max trees>
//   ./near_host_check check model_trees nq nr first_tree n_trees k flags
//                                                              -> <status> <n_trees as resolved> <message>    (model_trees < 0: a null model)
//   ./near_host_check plan nq nr bytes_per_row scratch_bytes   -> plan <query chunk> <reference band> <rows of the partial lists>
//                                                                 launch <queries> <references> <tiles per split> <splits>   per (chunk, band) size
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "../ranklib_amd/csrc/rl_near_host.h"

using namespace rl;

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "shape")) {
        printf("shape %d %d %d %d %d %d %d\n", kNearQT, kNearRT, kNearTC, kNearBlocks, kNearMaxK, kNearMaxSplits, kNearMaxTrees);
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "check")) {
        int32_t nt = atoi(argv[6]);
        int dummy = 0;
        std::string err;
        const int rc = near_check("", atoll(argv[2]), &dummy, atoll(argv[3]), &dummy, atoll(argv[4]), 1, atoi(argv[5]), &nt, atoi(argv[7]), atoi(argv[8]), 0,
                                  &dummy, &dummy, err);
        printf("%d %d %s\n", rc, nt, err.c_str());
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "plan")) {
        const int64_t nq = atoll(argv[2]), nr = atoll(argv[3]);
        const NearPlan p = near_plan(nq, nr, atoll(argv[4]), atoll(argv[5]));
        printf("plan %lld %lld %lld\n", (long long)p.q_chunk, (long long)p.r_band, (long long)p.part_rows);
        std::set<std::pair<int64_t, int64_t>> sizes;
        for (int64_t q0 = 0; q0 < nq; q0 += p.q_chunk)
            for (int64_t r0 = 0; r0 < nr; r0 += p.r_band) sizes.insert({std::min(p.q_chunk, nq - q0), std::min(p.r_band, nr - r0)});
        for (const auto &s : sizes) {
            int64_t per = 0, splits = 0;
            near_splits((s.first + kNearQT - 1) / kNearQT, (s.second + kNearRT - 1) / kNearRT, &per, &splits);
            if (splits * s.first > p.part_rows) { fprintf(stderr, "the partial lists are too small\n"); return 1; }
            printf("launch %lld %lld %lld %lld\n", (long long)s.first, (long long)s.second, (long long)per, (long long)splits);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s shape | check model_trees nq nr first_tree n_trees k flags | plan nq nr bytes_per_row scratch_bytes\n", argv[0]);
    return 2;
}
