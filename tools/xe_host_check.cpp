// xe_host_check.cpp -- a stand-alone run of the host side of the XE-NDCG objective (ranklib_amd/csrc/rl_xe_host.h: the tile size in force and the
// block table of k_lambda_xe): host code only, no device, run on the CPU.
//
//   g++ -std=c++17 tools/xe_host_check.cpp -o xe_host_check                                       (tests/test_xe_cpu.py builds and reads it)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/xe_host_check.cpp -o xe_host_check
//   ./xe_host_check tile len_0 len_1 ...
//
// Prints the tile size in force, then one line "q0 nq" per block of the lists of the given lengths.
#include <cstdio>
#include <cstdlib>

#include "../ranklib_amd/csrc/rl_xe_host.h"

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: xe_host_check tile len_0 [len_1 ...]\n"); return 2; }
    std::vector<int32_t> qoff{0};
    for (int i = 2; i < argc; i++) qoff.push_back(qoff.back() + atoi(argv[i]));
    const int tile = rl::xe_tile(atoi(argv[1]));
    std::vector<rl::XeBlock> blocks;
    rl::xe_pack(qoff.data(), (int32_t)qoff.size() - 1, tile, blocks);
    printf("tile %d\n", tile);
    for (const rl::XeBlock &b : blocks) printf("%d %d\n", b.q0, b.nq);
    return 0;
}
