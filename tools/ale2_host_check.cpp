// ale2_host_check.cpp -- a stand-alone run of the host side of second-order accumulated local effects (ranklib_amd/csrc/rl_ale2_host.h:
// the plan of a call -- chunks of pairs, batches of up to P pairs, two uses bits per pair and tree) for given pairs and a model file:
// host code only, no device, run on the CPU.
//
//   g++ -std=c++17 -ffp-contract=off tools/ale2_host_check.cpp ranklib_amd/csrc/rl_model.cpp -o ale2_host_check        (tests/test_ale2_cpu.py builds and reads it)
//   ./ale2_host_check model.txt P scratch_bytes n_docs corners 3:5:10:10 5:3:4:2
//
// P: the pairs of a batch (the library's is RL_ALE2_BATCH); scratch_bytes, n_docs and corners (0 / 1: out_corner is asked for) are what
// ale2_chunk_pairs derives the chunk from; then one argument per pair, a:b:Ka:Kb.  It prints
//   plan <cells> <chunk> <chunks> <supers> <max cells of a chunk>
//   chunk <number> <first pair> <pairs> <first batch> <batches>
//   batch <number> <uses of tree 0, hex> <uses of tree 1, hex> ...
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "../ranklib_amd/csrc/rl_ale2_host.h"

using namespace rl;

int main(int argc, char **argv)
{
    if (argc < 7) { fprintf(stderr, "usage: %s model.txt P scratch_bytes n_docs corners a:b:Ka:Kb ...\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::stringstream text;
    text << in.rdbuf();
    std::vector<HostTree> trees;
    std::string err;
    if (!model_from_text(text.str(), trees, err)) { fprintf(stderr, "model_from_text: %s\n", err.c_str()); return 1; }
    const int32_t P = atoi(argv[2]);
    const int64_t scratch = atoll(argv[3]), n_docs = atoll(argv[4]);
    if (P < 1 || P > 16 || n_docs < 1) { fprintf(stderr, "P must be 1 .. 16, n_docs >= 1\n"); return 2; }
    std::vector<int32_t> pairs, off(1, 0);
    for (int i = 6; i < argc; i++) {
        int a = 0, b = 0, ka = 0, kb = 0;
        if (sscanf(argv[i], "%d:%d:%d:%d", &a, &b, &ka, &kb) != 4 || ka < 1 || kb < 1) { fprintf(stderr, "%s: not a:b:Ka:Kb\n", argv[i]); return 2; }
        pairs.push_back(a); pairs.push_back(b);
        off.push_back(off.back() + ka + 1); off.push_back(off.back() + kb + 1);
    }
    const int32_t n_pairs = (int32_t)pairs.size() / 2;
    const int32_t chunk = ale2_chunk_pairs(scratch, (int64_t)256 << 20, n_docs, n_pairs, atoi(argv[5]) != 0, 65535);
    const Ale2Plan p = ale2_plan(trees, pairs.data(), n_pairs, off.data(), chunk, P);
    printf("plan %d %d %d %d %d\n", p.cell_off.back(), p.chunk, p.chunks(), ale2_supers(n_docs, 256), p.max_cells);
    for (int32_t ci = 0; ci < p.chunks(); ci++) {
        const int32_t b0 = p.first[(size_t)ci], b1 = p.first[(size_t)ci + 1];
        printf("chunk %d %d %d %d %d\n", ci, p.pair0(ci), p.pair1(ci) - p.pair0(ci), b0, b1 - b0);
        for (int32_t b = b0; b < b1; b++) {
            printf("batch %d", b);
            for (int32_t t = 0; t < p.n_trees; t++) printf(" %x", p.uses[(size_t)b * p.n_trees + t]);
            printf("\n");
        }
    }
    return 0;
}
