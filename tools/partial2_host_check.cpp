// partial2_host_check.cpp -- a stand-alone run of the host side of two-feature partial dependence (ranklib_amd/csrc/rl_partial2_host.h:
// the argument checks and the plan of a call -- tiles that never straddle a pair, chunks of whole tiles, uses per pair) for given pairs,
// grids and a model file: host code only, no device, run on the CPU.
//
//   g++ -std=c++17 -ffp-contract=off tools/partial2_host_check.cpp ranklib_amd/csrc/rl_model.cpp -o partial2_host_check        (tests/test_partial2_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/partial2_host_check.cpp ranklib_amd/csrc/rl_model.cpp -o partial2_host_check
//   ./partial2_host_check model.txt TA TB chunk 3:-1,0,0.5/5:0.25,inf 7:0/3:1,2
//
// TA, TB: the sides of a tile (the library's are RL_PARTIAL2_TILE_A and _B); chunk: the cells a chunk holds at most (the library derives
// it from scratch_bytes); then one argument per pair, a:values/b:values, which strtof reads (inf, -inf and nan too).  It parses the text
// with model_from_text as rl_model_from_text does, runs partial2_check on the arguments (4 documents of 3 columns stand in for the rows)
// and prints
//   rc <code> <message>                                                        (the plan follows where the code is 0)
//   plan <cells> <chunk> <TA> <TB> <trees> <chunks>
//   chunk <number> <first tile> <tiles> <cells>
//   tile <a> <b> <pair> <first slot in the chunk> <values of a> <values of b> <first cell of the call> <gb> <the TA + TB values' bits, hex> <uses>
// with the base as the first line of tiles, before the first chunk.  tests/test_partial2_cpu.py recomputes the lines with
// tests/partial2_restatement.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_partial2_host.h"

using namespace rl;

// "3:-1,0,0.5": the column and its values, up to `end`
static bool read_axis(const char *p, const char *end, int32_t &col, std::vector<float> &grid)
{
    const char *c = (const char *)memchr(p, ':', (size_t)(end - p));
    if (!c) return false;
    col = atoi(p);
    for (p = c + 1; p < end;) {
        char *stop = nullptr;
        const float v = strtof(p, &stop);
        if (stop == p || stop > end || (stop < end && *stop != ',')) return false;
        grid.push_back(v);
        p = (stop < end) ? stop + 1 : stop;
    }
    return true;
}

static void print_tile(const Partial2Plan &p, int32_t t)
{
    const Partial2Tile &td = p.tiles[(size_t)t];
    printf("tile %d %d %d %d %d %d %d %d", td.col_a, td.col_b, td.pair, td.slot0, td.cnt_a, td.cnt_b, td.cell, td.gb);
    for (int32_t u = 0; u < p.TA + p.TB; u++) {
        uint32_t bits;
        memcpy(&bits, &p.values[(size_t)t * (p.TA + p.TB) + u], 4);
        printf("%s%08x", u ? "," : " ", bits);
    }
    printf(" ");
    for (int32_t k = 0; k < p.n_trees; k++) putchar('0' + p.uses[(size_t)t * p.n_trees + k]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 6) { fprintf(stderr, "usage: %s model.txt TA TB chunk a:value,.../b:value,... ...\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::stringstream text;
    text << in.rdbuf();
    std::vector<HostTree> trees;
    std::string err;
    if (!model_from_text(text.str(), trees, err)) { fprintf(stderr, "model_from_text: %s\n", err.c_str()); return 1; }
    const int32_t TA = atoi(argv[2]), TB = atoi(argv[3]), chunk = atoi(argv[4]);
    if (TA < 1 || TB < 1 || TA > kPartial2MaxSide || TB > kPartial2MaxSide || chunk < 1) { fprintf(stderr, "TA and TB must be 1 .. 255, chunk >= 1\n"); return 2; }
    std::vector<int32_t> pairs, off(1, 0);
    std::vector<float> grid;
    for (int i = 5; i < argc; i++) {
        const char *mid = strchr(argv[i], '/'), *end = argv[i] + strlen(argv[i]);
        int32_t a = 0, b = 0;
        if (!mid || !read_axis(argv[i], mid, a, grid)) { fprintf(stderr, "%s: not a:values/b:values\n", argv[i]); return 2; }
        off.push_back((int32_t)grid.size());
        if (!read_axis(mid + 1, end, b, grid)) { fprintf(stderr, "%s: not a:values/b:values\n", argv[i]); return 2; }
        off.push_back((int32_t)grid.size());
        pairs.push_back(a);
        pairs.push_back(b);
    }
    grid.push_back(0.f);                                       // (never an empty buffer: the check names what is wrong)
    const float X[12] = {0};
    double mean = 0, shift2 = 0;
    const int rc = partial2_check("who: ", X, 4, 3, pairs.data(), (int32_t)pairs.size() / 2, off.data(), grid.data(), 0, &mean, &shift2, err);
    printf("rc %d %s\n", rc, err.c_str());
    if (rc) return 0;
    const Partial2Plan p = partial2_plan(trees, pairs.data(), (int32_t)pairs.size() / 2, off.data(), grid.data(), chunk, TA, TB);
    printf("plan %d %d %d %d %d %d\n", p.n_cells, p.chunk, p.TA, p.TB, p.n_trees, p.chunks());
    print_tile(p, 0);
    for (int32_t ci = 0; ci < p.chunks(); ci++) {
        printf("chunk %d %d %d %d\n", ci, p.first[(size_t)ci], p.first[(size_t)ci + 1] - p.first[(size_t)ci], p.slots[(size_t)ci]);
        for (int32_t t = p.first[(size_t)ci]; t < p.first[(size_t)ci + 1]; t++) print_tile(p, t);
    }
    return 0;
}
