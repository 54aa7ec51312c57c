// partial_host_check.cpp -- a stand-alone run of the host side of partial dependence (ranklib_amd/csrc/rl_partial_host.h: the argument
// checks and the plan of a call -- chunks of cells, batches that never straddle a column, uses per column) for given columns, grids and
// a model file: host code only, no device.
//
//   g++ -std=c++17 -ffp-contract=off tools/partial_host_check.cpp ranklib_amd/csrc/rl_model.cpp -o partial_host_check        (tests/test_partial_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/partial_host_check.cpp ranklib_amd/csrc/rl_model.cpp -o partial_host_check
//   ./partial_host_check model.txt batch chunk 3:-1,0,0.5 7:0.25 3:inf
//
// batch: the cells a batch holds at most (the library's is RL_PARTIAL_BATCH); chunk: the cells a chunk holds at most (the library
// derives it from scratch_bytes); then one argument per column, its id and its grid values, which strtof reads (inf, -inf and nan too).
// It parses the text with model_from_text as rl_model_from_text does, runs partial_check on the arguments (4 documents of 3 columns
// stand in for the rows) and prints
//   rc <code> <message>                                                        (the plan follows where the code is 0)
//   plan <cells> <chunk> <batch> <trees> <chunks>
//   chunk <number> <first batch> <batches> <first cell> <cells>
//   batch <column> <place in the columns> <first cell in the chunk> <cells> <the values' bits, hex> <uses, one 0 / 1 per tree>
// tests/test_partial_cpu.py recomputes the lines with tests/partial_restatement.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_partial_host.h"

using namespace rl;

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: %s model.txt batch chunk column:value,value,... ...\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::stringstream text;
    text << in.rdbuf();
    std::vector<HostTree> trees;
    std::string err;
    if (!model_from_text(text.str(), trees, err)) { fprintf(stderr, "model_from_text: %s\n", err.c_str()); return 1; }
    const int32_t B = atoi(argv[2]), chunk = atoi(argv[3]);
    if (B < 1 || chunk < 1) { fprintf(stderr, "batch and chunk must be >= 1\n"); return 2; }
    std::vector<int32_t> columns, off(1, 0);
    std::vector<float> grid;
    for (int i = 4; i < argc; i++) {
        const char *p = strchr(argv[i], ':');
        if (!p) { fprintf(stderr, "%s: no ':'\n", argv[i]); return 2; }
        columns.push_back(atoi(argv[i]));
        for (p++; *p;) {
            char *end = nullptr;
            const float v = strtof(p, &end);
            if (end == p) { fprintf(stderr, "%s: not a number at '%s'\n", argv[i], p); return 2; }
            grid.push_back(v);
            p = (*end == ',') ? end + 1 : end;
            if (*end && *end != ',') { fprintf(stderr, "%s: not a number at '%s'\n", argv[i], end); return 2; }
        }
        off.push_back((int32_t)grid.size());
    }
    grid.push_back(0.f);                                       // (never an empty buffer: the check names what is wrong)
    const float X[12] = {0};
    double mean = 0, shift2 = 0;
    const int rc = partial_check("who: ", X, 4, 3, columns.data(), (int32_t)columns.size(), off.data(), grid.data(), 0, &mean, &shift2, err);
    printf("rc %d %s\n", rc, err.c_str());
    if (rc) return 0;
    const PartialPlan p = partial_plan(trees, columns.data(), (int32_t)columns.size(), off.data(), grid.data(), chunk, B);
    printf("plan %d %d %d %d %d\n", p.n_cells, p.chunk, p.B, p.n_trees, p.chunks());
    for (int32_t ci = 0; ci < p.chunks(); ci++) {
        printf("chunk %d %d %d %d %d\n", ci, p.first[(size_t)ci], p.first[(size_t)ci + 1] - p.first[(size_t)ci], p.cell0[(size_t)ci], p.cells_of(ci));
        for (int32_t b = p.first[(size_t)ci]; b < p.first[(size_t)ci + 1]; b++) {
            const PartialBatch &bd = p.batches[(size_t)b];
            printf("batch %d %d %d %d", bd.col, bd.place, bd.cell0, bd.cnt);
            for (int32_t u = 0; u < B; u++) {
                uint32_t bits;
                memcpy(&bits, &p.values[(size_t)b * B + u], 4);
                printf("%s%08x", u ? "," : " ", bits);
            }
            printf(" ");
            for (int32_t t = 0; t < p.n_trees; t++) putchar('0' + p.uses[(size_t)b * p.n_trees + t]);
            printf("\n");
        }
    }
    return 0;
}
