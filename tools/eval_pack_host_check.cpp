// eval_pack_host_check.cpp -- a stand-alone run of the host side of the tiled scoring kernel (ranklib_amd/csrc/rl_eval_pack_host.h:
// which models k_model_eval_tiled takes and the packed nodes, walker assignment and walk lengths it walks) on a model file: host code
// only, no device.
//
//   g++ -std=c++17 -ffp-contract=off tools/eval_pack_host_check.cpp ranklib_amd/csrc/rl_model.cpp -o eval_pack_host_check        (tests/test_eval_pack_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/eval_pack_host_check.cpp ranklib_amd/csrc/rl_model.cpp -o eval_pack_host_check
//   ./eval_pack_host_check model.txt deal phased          (deal, phased: 0 or 1, as RLHIP_EVAL_DEAL and RLHIP_EVAL_PHASED set them)
//
// It parses the text with model_from_text as rl_model_from_text does, calls eval_pack and prints
//   shape <trees> <maxn> <docs> <parts> <per> <phases> <ph1> <ph2> <phlast>
//   ok                          or        refused <the rule>
//   maxcol <largest column any node reads>
//   nodes <hex words, [trees][maxn]>
//   perm <hex bytes, [tiles][parts * per]>
//   meta <hex bytes, [tiles][parts * (1 + phases)]>
// tests/eval_pack_restatement.py decodes the lines, checks their structure and replays the kernel's walk on them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_eval_pack_host.h"

using namespace rl;

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s model.txt deal phased\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::stringstream text;
    text << in.rdbuf();
    std::vector<HostTree> trees;
    std::string err;
    if (!model_from_text(text.str(), trees, err)) { fprintf(stderr, "model_from_text: %s\n", err.c_str()); return 1; }
    int maxn = 1;
    for (const HostTree &t : trees) maxn = std::max(maxn, t.n_nodes);
    const EvalPack pk = eval_pack(trees, maxn, atoi(argv[2]) != 0, atoi(argv[3]) != 0);
    printf("shape %zu %d %d %d %d %d %d %d %d\n", trees.size(), maxn, kEvalDocs, kEvalParts, kEvalPer, kEvalPhases, kEvalPh1, kEvalPh2, kEvalPhLast);
    if (pk.ok) printf("ok\n");
    else printf("refused %s\n", pk.why);
    printf("maxcol %d\n", pk.maxcol);
    printf("nodes"); for (unsigned long long w : pk.nodes) printf(" %016llx", w); printf("\n");
    printf("perm"); for (unsigned char b : pk.perm) printf(" %02x", b); printf("\n");
    printf("meta"); for (unsigned char b : pk.meta) printf(" %02x", b); printf("\n");
    return 0;
}
