// contrib_host_check.cpp -- a stand-alone run of the host side of the feature contributions (ranklib_amd/csrc/rl_contrib_host.h: the
// argument checks, contrib_fill_inner, contrib_node_values, contrib_node_slots and the LDS plan) on a 5-tree model whose leaf covers are
// set by hand from a 40-row background: host code only, no device.
//
//   g++ -std=c++17 -ffp-contract=off tools/contrib_host_check.cpp -o contrib_host_check        (tests/test_contribs_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/contrib_host_check.cpp -o contrib_host_check
//   ./contrib_host_check
//
// Per tree it prints the nodes and the leaves' covers, then what the header made of them: the covers of all nodes, the node values as
// the doubles' bit patterns in hexadecimal and the slots under the columns (7, 2); then one line "rc <code> <message>" per argument case
// and the plan for three model shapes.  The test recomputes the trees' lines with tests/contrib_restatement.py and compares bit for bit.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_contrib_host.h"

using namespace rl;

struct N { int32_t f; float thr; int32_t l, r; float out; uint64_t leaf_cover; };

static HostTree make(const std::vector<N> &nodes, std::vector<uint64_t> &cover)
{
    HostTree t;
    t.n_nodes = (int)nodes.size();
    for (const N &n : nodes) {
        t.feature.push_back(n.f); t.threshold.push_back(n.thr); t.left.push_back(n.l); t.right.push_back(n.r); t.output.push_back(n.out);
        cover.push_back(n.f == -1 ? n.leaf_cover : 12345);      // an inner node's entry is overwritten whatever it held
    }
    return t;
}

int main()
{
    // 40 background rows: every tree's leaves hold 40 between them, tree 3's right subtree holds none, tree 4 is a single leaf
    const std::vector<std::vector<N>> model = {
        {{1, 0.0f, 1, 2, 0, 0}, {-1, 0, -1, -1, -1.0f, 30}, {-1, 0, -1, -1, 3.0f, 10}},
        {{2, 0.5f, 1, 4, 0, 0}, {7, -1.0f, 2, 3, 0, 0}, {-1, 0, -1, -1, 0.1f, 7}, {-1, 0, -1, -1, -0.3f, 13}, {-1, 0, -1, -1, 1e-3f, 20}},
        {{7, 1.5f, 1, 2, 0, 0}, {-1, 0, -1, -1, 0.7f, 1}, {3, 0.25f, 3, 4, 0, 0}, {-1, 0, -1, -1, 2.5f, 38}, {-1, 0, -1, -1, -7.0f, 1}},
        {{2, -0.5f, 1, 2, 0, 0}, {-1, 0, -1, -1, 0.3f, 40}, {9, 0.0f, 3, 6, 0, 0}, {2, 1.0f, 4, 5, 0, 0}, {-1, 0, -1, -1, 1.1f, 0},
         {-1, 0, -1, -1, 0.2f, 0}, {-1, 0, -1, -1, -0.9f, 0}},
        {{-1, 0, -1, -1, 0.123f, 40}},
    };
    const std::vector<std::pair<int32_t, int32_t>> sorted = {{2, 1}, {7, 0}};      // columns (7, 2)
    for (size_t ti = 0; ti < model.size(); ti++) {
        std::vector<uint64_t> cover;
        const HostTree t = make(model[ti], cover);
        printf("tree %zu\n", ti);
        for (int j = 0; j < t.n_nodes; j++) {
            uint32_t tb, ob;
            memcpy(&tb, &t.threshold[j], 4); memcpy(&ob, &t.output[j], 4);
            printf("node %d %d %08x %d %d %08x %" PRIu64 "\n", j, t.feature[j], tb, t.left[j], t.right[j], ob, t.feature[j] == -1 ? cover[j] : 0);
        }
        contrib_fill_inner(t, cover.data());
        std::vector<double> val((size_t)t.n_nodes);
        contrib_node_values(t, cover.data(), val.data());
        std::vector<int32_t> slot((size_t)t.n_nodes);
        contrib_node_slots(t, sorted, 2, slot.data());
        printf("cover"); for (uint64_t c : cover) printf(" %" PRIu64, c); printf("\n");
        printf("value"); for (double v : val) { uint64_t b; memcpy(&b, &v, 8); printf(" %016" PRIx64, b); } printf("\n");
        printf("slot"); for (int32_t s : slot) printf(" %d", s); printf("\n");
    }
    const float X[4] = {0, 1, 2, 3};
    double out[8];
    const int32_t good[3] = {7, 2, 9}, neg[3] = {7, -2, 9}, twice[4] = {7, 2, 9, 2};
    std::string err;
    auto rows = [&](int64_t nt, const void *x, int64_t n, int32_t stride) {
        err.clear();
        const int rc = contrib_check_rows("who: ", nt, x, n, stride, err);
        printf("rc %d %s\n", rc, err.c_str());
    };
    auto cols = [&](const int32_t *c, int32_t nc, int64_t scratch, const void *o) {
        err.clear();
        const int rc = contrib_check_columns("who: ", c, nc, scratch, o, err);
        printf("rc %d %s\n", rc, err.c_str());
    };
    rows(5, X, 2, 2); rows(-1, X, 2, 2); rows(5, nullptr, 2, 2); rows(5, X, -1, 2); rows(5, X, 2, 0); rows(0, X, 2, 2); rows(5, X, 0, 2);
    rows(5, X, (int64_t)1 << 31, 2);
    cols(good, 3, 0, out); cols(nullptr, 0, 0, out); cols(good, 3, 0, nullptr); cols(nullptr, -1, 0, out); cols(good, 0, 0, out);
    cols(neg, 3, 0, out); cols(twice, 4, 0, out); cols(good, 3, -1, out); cols(good, 1, 1, out);
    for (int maxn : {3, 61, 5103, 5104}) {
        int docs = 0; int64_t per = 0;
        for (int64_t slots : {3, 138, 402}) {
            const bool ok = contrib_plan(maxn, slots, docs, per);
            printf("plan maxn %d slots %" PRId64 ": %d tile %d docs %d per_pass %" PRId64 " limit64 %" PRId64 "\n", maxn, slots, (int)ok,
                   contrib_tree_tile(maxn), docs, per, contrib_slot_limit(maxn, 64));
        }
    }
    return 0;
}
