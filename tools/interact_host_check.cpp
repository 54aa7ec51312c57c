// interact_host_check.cpp -- a stand-alone run of the host side of the SHAP interaction values (ranklib_amd/csrc/rl_interact_host.h: the
// per-slot leaf lists, the LDS plan of k_model_interact and the row-chunk rule; the path tables of rl_shap_host.h and the argument checks
// of rl_contrib_host.h under this entry point's name) on hand-built trees: host code only, no device.
//
//   g++ -std=c++17 -ffp-contract=off tools/interact_host_check.cpp -o interact_host_check        (tests/test_interact_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/interact_host_check.cpp -o interact_host_check
//   ./interact_host_check
//
// It prints "leaves <count>" and per leaf "leaf <index> <tree> <d> <slot> ..." under the columns (7, 2, 11), then per conditioned slot
// "list <slot> <leaf>:<tree> ...", the same under columns == NULL's slots, one line "plan ..." per shape, one line "chunk ..." per case
// of the row-chunk rule and one line "rc <code> <message>" per argument case.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_interact_host.h"

using namespace rl;

struct N { int32_t f; float thr; int32_t l, r; float out; };

static HostTree make(const std::vector<N> &nodes)
{
    HostTree t;
    t.n_nodes = (int)nodes.size();
    for (const N &n : nodes) {
        t.feature.push_back(n.f); t.threshold.push_back(n.thr); t.left.push_back(n.l); t.right.push_back(n.r); t.output.push_back(n.out);
    }
    return t;
}

static bool lists_of(const std::vector<std::vector<N>> &model, const std::vector<std::pair<int32_t, int32_t>> &sorted, int32_t C, const char *tag)
{
    ShapPaths p;
    for (const auto &nodes : model) {
        const HostTree t = make(nodes);
        std::vector<uint64_t> cover((size_t)t.n_nodes, 0);
        for (int j = 0; j < t.n_nodes; j++) cover[(size_t)j] = t.feature[(size_t)j] == -1 ? 5 : 0;
        contrib_fill_inner(t, cover.data());
        std::vector<int32_t> slot((size_t)t.n_nodes);
        contrib_node_slots(t, sorted, C, slot.data());
        shap_tree_paths(t, cover.data(), slot.data(), p);
    }
    printf("%s leaves %zu\n", tag, p.leaves.size());
    for (size_t t = 0; t + 1 < p.leaf0.size(); t++)
        for (int32_t lf = p.leaf0[t]; lf < p.leaf0[t + 1]; lf++) {
            printf("%s leaf %d %zu %d", tag, lf, t, p.leaves[(size_t)lf].d);
            for (int e = 0; e < p.leaves[(size_t)lf].d; e++) printf(" %d", p.elems[(size_t)(p.leaves[(size_t)lf].el0 + e)].slot);
            printf("\n");
        }
    const InteractLists il = interact_lists(p, C);
    if (il.list0.size() != (size_t)C + 2 || il.list0[0] != 0 || (size_t)il.list0.back() != il.list.size()) { printf("list0 is wrong\n"); return false; }
    for (int32_t s = 0; s <= C; s++) {
        printf("%s list %d", tag, s);
        for (int32_t k = il.list0[(size_t)s]; k < il.list0[(size_t)s + 1]; k++) {
            const InteractLeaf &en = il.list[(size_t)k];
            if (en.leaf < 0 || (size_t)en.leaf >= p.leaves.size() || en.leaf < p.leaf0[(size_t)en.tree] || en.leaf >= p.leaf0[(size_t)en.tree + 1]) {
                printf(" the entry is wrong\n");
                return false;
            }
            printf(" %d:%d", en.leaf, en.tree);
        }
        printf("\n");
    }
    return true;
}

int main()
{
    // tree 0: a stump on 7 (leaves of one element: in no list); tree 1: 2 above 7 left, a leaf right; tree 2: 7, then 3, then 7 again
    // (a repeated feature is one element) and 9 below: rest holds two elements of one leaf; tree 3: a single leaf; tree 4: 11 above 2
    const std::vector<std::vector<N>> model = {
        {{7, 0.0f, 1, 2, 0}, {-1, 0, -1, -1, -1.0f}, {-1, 0, -1, -1, 3.0f}},
        {{2, 0.5f, 1, 4, 0}, {7, -1.0f, 2, 3, 0}, {-1, 0, -1, -1, 0.1f}, {-1, 0, -1, -1, -0.3f}, {-1, 0, -1, -1, 1e-3f}},
        {{7, 1.5f, 1, 2, 0}, {-1, 0, -1, -1, 0.7f}, {3, 0.25f, 3, 4, 0}, {7, 2.5f, 5, 6, 0}, {-1, 0, -1, -1, -7.0f}, {-1, 0, -1, -1, 2.5f},
         {9, 0.f, 7, 8, 0}, {-1, 0, -1, -1, 0.25f}, {-1, 0, -1, -1, 0.5f}},
        {{-1, 0, -1, -1, 0.123f}},
        {{11, 0.0f, 1, 2, 0}, {-1, 0, -1, -1, 2.0f}, {2, 1.0f, 3, 4, 0}, {-1, 0, -1, -1, -2.0f}, {-1, 0, -1, -1, 4.0f}},
    };
    if (!lists_of(model, {{2, 1}, {7, 0}, {11, 2}}, 3, "some")) return 1;                 // columns (7, 2, 11): 3 and 9 are in rest
    if (!lists_of(model, {{2, 0}, {3, 1}, {7, 2}, {9, 3}, {11, 4}}, 5, "all")) return 1;   // columns == NULL: rest stays empty
    if (!lists_of({model[3]}, {{1, 0}}, 1, "leaf")) return 1;                              // single leaves only: every list is empty

    for (int longest : {0, 1, 2, 13, 32})
        for (int64_t slots : {2, 137, 401}) {                             // the attributed slots C + 1
            int docs = 0; int64_t per = 0;
            const int wr = interact_w_rows(longest);
            const bool ok = interact_plan(wr, slots, docs, per);
            printf("plan longest %d wr %d slots %" PRId64 ": %d docs %d per_pass %" PRId64 " limit64 %" PRId64 " limit128 %" PRId64 " limit256 %" PRId64 "\n",
                   longest, wr, slots, (int)ok, docs, per, interact_slot_limit(wr, 64), interact_slot_limit(wr, 128), interact_slot_limit(wr, 256));
        }
    // the row-chunk rule: n_docs, row_stride, C, scratch_bytes
    for (const auto &c : std::vector<std::vector<int64_t>>{{257, 35, 12, 0}, {257, 35, 12, 100 * (35 * 4 + 8 * 14 * 14 + 8 * 14)},
                                                          {257, 35, 12, 100 * (35 * 4 + 8 * 14 * 14 + 8 * 14) - 1}, {5, 35, 12, 1}, {0, 35, 12, 0},
                                                          {1000000, 137, 136, 0}, {1000000, 137, 136, (int64_t)1 << 30}, {3, 1, 65534, 0}})
        printf("chunk %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 ": %" PRId64 " rows of %" PRId64 " bytes\n", c[0], c[1], c[2], c[3],
               interact_chunk_rows(c[0], (int32_t)c[1], c[2], c[3]), interact_row_bytes((int32_t)c[1], c[2]));

    const float X[4] = {0, 1, 2, 3};
    double out[32];
    const int32_t good[3] = {7, 2, 9}, neg[3] = {7, -2, 9}, twice[4] = {7, 2, 9, 2};
    const std::string w = "rl_model_predict_interactions: ";
    std::string err;
    auto rows = [&](int64_t nt, const void *x, int64_t nd, int32_t stride) {
        err.clear();
        const int rc = contrib_check_rows(w, nt, x, nd, stride, err);
        printf("rc %d %s\n", rc, err.c_str());
    };
    auto cols = [&](const int32_t *c, int32_t nc, int64_t scratch, const void *o) {
        err.clear();
        const int rc = contrib_check_columns(w, c, nc, scratch, o, err);
        printf("rc %d %s\n", rc, err.c_str());
    };
    rows(5, X, 2, 2); rows(-1, X, 2, 2); rows(5, nullptr, 2, 2); rows(5, X, -1, 2); rows(5, X, 2, 0); rows(0, X, 2, 2); rows(5, X, 0, 2);
    rows(5, X, (int64_t)1 << 31, 2);
    cols(good, 3, 0, out); cols(nullptr, 0, 0, out); cols(good, 3, 0, nullptr); cols(nullptr, -1, 0, out); cols(good, 0, 0, out);
    cols(neg, 3, 0, out); cols(twice, 4, 0, out); cols(good, 3, -1, out); cols(good, 1, 1, out);
    for (int64_t C : {0, 65534, 65535}) {                                  // C + 1 conditioned slots
        err.clear();
        const int rc = interact_check_slots(w, C, err);
        printf("rc %d %s\n", rc, err.c_str());
    }
    // the path limit is rl_shap_host.h's: a right chain of 33 distinct features is refused under this entry point's name
    for (int depth : {kShapP, kShapP + 1}) {
        HostTree t;
        t.n_nodes = 2 * depth + 1;
        for (int k = 0; k < depth; k++) {
            t.feature.push_back(k + 1); t.threshold.push_back(0.5f); t.left.push_back(2 * k + 1); t.right.push_back(2 * k + 2); t.output.push_back(0.f);
            t.feature.push_back(-1); t.threshold.push_back(0.f); t.left.push_back(-1); t.right.push_back(-1); t.output.push_back((float)k);
        }
        t.feature.push_back(-1); t.threshold.push_back(0.f); t.left.push_back(-1); t.right.push_back(-1); t.output.push_back(-1.f);
        int32_t longest = -1;
        err.clear();
        const int rc = shap_check_paths(w, {t}, &longest, err);
        printf("rc %d %s\n", rc, err.c_str());
        printf("longest %d\n", longest);
    }
    return 0;
}
