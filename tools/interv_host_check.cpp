// interv_host_check.cpp -- a stand-alone run of the host side of interventional TreeSHAP (ranklib_amd/csrc/rl_interv_host.h: the table T,
// the checks of the background's arguments, the LDS plan of k_model_interv and the tree chunks of the mask buffer; the path tables without
// covers and the path limit of rl_shap_host.h; the argument checks it shares with rl_contrib_host.h): host code only, no device.
//
//   g++ -std=c++17 -ffp-contract=off tools/interv_host_check.cpp -o interv_host_check        (tests/test_interv_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/interv_host_check.cpp -o interv_host_check
//   ./interv_host_check
//
// It prints "table <p> <q> <bits of T[p][q]>" for every cell of the table's domain and "unused <cells outside it that are not +0.0>";
// "paths <leaves> <elements> <conditions>" of a two-tree model whose path tables are built with null covers; "strides ..." of the mask
// buffer's rows; one line "rc <code> <message>" per argument and path-limit case; the LDS plan for some shapes and the tree chunks for
// some budgets.  The test compares the table with tests/interv_restatement.py's and the other lines with values worked out by hand.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_interv_host.h"

using namespace rl;

static HostTree make(const std::vector<std::vector<float>> &nodes)     // {feature, threshold, left, right, out}
{
    HostTree t;
    t.n_nodes = (int)nodes.size();
    for (const auto &n : nodes) {
        t.feature.push_back((int32_t)n[0]); t.threshold.push_back(n[1]); t.left.push_back((int32_t)n[2]); t.right.push_back((int32_t)n[3]);
        t.output.push_back(n[4]);
    }
    return t;
}

// a right chain of `depth` splits on the features first, first + 1, ...: node 2k is a split with the leaf 2k + 1 on its left (pre-order)
static HostTree chain(int depth, int first)
{
    std::vector<std::vector<float>> nodes;
    for (int k = 0; k < depth; k++) {
        nodes.push_back({(float)(first + k), 0.5f, (float)(2 * k + 1), (float)(2 * k + 2), 0.f});
        nodes.push_back({-1.f, 0.f, -1.f, -1.f, (float)k});
    }
    nodes.push_back({-1.f, 0.f, -1.f, -1.f, -1.f});
    return make(nodes);
}

int main()
{
    const std::vector<double> tb = interv_table();
    int unused = 0;
    for (int p = 0; p < kShapT; p++)
        for (int q = 0; q < kShapT; q++) {
            const double v = tb[(size_t)p * kShapT + q];
            uint64_t b;
            memcpy(&b, &v, 8);
            if (p >= 1 && p + q <= kShapP) printf("table %d %d %016" PRIx64 "\n", p, q, b);
            else unused += b != 0;
        }
    printf("unused %d\n", unused);

    // tools/shap_host_check.cpp's third tree (feature 7 twice on two of its paths) and a single leaf, under the columns (7, 2): no covers
    const std::vector<HostTree> two = {make({{7, 1.5f, 1, 2, 0}, {-1, 0, -1, -1, 0.7f}, {3, 0.25f, 3, 4, 0}, {7, 2.5f, 5, 6, 0}, {-1, 0, -1, -1, -7.0f},
                                             {-1, 0, -1, -1, 2.5f}, {-1, 0, -1, -1, 0.25f}}),
                                       make({{-1, 0, -1, -1, 0.123f}})};
    const std::vector<std::pair<int32_t, int32_t>> sorted = {{2, 1}, {7, 0}};
    ShapPaths paths;
    for (const HostTree &t : two) {
        std::vector<int32_t> slot((size_t)t.n_nodes);
        contrib_node_slots(t, sorted, 2, slot.data());
        shap_tree_paths(t, nullptr, slot.data(), paths);
    }
    printf("paths %zu %zu %zu\n", paths.leaves.size(), paths.elems.size(), paths.conds.size());
    printf("strides %d %d %d %d\n", interv_mask_stride(1), interv_mask_stride(4), interv_mask_stride(5), interv_mask_stride(kIntervMaxBg));

    const std::string w = "rl_model_predict_shap_background: ";
    const float X[4] = {0, 1, 2, 3};
    double out[8];
    const int32_t good[3] = {7, 2, 9}, neg[3] = {7, -2, 9};
    std::string err;
    auto say = [&](int rc) { printf("rc %d %s\n", rc, err.c_str()); err.clear(); };
    say(contrib_check_rows(w, 5, X, 2, 2, err)); say(contrib_check_rows(w, -1, X, 2, 2, err)); say(contrib_check_rows(w, 5, nullptr, 2, 2, err));
    say(contrib_check_rows(w, 5, X, -1, 2, err)); say(contrib_check_rows(w, 5, X, 2, 0, err)); say(contrib_check_rows(w, 0, X, 2, 2, err));
    say(contrib_check_rows(w, 5, X, (int64_t)1 << 31, 2, err)); say(contrib_check_rows(w, 5, X, 0, 2, err));
    say(interv_check_background(w, nullptr, 2, 2, err)); say(interv_check_background(w, X, 0, 2, err)); say(interv_check_background(w, X, -3, 2, err));
    say(interv_check_background(w, X, 2, 0, err)); say(interv_check_background(w, X, kIntervMaxBg, 2, err));
    say(interv_check_background(w, X, kIntervMaxBg + 1, 2, err));
    say(contrib_check_columns(w, good, 3, 0, nullptr, err)); say(contrib_check_columns(w, neg, 3, 0, out, err));
    say(contrib_check_columns(w, good, 3, -1, out, err)); say(contrib_check_columns(w, nullptr, 0, 1, out, err));
    int32_t longest = -1;
    say(shap_check_paths(w, {chain(3, 1), chain(kShapP + 1, 1)}, &longest, err));

    for (int wd : {0, 1, 13, 32})
        for (int64_t slots : {3, 138, 402}) {
            int docs = 0; int64_t per = 0;
            const bool ok = interv_plan(wd, slots, docs, per);
            printf("plan wd %d slots %" PRId64 ": %d docs %d per_pass %" PRId64 "\n", wd, slots, (int)ok, docs, per);
            if (interv_lds_bytes(wd, docs, (int)per) > (size_t)kShapLds) { printf("the plan does not fit\n"); return 1; }
        }
    const std::vector<int32_t> leaf0 = {0, 2, 5, 9, 13, 14, 16};       // six trees of 2, 3, 4, 4, 1 and 2 leaves
    for (const auto &c : std::vector<std::pair<int32_t, int64_t>>{{5, 0}, {5, 632}, {5, 400}, {5, 300}, {5, 1}, {300, 2000}}) {
        printf("chunks %d %" PRId64, c.first, c.second);
        for (int32_t t : interv_tree_chunks(leaf0, c.first, c.second)) printf(" %d", t);
        printf("\n");
    }
    return interv_tree_chunks({}, 5, 0).size() == 1 ? 0 : 1;
}
