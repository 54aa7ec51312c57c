// shap_host_check.cpp -- a stand-alone run of the host side of the exact TreeSHAP contributions (ranklib_amd/csrc/rl_shap_host.h: the path
// tables of every leaf, the path limit, the factor tables and the LDS plan of k_model_shap; the argument checks it shares with
// rl_contrib_host.h) on a 6-tree model whose leaf covers are set by hand from a 40-row background: host code only, no device.
//
//   g++ -std=c++17 -ffp-contract=off tools/shap_host_check.cpp -o shap_host_check        (tests/test_shap_cpu.py builds and reads it)
//   g++ -std=c++17 -ffp-contract=off -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/shap_host_check.cpp -o shap_host_check
//   ./shap_host_check
//
// Per tree it prints the nodes and the leaves' covers, then per leaf "leaf <node> <out bits> <d>" and per element
// "elem <feature> <slot> <z bits> <threshold bits>:<goes left> ..." under the columns (7, 2), and "max <longest element list> <leaf> <node>";
// then the tables' bit patterns, one line "rc <code> <message>" per argument and path-limit case and the plan for some shapes.  The
// test recomputes the lines with tests/shap_restatement.py and compares bit for bit.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_shap_host.h"

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

// a right chain of `depth` splits on the features first, first + 1, ...; every `period`-th split repeats the feature of the split before it
static HostTree chain(int depth, int first, int period)
{
    HostTree t;
    t.n_nodes = 2 * depth + 1;
    int f = first - 1;
    for (int k = 0; k < depth; k++) {                              // node 2k is a split: left the leaf 2k + 1, right 2k + 2 (pre-order)
        if (!(period && k % period == period - 1)) f++;
        t.feature.push_back(f); t.threshold.push_back(0.5f); t.left.push_back(2 * k + 1); t.right.push_back(2 * k + 2); t.output.push_back(0.f);
        t.feature.push_back(-1); t.threshold.push_back(0.f); t.left.push_back(-1); t.right.push_back(-1); t.output.push_back((float)k);
    }
    t.feature.push_back(-1); t.threshold.push_back(0.f); t.left.push_back(-1); t.right.push_back(-1); t.output.push_back(-1.f);
    return t;
}

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
static uint32_t bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

int main()
{
    // 40 background rows: every tree's leaves hold 40 between them; tree 3's right subtree holds none (both sides of the a + b == 0 rule
    // and zero-cover children), tree 2 and tree 3 repeat a feature on a path, tree 4 is a single leaf, tree 5 sends everything left
    const std::vector<std::vector<N>> model = {
        {{1, 0.0f, 1, 2, 0, 0}, {-1, 0, -1, -1, -1.0f, 30}, {-1, 0, -1, -1, 3.0f, 10}},
        {{2, 0.5f, 1, 4, 0, 0}, {7, -1.0f, 2, 3, 0, 0}, {-1, 0, -1, -1, 0.1f, 7}, {-1, 0, -1, -1, -0.3f, 13}, {-1, 0, -1, -1, 1e-3f, 20}},
        {{7, 1.5f, 1, 2, 0, 0}, {-1, 0, -1, -1, 0.7f, 1}, {3, 0.25f, 3, 4, 0, 0}, {7, 2.5f, 5, 6, 0, 0}, {-1, 0, -1, -1, -7.0f, 1},
         {-1, 0, -1, -1, 2.5f, 35}, {-1, 0, -1, -1, 0.25f, 3}},
        {{2, -0.5f, 1, 2, 0, 0}, {-1, 0, -1, -1, 0.3f, 40}, {9, 0.0f, 3, 6, 0, 0}, {2, 1.0f, 4, 5, 0, 0}, {-1, 0, -1, -1, 1.1f, 0},
         {-1, 0, -1, -1, 0.2f, 0}, {-1, 0, -1, -1, -0.9f, 0}},
        {{-1, 0, -1, -1, 0.123f, 40}},
        {{5, 0.0f, 1, 2, 0, 0}, {-1, 0, -1, -1, 2.0f, 40}, {-1, 0, -1, -1, -2.0f, 0}},
    };
    const std::vector<std::pair<int32_t, int32_t>> sorted = {{2, 1}, {7, 0}};      // columns (7, 2)
    ShapPaths all;
    for (size_t ti = 0; ti < model.size(); ti++) {
        std::vector<uint64_t> cover;
        const HostTree t = make(model[ti], cover);
        printf("tree %zu\n", ti);
        for (int j = 0; j < t.n_nodes; j++)
            printf("node %d %d %08x %d %d %08x %" PRIu64 "\n", j, t.feature[j], bits(t.threshold[j]), t.left[j], t.right[j], bits(t.output[j]),
                   t.feature[j] == -1 ? cover[j] : 0);
        contrib_fill_inner(t, cover.data());
        std::vector<int32_t> slot((size_t)t.n_nodes);
        contrib_node_slots(t, sorted, 2, slot.data());
        ShapPaths p;
        shap_tree_paths(t, cover.data(), slot.data(), p);
        shap_tree_paths(t, cover.data(), slot.data(), all);          // and appended behind the trees before it, as a call builds them
        int leaf = 0;
        for (int j = 0; j < t.n_nodes; j++) {
            if (t.feature[j] != -1) continue;
            const ShapLeaf &lf = p.leaves[(size_t)leaf++];
            printf("leaf %d %016" PRIx64 " %d\n", j, bits(lf.out), lf.d);
            for (int e = 0; e < lf.d; e++) {
                const ShapElem &el = p.elems[(size_t)(lf.el0 + e)];
                printf("elem %d %d %016" PRIx64, el.feat, el.slot, bits(el.z));
                for (int k = 0; k < el.nc; k++) printf(" %08x:%d", bits(p.conds[(size_t)(el.c0 + k)].thr), p.conds[(size_t)(el.c0 + k)].left);
                printf("\n");
            }
        }
        int32_t at = -1, node = -1;
        const int32_t longest = shap_tree_max_path(t, &at, &node);
        printf("max %d %d %d\n", longest, at, node);
        if (p.leaf0.size() != 2 || p.leaf0[1] != leaf || all.leaf0.size() != ti + 2) { printf("leaf0 is wrong\n"); return 1; }
    }
    printf("all %zu %zu %zu\n", all.leaves.size(), all.elems.size(), all.conds.size());
    for (size_t i = 0; i < all.leaves.size(); i++)                    // the appended tables index into the shared arrays
        if (all.leaves[i].el0 < 0 || (size_t)(all.leaves[i].el0 + all.leaves[i].d) > all.elems.size()) { printf("el0 is wrong\n"); return 1; }
    for (const ShapElem &el : all.elems)
        if (el.c0 < 0 || el.nc < 1 || (size_t)(el.c0 + el.nc) > all.conds.size()) { printf("c0 is wrong\n"); return 1; }

    const std::vector<double> tb = shap_tables();
    const size_t n = (size_t)kShapT * kShapT;
    printf("P %d\n", kShapP);
    for (int l : {1, 2, 3, 7, 30, 32})
        for (int i : {0, 1, 2, 6, 31})
            if (i < l)
                printf("table %d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", l, i, bits(tb[(size_t)l * kShapT + i]),
                       bits(tb[n + (size_t)l * kShapT + i]), bits(tb[2 * n + (size_t)l * kShapT + i]), bits(tb[3 * n + (size_t)l * kShapT + i]));

    const float X[4] = {0, 1, 2, 3};
    double out[8];
    const int32_t good[3] = {7, 2, 9}, neg[3] = {7, -2, 9}, twice[4] = {7, 2, 9, 2};
    std::string err;
    auto rows = [&](int64_t nt, const void *x, int64_t nd, int32_t stride) {
        err.clear();
        const int rc = contrib_check_rows("rl_model_predict_shap: ", nt, x, nd, stride, err);
        printf("rc %d %s\n", rc, err.c_str());
    };
    auto cols = [&](const int32_t *c, int32_t nc, int64_t scratch, const void *o) {
        err.clear();
        const int rc = contrib_check_columns("rl_model_predict_shap: ", c, nc, scratch, o, err);
        printf("rc %d %s\n", rc, err.c_str());
    };
    rows(5, X, 2, 2); rows(-1, X, 2, 2); rows(5, nullptr, 2, 2); rows(5, X, -1, 2); rows(5, X, 2, 0); rows(0, X, 2, 2); rows(5, X, 0, 2);
    rows(5, X, (int64_t)1 << 31, 2);
    cols(good, 3, 0, out); cols(nullptr, 0, 0, out); cols(good, 3, 0, nullptr); cols(nullptr, -1, 0, out); cols(good, 0, 0, out);
    cols(neg, 3, 0, out); cols(twice, 4, 0, out); cols(good, 3, -1, out); cols(good, 1, 1, out);
    // the path limit: 32 distinct features on a path are taken, 33 are not; 40 splits that repeat every fourth feature are 30 distinct ones
    for (const auto &c : std::vector<std::vector<int>>{{kShapP, 1, 0}, {kShapP + 1, 1, 0}, {40, 3, 4}}) {
        const std::vector<HostTree> trees = {chain(3, 1, 0), chain(c[0], c[1], c[2])};
        int32_t longest = -1;
        err.clear();
        const int rc = shap_check_paths("rl_model_predict_shap: ", trees, &longest, err);
        printf("rc %d %s\n", rc, err.c_str());
        printf("longest %d\n", longest);
    }
    for (int wd : {1, 2, 13, 33})
        for (int64_t slots : {3, 138, 402}) {
            int docs = 0; int64_t per = 0;
            const bool ok = shap_plan(wd, slots, docs, per);
            printf("plan wd %d slots %" PRId64 ": %d docs %d per_pass %" PRId64 " limit64 %" PRId64 "\n", wd, slots, (int)ok, docs, per,
                   shap_slot_limit(wd, 64));
        }
    return 0;
}
