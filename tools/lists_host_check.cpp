// lists_host_check.cpp -- a stand-alone run of the host side of a set of ranked lists (ranklib_amd/csrc/rl_lists_host.h: check_lists,
// ListSetHost, ideal_cache) and of eval_prepare_lists (rl_eval_host.h) over a fixed table of cases: host code only, no device.
//
//   g++ -std=c++17 tools/lists_host_check.cpp -o lists_host_check                 (tests/test_lists_host_cpu.py builds and reads it)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lists_host_check.cpp -o lists_host_check
//   ./lists_host_check
//
// Every case prints its inputs, then what the header made of them: "rc <code> <message>", and for the ideal DCGs one line per set and
// output, own<s> / cached<s> (ideal_cache) and prep0 (eval_prepare_lists), as the doubles' bit patterns in hexadecimal.  The test
// recomputes each case from the printed inputs with ranklib_amd.metric.NDCGScorer and compares bit for bit.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ranklib_amd/csrc/rl_eval_host.h"
#include "../ranklib_amd/csrc/rl_lists_host.h"

using namespace rl;

struct Set {
    std::vector<float> labels; std::vector<int32_t> qoff, qkey;     // qkey empty: none
    std::vector<double> ext;                                        // empty: no external table
};

static const double kNone = std::nan("");

static void print_bits(const char *what, int s, const std::vector<double> &v)
{
    printf("%s%d", what, s);
    for (double x : v) { uint64_t b; memcpy(&b, &x, 8); printf(" %016" PRIx64, b); }
    printf("\n");
}

static void print_set(int s, const Set &d)
{
    printf("qoff%d", s); for (int32_t v : d.qoff) printf(" %d", v); printf("\n");
    printf("labels%d", s); for (float v : d.labels) printf(" %.9g", (double)v); printf("\n");
    if (!d.qkey.empty()) { printf("qkey%d", s); for (int32_t v : d.qkey) printf(" %d", v); printf("\n"); }
    if (!d.ext.empty()) { printf("ext%d", s); for (double v : d.ext) printf(" %.17g", v); printf("\n"); }
}

static int load(const Set &d, ListSetHost &h)
{
    const int32_t Q = (int32_t)d.qoff.size() - 1;
    std::string err;
    const int rc = check_lists("", d.labels.data(), (int64_t)d.labels.size(), d.qoff.data(), Q, err);
    if (rc) { printf("rc %d %s\n", rc, err.c_str()); return rc; }
    h.store(d.labels.data(), (int64_t)d.labels.size(), d.qoff.data(), Q, d.qkey.empty() ? nullptr : d.qkey.data());
    return h.set_external(d.ext.empty() ? nullptr : d.ext.data(), nullptr, err);
}

// rule: "trainer" = min(n, k) (rl_init), "eval" = (k > n || k <= 0) ? n : k (everything else; eval_prepare_lists is run beside it)
static void ideal_case(const char *name, const Set &train, const Set *valid, int k, const char *rule)
{
    printf("case %s k=%d rule=%s\n", name, k, rule);
    print_set(0, train);
    if (valid) print_set(1, *valid);
    ListSetHost tr, va;
    if (load(train, tr) || (valid && load(*valid, va))) return;
    printf("rc 0\n");
    const std::vector<double> disc = discount_table(std::max(tr.maxq, valid ? va.maxq : 0));
    std::vector<double> own[2], cached[2];
    if (!strcmp(rule, "trainer")) ideal_cache(tr, valid ? &va : nullptr, disc, [k](int n) { return std::min(n, k); }, cached, own);
    else ideal_cache(tr, valid ? &va : nullptr, disc, [k](int n) { return (k > n || k <= 0) ? n : k; }, cached, own);
    for (int s = 0; s < (valid ? 2 : 1); s++) { print_bits("own", s, own[s]); print_bits("cached", s, cached[s]); }
    if (!strcmp(rule, "eval") && !valid) {
        std::vector<double> ideal, d2; std::string err; double out = 0;
        const int rc = eval_prepare_lists("prep", RL_METRIC_NDCG, k, 16.0, nullptr, train.labels.data(), (int64_t)train.labels.size(),
                                          train.qoff.data(), tr.Q, train.qkey.empty() ? nullptr : train.qkey.data(),
                                          train.ext.empty() ? nullptr : train.ext.data(), nullptr, &out, ideal, d2, err);
        if (rc) printf("prep rc %d %s\n", rc, err.c_str()); else print_bits("prep", 0, ideal);
    }
}

static void refusal_case(const char *name, const char *who, const std::vector<float> &labels, const std::vector<int32_t> &qoff)
{
    std::string err;
    const int rc = check_lists(who, labels.data(), (int64_t)labels.size(), qoff.data(), (int32_t)qoff.size() - 1, err);
    printf("case %s\nrc %d %s\n", name, rc, err.c_str());
}

int main()
{
    // a, b, c: two sets of two lists; the key 7 is shared across the sets and its two lists carry different labels
    Set tr{{3, 1, 0, 2, 2}, {0, 3, 5}, {7, 8}, {}}, va{{1, 0, 0, 1, 4, 0}, {0, 4, 6}, {7, 9}, {}};
    ideal_case("a", tr, &va, 10, "eval");
    ideal_case("a.trainer", tr, &va, 10, "trainer");
    Set tr_b = tr, va_b = va;
    tr_b.qkey.clear(); va_b.qkey.clear();
    ideal_case("b", tr_b, &va_b, 10, "eval");
    ideal_case("b.trainer", tr_b, &va_b, 10, "trainer");
    Set tr_c = tr, va_c = va;
    tr_c.ext = {2.5, kNone}; va_c.ext = {kNone, kNone};
    ideal_case("c", tr_c, &va_c, 10, "eval");
    ideal_case("c.trainer", tr_c, &va_c, 10, "trainer");
    ideal_case("c.one_set", tr_c, nullptr, 10, "eval");
    // d: lists of 1, 3 and 12 documents around the cut-off
    Set d{{2, 0, 3, 1, 1, 0, 2, 4, 0, 3, 1, 2, 0, 1, 3, 2}, {0, 1, 4, 16}, {}, {}};
    for (int k : {10, 3, 0})
        for (const char *rule : {"trainer", "eval"}) ideal_case(("d.k" + std::to_string(k) + "." + rule).c_str(), d, nullptr, k, rule);
    // e: (int) casts and Java int gains: 1.7 -> 1, (1 << 31) - 1, 1 << 32 wraps to 1 << 0, 16777215 & 31 == 31
    Set e{{0, 1.7f, 31, 32, 33, 16777215, 0, 1.7f, 31, 32, 33, 16777215}, {0, 6, 7, 8, 9, 10, 11, 12}, {}, {}};
    ideal_case("e", e, nullptr, 10, "eval");
    ideal_case("e.trainer", e, nullptr, 10, "trainer");
    // f: one refusal per rule, the offending list not the first
    const std::vector<float> five{1, 0, 2, 0, 1};
    refusal_case("f.start", "", five, {1, 2, 5});
    refusal_case("f.empty", "rl_x", five, {0, 2, 2, 5});
    refusal_case("f.past", "", five, {0, 2, 7, 5});
    refusal_case("f.end", "rl_x", five, {0, 2, 4});
    refusal_case("f.negative", "", {1, 0, 2, -1, 1}, {0, 2, 5});
    refusal_case("f.nan", "rl_x", {1, 0, 2, std::nanf(""), 1}, {0, 2, 5});
    refusal_case("f.big", "", {1, 0, 2, 16777216.f, 1}, {0, 2, 5});
    {
        ListSetHost h; std::string err;
        h.store(five.data(), 5, std::vector<int32_t>{0, 2, 5}.data(), 2, nullptr);
        const int32_t rd[2] = {1, -1};
        const int rc = h.set_external(nullptr, rd, err);
        printf("case f.rd\nrc %d %s\n", rc, err.c_str());
        std::vector<double> ideal, disc; double out = 0;
        const int32_t qoff[3] = {0, 2, 5};
        const int rc2 = eval_prepare_lists("rl_x", RL_METRIC_MAP, 10, 16.0, nullptr, five.data(), 5, qoff, 2, nullptr, nullptr, rd, &out, ideal, disc, err);
        printf("case f.rd.prep\nrc %d %s\n", rc2, err.c_str());
    }
    return 0;
}
