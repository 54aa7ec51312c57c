// letor_format_check.cpp -- a stand-alone run of the native LETOR writer (rl_letor_format) for a sanitizer build: host code only, no device.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/letor_format_check.cpp ranklib_amd/csrc/rl_letor.cpp ranklib_amd/csrc/rl_model.cpp -lpthread -o letor_format_check
//   ./letor_format_check
//
// Random rows -- NaN cells, rows without features (row_len 1 and 0), empty descriptions, fractional labels, arbitrary float bit patterns --
// are formatted on several threads through both calls of the needed / buf protocol, read back with rl_letor_parse, and compared cell by
// cell, bit for bit.  Exit status 0 and "ok" when everything agrees.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/rlhip.h"

namespace rl {      // what rl_trainer.hip gives the library
static std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(int code, const std::string &msg) { g_err = msg; return code; }
}  // namespace rl

static int die(const char *what, long long i) { fprintf(stderr, "FAILED: %s (row %lld): %s\n", what, i, rl::g_err.c_str()); return 1; }

int main()
{
    const int64_t n = 40000, stride = 12;
    std::mt19937_64 rng(7);
    std::vector<float> X((size_t)(n * stride)), labels((size_t)n);
    std::vector<int32_t> row_len((size_t)n), qid_len((size_t)n), desc_len((size_t)n);
    std::vector<int64_t> qid_off((size_t)n), desc_off((size_t)n);
    std::string strings;
    for (int64_t i = 0; i < n; i++) {
        row_len[i] = (int32_t)(rng() % (stride + 1));                   // 0 and 1: no features
        for (int64_t f = 0; f < stride; f++) {
            uint32_t b = (uint32_t)rng();
            float v; memcpy(&v, &b, 4);
            if (rng() % 3 == 0) v = (float)((int)(rng() % 4000) - 2000) / 8.0f;
            if (rng() % 5 == 0) v = NAN;
            X[(size_t)(i * stride + f)] = v;
        }
        if (row_len[i] > 1) { float &last = X[(size_t)(i * stride + row_len[i] - 1)]; if (last != last) last = 0.5f; }   // so that the parser sees the row's length
        labels[i] = (float)(rng() % 5) + (rng() % 2 ? 0.7f : 0.f);
        const std::string q = "q" + std::to_string(i / 9), d = (i % 4 == 0) ? std::string() : "#doc" + std::to_string(i);
        qid_off[i] = (int64_t)strings.size(); qid_len[i] = (int32_t)q.size(); strings += q;
        desc_off[i] = (int64_t)strings.size(); desc_len[i] = (int32_t)d.size(); strings += d;
    }
    int64_t need = 0, need2 = 0;
    if (rl_letor_format(X.data(), n, stride, row_len.data(), labels.data(), strings.data(), (int64_t)strings.size(), qid_off.data(), qid_len.data(),
                        desc_off.data(), desc_len.data(), nullptr, 0, &need) != RL_OK || need <= 0) return die("sizing call", -1);
    std::vector<char> small((size_t)need - 1, 'x');                     // one byte short: nothing may be written
    if (rl_letor_format(X.data(), n, stride, row_len.data(), labels.data(), strings.data(), (int64_t)strings.size(), qid_off.data(), qid_len.data(),
                        desc_off.data(), desc_len.data(), small.data(), need - 1, &need2) != RL_OK || need2 != need) return die("short call", -1);
    for (char c : small) if (c != 'x') return die("short call wrote", -1);
    std::vector<char> text((size_t)need);
    if (rl_letor_format(X.data(), n, stride, row_len.data(), labels.data(), strings.data(), (int64_t)strings.size(), qid_off.data(), qid_len.data(),
                        desc_off.data(), desc_len.data(), text.data(), need, &need2) != RL_OK || need2 != need) return die("writing call", -1);
    // bad arguments are refused, not read
    row_len[5] = (int32_t)stride + 1;
    if (rl_letor_format(X.data(), n, stride, row_len.data(), labels.data(), strings.data(), (int64_t)strings.size(), qid_off.data(), qid_len.data(),
                        desc_off.data(), desc_len.data(), text.data(), need, &need2) == RL_OK) return die("row_len past the stride accepted", 5);
    row_len[5] = 3;
    // and back through the parser
    rl_letor *L = nullptr;
    if (rl_letor_parse(text.data(), need, &L) != RL_OK) return die("parse", -1);
    int64_t nd = 0, ns = 0; int32_t mf = 0;
    rl_letor_info(L, &nd, &mf, &ns);
    if (nd != n || ns != 0 || mf >= stride) { fprintf(stderr, "FAILED: %lld lines, %lld slow, max fid %d\n", (long long)nd, (long long)ns, mf); return 1; }
    std::vector<float> back((size_t)(n * stride)), lab((size_t)n);
    std::vector<int32_t> ql((size_t)n), dl((size_t)n);
    std::vector<int64_t> qo((size_t)n), dofs((size_t)n);
    rl_letor_arrays(L, lab.data(), nullptr, qo.data(), ql.data(), dofs.data(), dl.data(), nullptr, nullptr, nullptr);
    if (rl_letor_rows(L, back.data(), stride) != RL_OK) return die("rows", -1);
    for (int64_t i = 0; i < n; i++) {
        if (i == 5) continue;                                           // (its length was changed above)
        if (lab[i] != (float)(int)labels[i]) return die("label", i);
        if (ql[i] != qid_len[i] || memcmp(text.data() + qo[i], strings.data() + qid_off[i], (size_t)ql[i])) return die("qid", i);
        if (dl[i] != desc_len[i] || memcmp(text.data() + dofs[i], strings.data() + desc_off[i], (size_t)dl[i])) return die("description", i);
        for (int64_t f = 1; f < stride; f++) {
            const float want = f < row_len[i] ? X[(size_t)(i * stride + f)] : NAN, got = back[(size_t)(i * stride + f)];
            if (want != want ? got == got : memcmp(&want, &got, 4) != 0) return die("cell", i);
        }
    }
    rl_letor_destroy(L);
    printf("ok: %lld rows, %lld bytes, written and read back bit for bit\n", (long long)n, (long long)need);
    return 0;
}
