// rl_lists_host.h -- what every entry family states about a set of ranked lists, once: the DCG discount and NDCGScorer.getIdealDCG, the
// host copy of a set (ListSetHost), the list rules (check_lists) and the qid-keyed idealGains cache (ideal_cache).  Plain C++ with no HIP
// in it, like rl_eval_host.h: a stand-alone program can include this file and run it under a host sanitizer (tools/lists_host_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/rlhip.h"

namespace rl {

inline double dcg_discount(int i) { return 1.0 / (std::log((double)(i + 2)) / std::log(2.0)); }   // DCGScorer.java:26

// the discounts of positions 0 .. maxq + 1
inline std::vector<double> discount_table(int maxq)
{
    std::vector<double> disc((size_t)maxq + 2);
    for (size_t i = 0; i < disc.size(); i++) disc[i] = dcg_discount((int)i);
    return disc;
}

inline double ideal_dcg(const float *labels, int n, int topk, const std::vector<double> &disc)
{   // NDCGScorer.getIdealDCG (:167-174): the (int) labels best first
    std::vector<int> rel((size_t)n);
    for (int i = 0; i < n; i++) rel[i] = (int)labels[i];
    std::sort(rel.begin(), rel.end(), [](int a, int b) { return a > b; });
    double dcg = 0;
    for (int i = 0; i < topk; i++) dcg += (double)(int32_t)(((uint32_t)1 << (rel[i] & 31)) - 1u) * disc[i];      // Java int arithmetic (DCGScorer.java:137-139)
    return dcg;
}

// The list rules of every entry point that takes ranked lists.  Returns RL_OK or the error code with its message in err, prefixed by who
// and ": " when who is not empty.  The caller has already refused a null qoff and sizes below 1.
inline int check_lists(const char *who, const float *labels, int64_t n_docs, const int32_t *qoff, int32_t n_lists, std::string &err)
{
    auto bad = [&](int code, const std::string &m) { err = *who ? std::string(who) + ": " + m : m; return code; };
    if (qoff[0] != 0) return bad(RL_ERR_INVALID, "qoff must start at 0");
    for (int32_t q = 0; q < n_lists; q++) {
        if (qoff[q + 1] <= qoff[q])
            return bad(RL_ERR_INVALID, "qoff must be strictly increasing (empty ranked list " + std::to_string(q) + ")");
        if ((int64_t)qoff[q + 1] > n_docs) return bad(RL_ERR_INVALID, "qoff must end at n_docs (list " + std::to_string(q) + " runs past it)");
    }
    if ((int64_t)qoff[n_lists] != n_docs) return bad(RL_ERR_INVALID, "qoff must end at n_docs");
    for (int64_t i = 0; labels && i < n_docs; i++) {      // (labels == nullptr: a caller without labels, rl_normalize_lists)
        if (!(labels[i] >= 0)) return bad(RL_ERR_INVALID, "Relevance label cannot be negative. System will now exit.");  // DataPoint.java:71-73
        // labels above 30 are legal: the gain (1 << l) - 1 wraps as Java ints do.  The Java keeps a gain cache of l + 10 doubles
        // (DCGScorer.java:131-140), so a label near 2^31 ends in an OutOfMemoryError there; the line is drawn where (int)label is exact
        if (labels[i] >= 16777216.f) return bad(RL_ERR_UNSUPPORTED, "relevance label of 2^24 or more");
    }
    return RL_OK;
}

// The host side of one set of ranked lists (already checked by check_lists)
struct ListSetHost {
    int64_t N = 0; int32_t Q = 0, maxq = 0;
    std::vector<float> labels; std::vector<int32_t> qoff, qkey; bool has_key = false;
    // -qrel: per list, the idealGains entry of its qid in the judgment file (NaN = none) and its relDocCount; empty = not given
    std::vector<double> ext_ideal; std::vector<int32_t> ext_rd;

    void store(const float *labels_, int64_t n, const int32_t *qoff_, int32_t Q_, const int32_t *qkey_)
    {
        N = n; Q = Q_;
        labels.assign(labels_, labels_ + n);
        qoff.assign(qoff_, qoff_ + Q_ + 1);
        has_key = qkey_ != nullptr;
        if (qkey_) qkey.assign(qkey_, qkey_ + Q_); else qkey.clear();
        maxq = 0;
        for (int32_t q = 0; q < Q_; q++) maxq = std::max(maxq, qoff_[q + 1] - qoff_[q]);
        ext_ideal.clear(); ext_rd.clear();
    }

    // either table may be null (= not given).  Returns RL_OK or the code with the bare message in err
    int set_external(const double *ideal, const int32_t *rel_doc_count, std::string &err)
    {
        ext_ideal.clear(); ext_rd.clear();
        if (ideal) ext_ideal.assign(ideal, ideal + Q);
        if (rel_doc_count) {
            for (int32_t q = 0; q < Q; q++) if (rel_doc_count[q] < 0) { err = "negative relevant-document count"; return RL_ERR_INVALID; }
            ext_rd.assign(rel_doc_count, rel_doc_count + Q);
        }
        return RL_OK;
    }
};

// The ideal DCG every list is scored against, with the qid-keyed cache quirk of NDCGScorer (idealGains, NDCGScorer.java:114-122,134-143:
// one entry per list id, whatever a later list's labels are).  The cache is filled in this order:
//   1. the external (-qrel) entries of both sets that are not NaN: NDCGScorer.loadExternalRelevanceJudgment fills idealGains BEFORE any
//      list is scored (:50-96), so such an entry wins for every list of its key, in both sets;
//   2. the training lists in order, then the validation lists (valid may be null): score() fills the cache in list order, the FIRST list
//      of a key decides.
// A set without qkey has anonymous keys, one per list, from 1 << 40 (training) and 1 << 41 (validation): list q of the one never shares a
// key with list q of the other.  size_of(n) is the caller's cut-off for a list of n documents.
// cached and own point to one vector per set (training, then validation when there is one).  cached[s][q] is the cache's entry for list
// q of set s; with own != nullptr, own[s][q] is the list's own ideal (the external entry where there is one).
template <class SizeOf>
inline void ideal_cache(const ListSetHost &train, const ListSetHost *valid, const std::vector<double> &disc, SizeOf size_of,
                        std::vector<double> *cached, std::vector<double> *own = nullptr)
{
    const ListSetHost *sets[2] = {&train, valid};
    const int64_t anon[2] = {(int64_t)1 << 40, (int64_t)1 << 41};
    auto key_of = [&](int s, int32_t q) { return sets[s]->has_key ? (int64_t)sets[s]->qkey[q] : anon[s] + q; };
    std::map<int64_t, double> cache;
    for (int s = 0; s < 2; s++)
        for (int32_t q = 0; sets[s] && q < sets[s]->Q && !sets[s]->ext_ideal.empty(); q++)
            if (sets[s]->ext_ideal[q] == sets[s]->ext_ideal[q]) cache[key_of(s, q)] = sets[s]->ext_ideal[q];
    const std::map<int64_t, double> external = cache;
    for (int s = 0; s < 2 && sets[s]; s++) {
        const ListSetHost &d = *sets[s];
        cached[s].resize((size_t)d.Q);
        if (own) own[s].resize((size_t)d.Q);
        for (int32_t q = 0; q < d.Q; q++) {
            const int n = d.qoff[q + 1] - d.qoff[q];
            const int64_t key = key_of(s, q);
            auto it = external.find(key);
            if (it != external.end()) { cached[s][q] = it->second; if (own) own[s][q] = it->second; continue; }
            it = cache.find(key);
            if (own || it == cache.end()) {
                const double mine = ideal_dcg(d.labels.data() + d.qoff[q], n, size_of(n), disc);
                if (own) own[s][q] = mine;
                if (it == cache.end()) it = cache.emplace(key, mine).first;
            }
            cached[s][q] = it->second;
        }
    }
}

}  // namespace rl
