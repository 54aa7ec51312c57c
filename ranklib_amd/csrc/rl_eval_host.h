// rl_eval_host.h -- the host half of rl_eval_lists (rl_eval.inc): argument validation and the per-list ideal DCGs.  Plain C++ with no
// HIP in it, so a stand-alone program can include this file and call eval_prepare under a host sanitizer; nothing here touches a device.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/rlhip.h"

namespace rl {

constexpr int kEvMetricLast = RL_METRIC_BEST;

inline double ev_discount(int i) { return 1.0 / (std::log((double)(i + 2)) / std::log(2.0)); }   // DCGScorer.java:26

inline double ev_ideal_dcg(const float *labels, int n, int topk, const std::vector<double> &disc)
{   // NDCGScorer.getIdealDCG (:167-174): the (int) labels best first, Java int gains
    std::vector<int> rel((size_t)n);
    for (int i = 0; i < n; i++) rel[i] = (int)labels[i];
    std::sort(rel.begin(), rel.end(), [](int a, int b) { return a > b; });
    double dcg = 0;
    for (int i = 0; i < topk; i++) dcg += (double)(int32_t)(((uint32_t)1 << (rel[i] & 31)) - 1u) * disc[i];
    return dcg;
}

// The score rule of rl_eval_lists: no NaN in any list.  Empty, or the message (without the caller's name).
inline std::string eval_check_scores(const double *scores, const int32_t *qoff, int32_t n_lists)
{
    for (int32_t q = 0; q < n_lists; q++)
        for (int32_t i = qoff[q]; i < qoff[q + 1]; i++)
            if (std::isnan(scores[i]))
                return "NaN score in list " + std::to_string(q) + " (document " + std::to_string(i - qoff[q])
                       + "): the counting rank is undefined on NaN, rank such a list on the host";
    return std::string();
}

// Everything rl_eval_lists checks and computes before it looks for a device.  Returns RL_OK or the error code with its message in err.
// On RL_OK: disc holds the discounts of positions 0 .. longest list + 1 and, for RL_METRIC_NDCG, ideal[q] is the ideal DCG list q is
// scored against: its ideal_dcg entry where that is not NaN, else the ideal of the FIRST list with its qkey (the idealGains cache of
// NDCGScorer.java:114-122: one entry per list id, whatever the later list's labels are); without qkey every list is its own key.  For
// the other metrics ideal is all NaN.
// who names the entry point in the messages.  scores == nullptr (rl_model_eval_stages: the scores do not exist yet, its kernel flags
// the NaN cells instead) skips the score rule and nothing else.
inline int eval_prepare_lists(const char *who, int32_t metric, int32_t k, double err_max, const double *scores, const float *labels,
                              int64_t n_docs, const int32_t *qoff, int32_t n_lists, const int32_t *qkey, const double *ideal_dcg,
                              const int32_t *rel_doc_count, const void *out_metric, std::vector<double> &ideal, std::vector<double> &disc,
                              std::string &err)
{
    auto bad = [&](int code, const std::string &m) { err = std::string(who) + ": " + m; return code; };
    if (!labels || !qoff || !out_metric) return bad(RL_ERR_INVALID, "null argument");
    if (metric < RL_METRIC_NDCG || metric > kEvMetricLast) return bad(RL_ERR_INVALID, "unknown metric " + std::to_string(metric));
    if (n_lists < 1 || n_docs < 1) return bad(RL_ERR_INVALID, "n_lists and n_docs must be >= 1");
    if (n_docs >= (int64_t)2147483647 - 4096) return bad(RL_ERR_UNSUPPORTED, "more than 2^31 documents per call");
    if (metric == RL_METRIC_ERR && (!(err_max > 0.0) || !std::isfinite(err_max)))
        return bad(RL_ERR_INVALID, "err_max (ERRScorer.MAX) must be positive and finite");
    if (qoff[0] != 0) return bad(RL_ERR_INVALID, "qoff must start at 0");
    for (int32_t q = 0; q < n_lists; q++) {
        if (qoff[q + 1] <= qoff[q])
            return bad(RL_ERR_INVALID, "qoff must be strictly increasing (empty ranked list " + std::to_string(q) + ")");
        if ((int64_t)qoff[q + 1] > n_docs) return bad(RL_ERR_INVALID, "qoff must end at n_docs (list " + std::to_string(q) + " runs past it)");
    }
    if ((int64_t)qoff[n_lists] != n_docs) return bad(RL_ERR_INVALID, "qoff must end at n_docs");
    for (int64_t i = 0; i < n_docs; i++) {
        if (!(labels[i] >= 0)) return bad(RL_ERR_INVALID, "Relevance label cannot be negative. System will now exit.");
        if (labels[i] >= 16777216.f) return bad(RL_ERR_UNSUPPORTED, "relevance label of 2^24 or more");
    }
    int maxq = 0;
    if (scores) {
        const std::string nan = eval_check_scores(scores, qoff, n_lists);
        if (!nan.empty()) return bad(RL_ERR_INVALID, nan);
    }
    for (int32_t q = 0; q < n_lists; q++) maxq = std::max(maxq, qoff[q + 1] - qoff[q]);
    if (rel_doc_count)
        for (int32_t q = 0; q < n_lists; q++)
            if (rel_doc_count[q] < 0) return bad(RL_ERR_INVALID, "negative relevant-document count");
    disc.resize((size_t)maxq + 2);
    for (size_t i = 0; i < disc.size(); i++) disc[i] = ev_discount((int)i);
    ideal.assign((size_t)n_lists, std::nan(""));
    if (metric != RL_METRIC_NDCG) return RL_OK;
    // as ca_prepare (rl_linear.inc): the given entries first, then the first list of a key decides
    const int64_t anon = (int64_t)1 << 40;
    std::map<int64_t, double> cache;
    for (int32_t q = 0; q < n_lists && ideal_dcg; q++)
        if (ideal_dcg[q] == ideal_dcg[q]) cache[qkey ? (int64_t)qkey[q] : anon + q] = ideal_dcg[q];
    const std::map<int64_t, double> external = cache;
    for (int32_t q = 0; q < n_lists; q++) {
        const int n = qoff[q + 1] - qoff[q];
        const int size = (k > n || k <= 0) ? n : k;
        const int64_t key = qkey ? (int64_t)qkey[q] : anon + q;
        auto pre = external.find(key);
        if (pre != external.end()) { ideal[q] = pre->second; continue; }
        auto it = cache.find(key);
        if (it == cache.end()) it = cache.emplace(key, ev_ideal_dcg(labels + qoff[q], n, size, disc)).first;
        ideal[q] = it->second;
    }
    return RL_OK;
}

inline int eval_prepare(int32_t metric, int32_t k, double err_max, const double *scores, const float *labels, int64_t n_docs,
                        const int32_t *qoff, int32_t n_lists, const int32_t *qkey, const double *ideal_dcg, const int32_t *rel_doc_count,
                        const double *out_metric, std::vector<double> &ideal, std::vector<double> &disc, std::string &err)
{
    if (!scores) { err = "rl_eval_lists: null argument"; return RL_ERR_INVALID; }
    return eval_prepare_lists("rl_eval_lists", metric, k, err_max, scores, labels, n_docs, qoff, n_lists, qkey, ideal_dcg, rel_doc_count,
                              out_metric, ideal, disc, err);
}

}  // namespace rl
