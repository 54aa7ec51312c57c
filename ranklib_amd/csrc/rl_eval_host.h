// rl_eval_host.h -- the host half of rl_eval_lists (rl_eval.inc): argument validation and the per-list ideal DCGs.  Plain C++ with no
// HIP in it, so a stand-alone program can include this file and call eval_prepare under a host sanitizer; nothing here touches a device.
#pragma once
#include "rl_lists_host.h"

namespace rl {

constexpr int kEvMetricLast = RL_METRIC_BEST;

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
    int rc = check_lists(who, labels, n_docs, qoff, n_lists, err);
    if (rc) return rc;
    if (scores) {
        const std::string nan = eval_check_scores(scores, qoff, n_lists);
        if (!nan.empty()) return bad(RL_ERR_INVALID, nan);
    }
    ListSetHost lists;
    lists.store(labels, n_docs, qoff, n_lists, qkey);
    if ((rc = lists.set_external(ideal_dcg, rel_doc_count, err))) return bad(rc, err);
    disc = discount_table(lists.maxq);
    ideal.assign((size_t)n_lists, std::nan(""));
    if (metric != RL_METRIC_NDCG) return RL_OK;
    ideal_cache(lists, nullptr, disc, [k](int n) { return (k > n || k <= 0) ? n : k; }, &ideal);      // one set: cached[0] alone
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
