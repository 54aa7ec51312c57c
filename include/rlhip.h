/*
 * rlhip.h -- C ABI of librlhip.so: an MI355X (gfx950) native LambdaMART trainer that is a
 * drop-in for the training / scoring path behind RankLib's `-ranker 6`.
 *
 * This is the drop-in boundary.  Everything a JNI shim, the ctypes host
 * mirror (ranklib_amd/) or a native CLI needs goes through these entry points: plain
 * pointers and sizes, no C++/torch types, int status codes, no exceptions across the ABI.
 * INTEGRATION.md shows the JNI binding and the Java host class a RankLib maintainer would add.
 *
 * Reference interfaces replaced (paths relative to
 * /root/reference/src/main/java/ciir/umass/edu/):
 *
 *   rl_create / rl_set_*        <- RankerFactory.createRanker + Ranker ctor/setters
 *                                  learning/RankerFactory.java:60-70, learning/Ranker.java:52-74,
 *                                  static parameters learning/tree/LambdaMART.java:37-42
 *   rl_init                     <- LambdaMART.init()            learning/tree/LambdaMART.java:68-166
 *   rl_boost_round(s)           <- one iteration of learn()     learning/tree/LambdaMART.java:180-251
 *   rl_finish                   <- tail of learn()              learning/tree/LambdaMART.java:253-265
 *   rl_get_tree / rl_num_trees  <- getEnsemble()                learning/tree/LambdaMART.java:327-329,
 *                                  Ensemble/RegressionTree/Split learning/tree/Ensemble.java:72-100
 *   rl_predict                  <- LambdaMART.eval -> Ensemble.eval  learning/tree/LambdaMART.java:275-277,
 *                                  learning/tree/Ensemble.java:110-116, learning/tree/Split.java:115-125
 *   rl_model_to_text/from_text  <- model() / loadFromString()   learning/tree/LambdaMART.java:290-310,
 *                                  learning/tree/Ensemble.java:45-70,119-130, learning/tree/Split.java:132-155
 *
 * Error convention: the reference throws unchecked RankLibError (utilities/RankLibError.java:25-42).
 * Here every call returns RL_OK (0) or a negative code and leaves a message retrievable with
 * rl_last_error() (thread-local); a JNI shim rethrows it as RankLibError.create(msg).
 *
 * Threading: like the reference (single caller, global statics) a handle must be used by one
 * thread at a time; distinct handles are independent.
 *
 * Ownership: the caller owns every buffer it passes; rl_set_* copy to HBM and never retain the
 * pointers.  Output buffers are caller-allocated.
 */
#ifndef RLHIP_H
#define RLHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLHIP_ABI_VERSION 5

enum {
    RL_OK = 0,
    RL_ERR_INVALID = -1,     /* bad argument / bad input data (e.g. negative label: learning/DataPoint.java:70-73) */
    RL_ERR_HIP = -2,         /* HIP runtime or kernel failure, message holds file:line */
    RL_ERR_STATE = -3,       /* call out of order (e.g. rl_boost_round before rl_init) */
    RL_ERR_UNSUPPORTED = -4, /* valid for RankLib but not built yet (documented in DESIGN.md) */
    RL_ERR_NO_DEVICE = -5,   /* no gfx950 device visible: there is NO CPU fallback */
    RL_ERR_COMM = -6,        /* RCCL failure */
    RL_ERR_NO_BEST = -7      /* rl_ln_learn / rl_rn_learn with a validation set: no epoch scored above 0.0, no model was saved (the Java throws) */
};

/* train / validation metric (-metric2t): metric/{NDCG,DCG,AP,ERR}Scorer.java, and RL_METRIC_P / RL_METRIC_RR (metric/PrecisionScorer.java,
 * metric/ReciprocalRankScorer.java; declared further down, with k >= 1).  RL_METRIC_BEST is not built for training (RL_ERR_UNSUPPORTED);
 * the host side can still report it on ranked lists. */
enum { RL_METRIC_NDCG = 0, RL_METRIC_DCG = 1, RL_METRIC_MAP = 2, RL_METRIC_ERR = 3 };
/* ranker: the indices of eval/Evaluator.java:69-73 */
enum { RL_RANKER_MART = 0, RL_RANKER_LAMBDAMART = 6 };

enum {                                  /* rl_params.flags */
    RL_FLAG_FAST_LEAF = 1,              /* opt-in, off by default: the two sums behind every leaf output are a fixed f64 reduction -- tiles of 256 samples in
                                           ascending sample order, each folded in halves (a[i] += a[i + s], s = 128 .. 1), the tile results folded the same way until
                                           one value is left, then rounded to float -- instead of the Java's float running sums (learning/tree/
                                           LambdaMART.java:401-408), which stay the default and bit-exact.  Deterministic and independent of any launch shape; two
                                           launches instead of about ten a round.  Leaf values differ from the reference's in their last bits (measured: DESIGN.md
                                           14), so later rounds may grow other trees; the per-round metric stays the exact float chain.  One GPU
                                           only: rl_dist_init* is RL_ERR_UNSUPPORTED (an f64 sum over ranks is not rank-count-invariant).  Not with
                                           RL_FLAG_JAVA_ORDER (the strict mode is a parity instrument) nor RL_FLAG_SERIAL_CHAIN: RL_ERR_INVALID at rl_create.
                                           Independent of RL_FLAG_FIRST_TIE; the two together are the speed-first setting. */
    RL_FLAG_TIMING = 2,                 /* record HIP events around the root histogram and the lambda kernels (rl_get_timing) */
    RL_FLAG_TIMING_NODES = 8,           /* ... and around every growth step's node-histogram launch (30 event pairs per round) */
    RL_FLAG_SERIAL_CHAIN = 4,           /* evaluate the float running sums with the literal serial kernel instead of
                                           the exact parallel scheme (same results; for cross-checks) */
    RL_FLAG_FIRST_TIE = 32,             /* exact ties between split candidates keep the first one in scan order instead of being re-decided in the Java's
                                           summation order (the lazy tie-break, HISTORY.md 4.13: default, also for sharded runs; never with feature sampling).
                                           Faster where nodes are tiny or columns sparse; the trees differ from the reference's only in the stored threshold
                                           inside an empty-bin plateau / in which of two equivalent features is named. */
    RL_FLAG_JAVA_ORDER = 16             /* strict mode: split gains and node deviances come from the f64 histogram RankLib itself
                                           would hold -- every (feature, bin) sum accumulated sequentially in ascending sample
                                           order (FeatureHistogram.java:126-146,166-195), sequential prefix, right sibling =
                                           parent - left on the cumulative arrays (:222-234), sumResponse / sqSumResponse as
                                           :133-137,182-186,202-203 -- so the arg-max of :236-264,302-309 lands on the candidate
                                           the Java picks even where exact arithmetic ties.  Same trees, several
                                           times slower (the sums are serial chains); one GPU only. */
};

typedef struct rl_trainer rl_trainer;   /* opaque */
typedef struct rl_model rl_model;       /* opaque: a loaded ensemble for scoring only */

typedef struct {
    int32_t n_trees;            /* LambdaMART.nTrees            default 1000 */
    int32_t n_leaves;           /* LambdaMART.nTreeLeaves       default 10   */
    int32_t n_threshold;        /* LambdaMART.nThreshold        default 256 (-1: every distinct value; any size: tables beyond 4095 entries run as
                                   several histogram features, rl_hist_features) */
    int32_t min_leaf_support;   /* LambdaMART.minLeafSupport    default 1    */
    int32_t early_stop_rounds;  /* LambdaMART.nRoundToStopEarly default 100  */
    float   learning_rate;      /* LambdaMART.learningRate      default 0.1F (a Java float) */
    int32_t metric;             /* RL_METRIC_*: NDCG, DCG, MAP, ERR, P, RR (RL_METRIC_BEST: RL_ERR_UNSUPPORTED) */
    int32_t metric_k;           /* the scorer's k: default 10 for NDCG / DCG / ERR / P (metric/DCGScorer.java:21,
                                   metric/ERRScorer.java:28, metric/PrecisionScorer.java:22), 0 for MAP (metric/APScorer.java:37-39);
                                   P and RR need k >= 1 (RR's own default k = 0 scores 0 everywhere) */
    int32_t device;             /* HIP device ordinal */
    int32_t flags;              /* RL_FLAG_* */
    int32_t ranker;             /* RL_RANKER_LAMBDAMART (default) or RL_RANKER_MART (learning/tree/MART.java:47-65) */
    float   feature_sampling_rate;  /* FeatureHistogram.samplingRate (learning/tree/FeatureHistogram.java:34,272-287), set by
                                   RFRanker.init (learning/tree/RFRanker.java:68): < 1 = every split attempt looks at
                                   (int)(rate * n_features) features drawn without replacement.  Default 1 (0 is read as 1). */
    uint64_t seed;              /* The Java draws from an unseeded java.util.Random.  Here the draw of a node is a pure function of
                                   (seed, index of the tree in this trainer, path of the node from the root): the features sorted by
                                   a 64-bit hash key, the first (int)(rate * F) in key order (the first drawn wins a tie, as the
                                   Java's scan order does).  oracle/rl_oracle.h ro_feature_order() is the same function. */
} rl_params;

/* One regression tree: nodes in pre-order (root 0, left subtree first) == Split.leaves() order
 * (learning/tree/Split.java:100-113).  Arrays are caller-allocated with `cap` entries
 * (2*n_leaves-1 always suffices). */
typedef struct {
    int32_t  n_nodes;     /* out */
    int32_t  cap;         /* in  */
    int32_t *feature;     /* feature ID as written to the model file; -1 = leaf   (Split.featureID) */
    float   *threshold;   /* Split.threshold: go left iff value <= threshold      (Split.java:118)  */
    int32_t *left;        /* child node index, -1 for leaves */
    int32_t *right;
    float   *output;      /* leaf output (Split.avgLabel set by updateTreeOutput), 0 for internal nodes */
    double  *deviance;    /* optional (may be NULL): Split.deviance */
    int32_t *count;       /* optional (may be NULL): training samples that reached the node */
} rl_tree;

/* ---- library ----------------------------------------------------------------------------- */
int         rl_abi_version(void);
const char *rl_last_error(void);
int         rl_device_count(int32_t *n);
void        rl_params_default(rl_params *p);              /* the defaults of LambdaMART.java:37-42 */

/* ERRScorer.MAX (metric/ERRScorer.java:25), the divisor of ERR's relevance grades R = (2^label - 1) / MAX; `-gmax g` sets it to 2^g
 * (eval/Evaluator.java:241-242).  A process-wide static in the reference, and here: trainers created afterwards use it.  Default 16. */
int  rl_set_err_max(double max_gain);

/* ---- trainer ----------------------------------------------------------------------------- */
int  rl_create(const rl_params *p, rl_trainer **out);
void rl_destroy(rl_trainer *t);

/* Training set.  X is row-major [n_docs][n_features], already resolved through
 * DataPoint.getFeatureValue(feature_ids[f]) (missing / NaN -> 0: learning/DenseDataPoint.java:21-32); a NaN left in X is RL_ERR_INVALID at
 * rl_init, +-Infinity is a value like any other (binned as learning/tree/LambdaMART.java:108-149 and FeatureHistogram.java:88-107 bin it).
 * qoff[n_queries+1]: docs of query q are qoff[q]..qoff[q+1]-1 (file order, learning/RankList.java).
 * feature_ids[n_features]: the IDs written into the model (Ranker.features); NULL => 1..n_features.
 * qkey[n_queries]: optional; equal keys == equal qid strings (idealGains cache quirk,
 * metric/NDCGScorer.java:114-122,134-143); NULL => all distinct. */
int rl_set_train(rl_trainer *t, const float *X, int64_t n_docs, int32_t n_features, const float *labels,
                 const int32_t *qoff, int32_t n_queries, const int32_t *feature_ids, const int32_t *qkey);
/* Ranker.setValidationSet (learning/Ranker.java:68-70); same layout, same feature columns. */
int rl_set_validation(rl_trainer *t, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff,
                      int32_t n_queries, const int32_t *qkey);

/* Chunked upload for callers that cannot hold the whole row matrix in one buffer (a Java direct ByteBuffer ends at 2 GiB; MSLR-WEB30K's
 * 3.77 M x 136 floats are 2.05 GB): pass X = NULL to rl_set_train / rl_set_validation (labels, qoff, ids as usual), then deliver the rows
 * in consecutive blocks, first_doc ascending from 0, before rl_init.  X: row-major [n_docs][n_features] of that block. */
int rl_set_rows(rl_trainer *t, int32_t validation, int64_t first_doc, int64_t n_docs, const float *X);

/* -qrel <file> (eval/Evaluator.java:243-244, :580-591): external relevance judgments, resolved per ranked list by the caller.
 *   ideal_dcg[Q]      NDCG: the entry NDCGScorer.loadExternalRelevanceJudgment (metric/NDCGScorer.java:50-96) put into idealGains for the
 *                     list's qid -- it is in the cache before any list is scored, so the list never computes its own; NaN = the qid is not
 *                     in the file.  NULL = no external ideal gains.
 *   rel_doc_count[Q]  MAP: relDocCount of the list's qid (metric/APScorer.java:45-66), 0 when the qid is not in the file (the Java then scores
 *                     the list 0 and returns all-zero swap changes, :86-94, :124-143).  NULL = every list counts its own relevant documents.
 * After rl_set_train / rl_set_validation of that data set, before rl_init.  Sharded runs: every rank passes the entries of ITS lists. */
int rl_set_external_judgments(rl_trainer *t, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count);

int rl_init(rl_trainer *t);

/* One boosting round, synchronous.  out may be NULL.  *stop is set to 1 when the early-stop test
 * (learning/tree/LambdaMART.java:248) fires after this round.  train_metric / valid_metric are the
 * float-accumulated per-round values of :216 / :237 (valid_metric untouched without validation data). */
int rl_boost_round(rl_trainer *t, rl_tree *out, float *train_metric, float *valid_metric, int32_t *stop);

/* Resume: the T0 trees of a saved model -- `text` is what rl_model_to_text wrote, one <ensemble> -- become rounds 0 .. T0 - 1 of
 * this trainer, replayed on its own data instead of grown.  After rl_init, before the first round and before rl_finish (else RL_ERR_STATE).
 * Afterwards the trainer stands where the trainer that grew those trees stood after round T0, bit for bit: RL_ARR_SCORE / RL_ARR_VALID_SCORE
 * are the f64 chains  s += (double)learning_rate * (double)output  over the T0 trees in order, the training lists are ranked by them,
 * rl_get_round_metrics(r < T0) are the float means of the scores after tree r, rl_best_validation is rebuilt by rl_boost_round's strict >
 * over those rounds, and *stop (may be NULL) is the early-stop test of LambdaMART.java:248 at round T0 - 1.  Adoption itself never stops;
 * rl_boost_round goes on with round T0 (n_trees stays the TOTAL number of trees; T0 == n_trees leaves rl_finish only).  The adopted trees'
 * `count` is -1 and `deviance` NaN in rl_get_tree: diagnostics the text does not hold.
 * scratch_bytes bounds the per-tree stage scores the replay keeps at a time (8 bytes per document of both data sets and tree; 0 = 256 MiB;
 * at least one tree); it cannot change a bit of the result.
 * RL_ERR_INVALID, the message naming the cause: null text, text the parser refuses, more than one <ensemble>, no trees, more trees than
 * n_trees, a tree with more nodes than rl_tree_capacity, a split on a feature id that is not among the trainer's feature_ids, a tree
 * weight whose bits differ from learning_rate (per-tree weights are not built), scratch_bytes < 0.  A sharded trainer: RL_ERR_UNSUPPORTED. */
int rl_adopt_model_text(rl_trainer *t, const char *text, int64_t scratch_bytes, int32_t *stop);

/* Refit: the T0 trees of a saved model keep their structure -- features, thresholds, children -- and get new leaf values from this
 * trainer's data.  `text` and the moment of the call are rl_adopt_model_text's: after rl_init, before the first round.  For r = 0 .. T0 - 1 in order:
 *   1. lambda and w of the current modelScores, exactly as round r of training computes them (MART: label - score); the trainer's metric and
 *      flags apply as in a normal round.
 *   2. every training document is walked down tree r on its RAW ROW, value <= threshold goes left (Split.java:115-125); the model's thresholds
 *      need not be bin boundaries of this data.
 *   3. the leaves are taken in left-first DFS order (Split.leaves), the documents of a leaf in ASCENDING DOCUMENT INDEX, the order
 *      Split.getSamples() has after stable partitions of 0 .. N-1.
 *   4. the new value of a leaf: LambdaMART the two float running sums of LambdaMART.java:401-413, 0 when s2 == 0; MART s1 / count
 *      (MART.java:54-65); evaluated by the leaf evaluator the flags select (default chains, RL_FLAG_SERIAL_CHAIN, RL_FLAG_FAST_LEAF).
 *   5. a leaf no document reaches keeps its old output.
 *   6. decay == 0: the stored output is the new value, no arithmetic (bit equal whatever the old output was); else it is
 *      (float)((double)decay * (double)old + (1.0 - (double)decay) * (double)new).
 *   7. the tree with its new outputs replaces tree r; modelScores[k] += (double)learning_rate * (double)output; the round's ranking and float-mean
 *      metric, and for a validation set the score update, ranking and metric, as behind a trained round.
 * Afterwards the trainer stands at round T0 as after rl_adopt_model_text: rl_get_round_metrics(r < T0) hold the refit rounds' values,
 * rl_best_validation is rebuilt by the strict >, *stop (may be NULL) is the test of LambdaMART.java:248 at round T0 - 1, rl_boost_round goes on
 * with round T0 on this data, rl_finish and rl_model_to_text work.  rl_get_tree reports the documents that reached each node as `count`;
 * `deviance` stays NaN.  Refitting a model on the data and parameters it was trained with, decay 0, gives the model back bit for bit.
 * RL_ERR_INVALID: what rl_adopt_model_text refuses, a decay that is NaN, negative or >= 1, a tree with more leaves than the leaf machinery
 * takes (n_leaves of the trainer, at most 512; the message states the number).  A sharded trainer: RL_ERR_UNSUPPORTED. */
int rl_refit_model_text(rl_trainer *t, const char *text, float decay, int32_t *stop);

/* out[3]: launches of the routing kernel of rl_refit_model_text that staged the rows in LDS, launches that read them from global memory (more
 * than 640 features, or RLHIP_REFIT_DIRECT), leaves that kept their old output because no document reached them. */
int rl_debug_refit_stats(const rl_trainer *t, int64_t *out);

/* Enqueue n rounds without any host synchronisation (no validation set allowed: early stopping needs
 * the host).  rl_sync waits for them; trees and per-round metrics are then available through
 * rl_get_tree / rl_get_round_metrics. */
int rl_boost_rounds_async(rl_trainer *t, int32_t n);
int rl_sync(rl_trainer *t);

/* End of learn(): rollback to the best validation model, final scorer.score(rank(samples)) with
 * Ensemble.eval's float accumulation.  valid_score may be NULL. */
int rl_finish(rl_trainer *t, double *train_score, double *valid_score);

int rl_num_trees(const rl_trainer *t, int32_t *n);
/* Nodes the largest possible tree of this trainer has = the `cap` of an rl_tree that always suffices, known after rl_init: 2 * n_leaves - 1, at
 * least 3 (the root is split unconditionally, RegressionTree.java:62-67); with -leaf -1 (n_leaves == -1) 2 * floor(N / min_leaf_support) - 1. */
int rl_tree_capacity(const rl_trainer *t, int32_t *cap);
int rl_get_tree(const rl_trainer *t, int32_t i, rl_tree *out);
int rl_get_round_metrics(const rl_trainer *t, int32_t round, float *train_metric, float *valid_metric);
int rl_best_validation(const rl_trainer *t, int32_t *best_round, double *best_score);

/* Ensemble.eval over rows (float accumulation in tree order).  X row-major [n][n_features] with the
 * trainer's feature columns. */
int rl_predict(rl_trainer *t, const float *X, int64_t n_docs, float *out);

/* ---- model text (RankLib's <ensemble> format) -------------------------------------------- */
/* Writes LambdaMART.model() into buf (NUL-terminated).  Returns RL_OK and *needed = bytes required
 * incl. NUL; if cap < *needed nothing is written. */
int  rl_model_to_text(const rl_trainer *t, char *buf, int64_t cap, int64_t *needed);
/* Text that Ensemble's constructor would refuse is RL_ERR_INVALID ("Error in Emsemble(xmlRepresentation): ..."), and so is a split whose
 * feature id is below -1 or does not fit an int: Integer.parseInt refuses the second, and the first indexes before the row when the
 * Java scores.  A feature id of -1 is a leaf (Split.eval, Split.java:116). */
int  rl_model_from_text(const char *text, int32_t device, rl_model **out);
void rl_model_destroy(rl_model *m);
int  rl_model_num_trees(const rl_model *m, int32_t *n);
/* Features used by the model: Ensemble.getFeatures (learning/tree/Ensemble.java:132-134). */
int  rl_model_features(const rl_model *m, int32_t *ids, int32_t cap, int32_t *n);
/* X row-major [n][row_stride]; feature ID f is read from column f (column 0 unused, like DataPoint.fVals);
 * IDs >= row_stride read as 0 (the -missingZero behaviour). */
int  rl_model_predict(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, float *out);
/* The same on buffers that already live in the model's device memory (rows and scores are DEVICE pointers); the work is
 * enqueued on `stream` (a hipStream_t, NULL = the default stream) and NOT synchronised.  This is the call a serving
 * loop uses: Ensemble.eval for a batch of rows without the PCIe round trip (eval/Evaluator.java:1076-1094 does the
 * same per DataPoint on the CPU). */
int  rl_model_predict_device(rl_model *m, const float *dX, int64_t n_docs, int32_t row_stride, float *dOut, void *stream);
/* which kernel the last rl_model_predict / rl_model_predict_device of a handle took (rl_model_debug_path) */
enum { RL_MODEL_PATH_NONE = 0, RL_MODEL_PATH_TILED = 1, RL_MODEL_PATH_GENERIC = 2 };
/* debug: RL_MODEL_PATH_* of the last predict call (Split.eval :115-125 and Ensemble.eval :110-116 are the same arithmetic in both kernels) */
int  rl_model_debug_path(const rl_model *m, int32_t *path);

/* ---- LETOR text (host only) ---------------------------------------------------
 * `label qid:ID fid:val ... # description` lines as learning/DataPoint.java:58-110 and features/FeatureManager.java:199-235 read
 * them: lines are trimmed, empty ones and '#' comments skipped, the description is the text from '#', the qid / the values are
 * the text after the LAST ':' of their token, values are Float.parseFloat (strtof: correctly rounded).  Every line that is not
 * plain `number qid:token (digits:number)*` -- or that the reference rejects (negative label, feature id <= 0) -- is only
 * FLAGGED (`slow`): the caller parses, or rejects, those lines itself, in file order.  `text` must outlive the handle. */
typedef struct rl_letor rl_letor;
int  rl_letor_parse(const char *text, int64_t len, rl_letor **out);
int  rl_letor_info(const rl_letor *l, int64_t *n_docs, int32_t *max_fid, int64_t *n_slow);
/* per data line (any pointer may be NULL): label, largest feature id, qid / description / whole trimmed line as (offset, length)
 * into `text`, and the slow flag */
int  rl_letor_arrays(const rl_letor *l, float *labels, int32_t *last_fid, int64_t *qid_off, int32_t *qid_len, int64_t *desc_off,
                     int32_t *desc_len, int64_t *line_off, int32_t *line_len, uint8_t *slow);
/* dense rows: X[i * row_stride + fid] = value, NaN where the line does not name the feature (DenseDataPoint's UNKNOWN);
 * row_stride >= max_fid + 1; rows of flagged lines are all NaN */
int  rl_letor_rows(const rl_letor *l, float *X, int64_t row_stride);
void rl_letor_destroy(rl_letor *l);
/* The way back (host only): DataPoint.toString (learning/DataPoint.java:188-199) of n_docs rows plus '\n' each, what
 * FeatureManager.save writes (features/FeatureManager.java:455-476):
 *   (int) label, " qid:" id " ", then for f = 1 .. row_len[i] - 1 every cell X[i * row_stride + f] that is not NaN as
 *   f ":" Float.toString(cell), followed by a space unless f == row_len[i] - 1, then " " description.
 * row_len[i] is the length of the row's fVals (column 0 unused), 0 <= row_len[i] <= row_stride; the qid and the description of row i
 * are (offset, length) into `strings` (strings_len bytes).  Returns RL_OK and *needed = bytes of text (no NUL is written); if
 * cap < *needed nothing is written.  Lines are formatted on at most 16 host threads. */
int  rl_letor_format(const float *X, int64_t n_docs, int64_t row_stride, const int32_t *row_len, const float *labels, const char *strings,
                     int64_t strings_len, const int64_t *qid_off, const int32_t *qid_len, const int64_t *desc_off, const int32_t *desc_len,
                     char *buf, int64_t cap, int64_t *needed);

/* ---- multi-GPU (one process per GPU; queries sharded across ranks) ---------- */
#define RL_UNIQUE_ID_BYTES 128
int rl_dist_unique_id(void *id_out /* RL_UNIQUE_ID_BYTES */);       /* call on rank 0, broadcast out of band */
/* Must be called before rl_init.  Each rank passes ITS shard of the queries to rl_set_train (and, if there is a validation set, its
 * shard of the validation queries to rl_set_validation: every rank or none); the per-split histograms (and the few per-round scalars)
 * are summed across ranks with RCCL, per-query metric values are gathered in rank order. */
int rl_dist_init(rl_trainer *t, const void *id, int32_t rank, int32_t n_ranks);

/* Exchange volume of this rank since rl_dist_init: out[0..7] = all-reduce calls, all-reduce payload bytes, all-gather calls, all-gather
 * bytes received, all-to-all calls, all-to-all bytes received from OTHER ranks -- the per-round pattern -- and, counted apart, the calls and
 * bytes received of the lazy tie-break's exchanges (zeros for an unsharded trainer).  bench.py prints the per-round figures for N > 1. */
int rl_dist_stats(const rl_trainer *t, int64_t *out);

/* The same sharded training over a caller-supplied transport instead of RCCL (gloo, MPI, shared memory ...):
 * the library stages each exchange through host memory and calls back.  Slower (a host synchronisation per
 * exchange); used by the tests to run several ranks on ONE GPU and prove k shards == 1 shard bit for bit.
 * dtype: RL_DT_*, op: RL_OP_*; all-reduce is in place on `host_buf`; all-gather writes n_ranks*bytes to `out`.
 * Callbacks return 0 on success. */
enum { RL_DT_I64 = 0, RL_DT_U64 = 1, RL_DT_I32 = 2, RL_DT_U32 = 3, RL_DT_F64 = 4 };
enum { RL_OP_SUM = 0, RL_OP_MAX = 1, RL_OP_MIN = 2 };
typedef int (*rl_host_allreduce_fn)(void *user, void *host_buf, int64_t count, int32_t dtype, int32_t op);
typedef int (*rl_host_allgather_fn)(void *user, const void *in, void *out, int64_t bytes_per_rank);
/* variable all-to-all in BYTES: rank p receives send[sdispl[p] .. +scount[p]) of this rank; what rank p sends to this rank lands at
 * recv[rdispl[p] .. +rcount[p]) (p == own rank included: a plain copy).  All four arrays have n_ranks entries. */
typedef int (*rl_host_alltoallv_fn)(void *user, const void *send, const int64_t *scount, const int64_t *sdispl, void *recv,
                                    const int64_t *rcount, const int64_t *rdispl);
/* alltoallv may be NULL: the leaf exchange is then emulated with all-gathers of whole send buffers (correct, R times the bytes). */
int rl_dist_init_callback(rl_trainer *t, int32_t rank, int32_t n_ranks, rl_host_allreduce_fn allreduce,
                          rl_host_allgather_fn allgather, rl_host_alltoallv_fn alltoallv, void *user);

/* ---- introspection for parity tests and the roofline report ------------------------------- */
enum {
    RL_ARR_LAMBDA = 1,       /* double[n_docs]  pseudoResponses of the last round */
    RL_ARR_WEIGHT = 2,       /* double[n_docs] */
    RL_ARR_SCORE = 3,        /* double[n_docs]  modelScores */
    RL_ARR_VALID_SCORE = 4,  /* double[n_valid_docs] */
    RL_ARR_NBINS = 5,        /* int32[n_features]           thresholds[f].length */
    RL_ARR_THRESHOLDS = 6,   /* float[n_features*stride]    rows padded to `stride` = max nbins */
    RL_ARR_BINS = 7,         /* uint16[n_features*n_docs]   sampleToThresholdMap, feature-major */
    RL_ARR_ROOT_COUNT = 8,   /* int32[n_features*stride]    cumulative root counts */
    RL_ARR_ROOT_SUM = 9,     /* double[n_features*stride]   cumulative root sums of the last round */
    RL_ARR_QUANT = 10,       /* int64[n_docs]               fixed-point lambdas of the last round */
    RL_ARR_ROOT_SUM_FIXED = 11, /* int64[2*n_features*stride] (hi,lo) 128-bit cumulative fixed-point sums */
    RL_ARR_NDCG_PER_QUERY = 12, /* double[n_queries] of the last round */
    RL_ARR_CHAIN_STATS = 13,    /* int32[6]: leaf float chains {evaluated, candidate-window misses repaired, finished
                                   by the serial kernel}; the same three for the per-round metric chain */
    RL_ARR_CHAIN_MISS = 14,     /* int32[2*(2*n_leaves)]: per (value array, leaf slot) window misses of the last round */
    RL_ARR_GROW_STATS = 15,     /* int32[4] cumulative: growth steps run, nodes prepared (partition + child histograms),
                                   splits committed to trees, trees grown -- speculative best-first growth */
    RL_ARR_ROOT_SUM_JAVA = 17,  /* double[n_features*stride]   with RL_FLAG_JAVA_ORDER: cumulative root sums of the last round in the
                                   Java's own accumulation order (== FeatureHistogram.sum of the root, bit for bit) */
    RL_ARR_GROW_DOCS = 18,      /* int64[4] cumulative documents: accumulated into child histograms (the smaller child of every prepared
                                   node), partitioned, left children of committed splits (= what the Java accumulates: the rho of
                                   SURVEY.md 8d times N), committed split nodes (nu times N) */
    RL_ARR_SPARSE_INFO = 19,    /* int64[8]: 16-feature groups whose root histogram comes from sparse-column entry lists (rl_csc.inc), entries,
                                   groups read as dense rows, live columns in the sparse groups; groups whose child passes read compact rows (0 = off),
                                   their entries (cells outside the mode bins), rows with more than eight entries (dense fallback), row stride */
    RL_ARR_TIE_STATS = 21,      /* int64[10] cumulative, the lazy Java-order tie-break (HISTORY.md 4.13): resolutions run by the host (stalled trees + batches), nodes
                                   whose tied best split was re-decided in the Java's summation order, nodes and documents of the derivation chains that were summed,
                                   host microseconds spent resolving, chain segments evaluated speculatively, candidate-window misses, segments run serially,
                                   [8] of the resolutions the batches at the end of a tree (deferred ties), [9] trees grown a second time (a deferred tie over
                                   several features did not cut the node one way) */
    RL_ARR_STEP_LOG = 20,       /* int32[8 + 8 * 8192], only with RLHIP_STEPLOG=1 in the environment of rl_init (else zeros): [0] = entries written; entry e at
                                   8 + 8 e: {tree, 0, growth step, slot, documents of the split node, documents of the accumulated child, tie flag, slots of the
                                   step} or {tree, 1, tie kind (1 = thresholds of one feature, 2 = several features), right child?, documents, largest node of
                                   the Java-order derivation chain, nodes in the chain, documents in the chain} for a committed split whose best candidate was tied */
    RL_ARR_PHASE_CLOCKS = 16,   /* int64[64][32] device wall-clock stamps (10 ns) inside the last 64 growth steps; all zero unless the
                                   library was built with -DRL_PHASE_CLOCKS (tools/phase_clocks.py) */
    RL_ARR_BLOCK_TRACE = 22,    /* int64[64][3][2048][8] entry / phase / exit stamps (10 ns; [0] entry, [7] exit) of every working block of the partition / child-histogram /
                                   finish kernels in the growth steps of the tree named by RLHIP_TRACE_TREE (-DRL_PHASE_CLOCKS builds,
                                   tools/step_trace.py); RL_ERR_STATE when no trace was requested */
    RL_ARR_PIECE_STATS = 24,    /* int64[2] cumulative, sharded runs with distributed float chains (rl_dist.inc): rounds of the repair loop, pieces re-evaluated from an
                                   exact start state after a detected window miss */
    RL_ARR_BUBBLES = 23,        /* int64[4] cumulative device wall-clock time (10 ns units) the main stream idled behind host decisions: [0] from the bookkeeping that ended a
                                   tree to the leaf table's first instruction, [1] trees, [2] from a leaf chain's last stitch to the leaf outputs, [3] rounds (round 6) */
    RL_ARR_LAUNCH_ARMS = 25     /* int64[RL_ARM_COUNT_], read-only: which kernel variant the host launched, counted on the host (one increment per launch, cumulative
                                   since rl_create), and the layout settings in force.  Indexed by the RL_ARM_* values below */
};
/* RL_ARR_LAUNCH_ARMS.  The histogram kernel's arms are counted apart for the root pass (RL_ARM_HIST_ROOT + arm) and the child passes (RL_ARM_HIST_CHILD + arm):
 * an arm names the k_hist instantiation launch_hist chose (rl_launch.inc), in the order it looks for one. */
enum {
    RL_HARM_COMPACT = 0,        /* child passes from compact rows (sparse data, RLHIP_CROWS) */
    RL_HARM_SUB8 = 1,           /* child passes, 8 features and 256 threads a block (RLHIP_SUB_CHILD=8) */
    RL_HARM_SUB4 = 2,           /* child passes, 4 features and 256 threads a block (RLHIP_SUB_CHILD=4) */
    RL_HARM_NT1024 = 3,         /* child passes, 1024 threads a block (RLHIP_HIST_NT >= 1024) */
    RL_HARM_NT512 = 4,          /* child passes, 512 threads a block (RLHIP_HIST_NT in 257 .. 1023) */
    RL_HARM_FQ_PACKED = 5,      /* root pass that quantises the lambdas itself, packed rows (the default root pass) */
    RL_HARM_FQ_ROWS16 = 6,      /* root pass that quantises the lambdas itself, 16-bit rows (RLHIP_P8=0) */
    RL_HARM_PACKED_RUNS = 7,    /* packed rows, columns that come in runs folded by quads */
    RL_HARM_PACKED = 8,         /* packed rows (root: RLHIP_FUSED_QUANT=0; children: RLHIP_P8=2) */
    RL_HARM_ROWS16_RUNS = 9,    /* 16-bit rows, columns that come in runs folded by quads */
    RL_HARM_ROWS16 = 10,        /* 16-bit rows (the default child pass) */
    RL_HARM_STRIDE = 11,        /* LDS row stride known at run time only: more than 264 bins a feature, or fewer than 16 features a block */
    RL_HARM_COUNT_ = 12,
    RL_ARM_HIST_ROOT = 0, RL_ARM_HIST_CHILD = 12,      /* + RL_HARM_* */
    /* launch_rank (training and validation lists alike) */
    RL_ARM_RANK_TINY = 24, RL_ARM_RANK_MIXED = 25, RL_ARM_RANK_WAVE_LONG = 26, RL_ARM_RANK_WAVE_SHORT = 27, RL_ARM_RANK_BLOCK = 28, RL_ARM_RANK_HUGE = 29,
    /* the lambda kernels of a round (enqueue_lambdas) */
    RL_ARM_LAM_MART = 30,       /* k_mart_residual */
    RL_ARM_LAM_TINY = 31,       /* k_lambda_tiny */
    RL_ARM_LAM_FUSED = 32,      /* k_lambda_fused<., 0>: NDCG / DCG, column by row */
    RL_ARM_LAM_COMPACT = 33,    /* k_lambda_fused<., 0, true>: NDCG / DCG from the lists of active pairs (RLHIP_LAMBDA_COMPACT) */
    RL_ARM_LAM_ERR = 34,        /* k_lambda_fused<., 1> */
    RL_ARM_LAM_MAP = 35,        /* k_lambda_fused<., 2>  (k_lambda_fused<., 3> and <., 4>, P and RR, have no arm: the table is full; their launches
                                   are counted by stream only, RL_ARM_LAM_ON_SIDE / RL_ARM_LAM_ON_MAIN) */
    RL_ARM_LAM_UNFUSED = 36,    /* k_pair_terms + k_lambda_acc (counted once a round) */
    RL_ARM_LAM_ON_SIDE = 37,    /* of the fused launches, those enqueued on a side stream (RLHIP_LAMBDA_SIDE) */
    RL_ARM_LAM_ON_MAIN = 38,    /* ... and on the main stream (k_lambda_tiny included) */
    RL_ARM_QUANTIZE = 39,       /* k_quantize launches: rounds whose root pass did not quantise the lambdas itself */
    RL_ARM_XPLAN_HOST = 40,     /* sharded, leaf-owner exchange: plans made on the host (RLHIP_DIST_HOST_PLAN) */
    RL_ARM_XPLAN_DEVICE = 41,   /* ... and on the device (k_plan_exchange) */
    RL_ARM_STEPS_ENQUEUED = 42, /* growth steps the host enqueued (empty ones behind a finished tree included) */
    /* growth steps the host keeps in flight beyond the progress word: one GPU (RLHIP_STEP_AHEAD), sharded (RLHIP_DIST_STEP_AHEAD); settings, not counters */
    RL_ARM_SET_STEP_AHEAD = 43, RL_ARM_SET_DIST_AHEAD = 44,
    /* the last child-pass launch: grid columns, grid rows, dynamic LDS bytes */
    RL_ARM_CHILD_GRID_X = 45, RL_ARM_CHILD_GRID_Y = 46, RL_ARM_CHILD_LDS = 47,
    /* settings in force once rl_init has run, not counters: packed rows 0 / 1 / 2, document-major root rows, RLHIP_DM_DIV, features per child block asked for, threads per
     * child block asked for, any column in runs, compact rows built, lazy tie-break mode (0 = off), then chunk_docs' and balance_slots' parameters */
    RL_ARM_SET_P8 = 48, RL_ARM_SET_DM_ROOT = 49, RL_ARM_SET_DM_DIV = 50, RL_ARM_SET_SUB_CHILD = 51, RL_ARM_SET_HIST_NT = 52, RL_ARM_SET_ANY_RUNS = 53,
    RL_ARM_SET_CROWS = 54, RL_ARM_SET_TIE_ON = 55, RL_ARM_SET_NODE_DIV = 56, RL_ARM_SET_NODE_MIN = 57, RL_ARM_SET_BALANCE = 58, RL_ARM_SET_BALANCE_TARGET = 59,
    RL_ARM_SET_BALANCE_MIN = 60, RL_ARM_SET_BALANCE_CAP = 61, RL_ARM_SET_NODE_CHUNK = 62, RL_ARM_SET_MAX_CHUNKS = 63,
    /* rl_adopt_model_text: launches of k_replay_scores (one per data set and chunk of trees) by arm.  The table grew behind its 64th entry for them:
     * rl_get_array copies as many entries as the caller's buffer holds, 64 at least */
    RL_ARM_REPLAY_TILED = 64,   /* rows staged into an LDS tile */
    RL_ARM_REPLAY_DIRECT = 65,  /* rows read from global memory: more than 640 features, or RLHIP_REPLAY_DIRECT */
    RL_ARM_COUNT_ = 66
};
/* The device's two exp implementations (rho of learning/tree/LambdaMART.java:383) on n arguments: the branch-free one the
 * lambda kernels use and the literal fdlibm e_exp transcription; both must equal StrictMath.exp bit for bit. */
int rl_debug_exp(const double *x, int32_t n, double *out_fast, double *out_ref);
/* The lambda kernels' divisions (rl_device.h: div_by_rcp / rcp_newton2 = the compiler's own IEEE expansion without the scaling steps that do
 * nothing on the operand ranges of learning/tree/LambdaMART.java:383 and metric/NDCGScorer.java:154) against the compiler's division.
 * den == NULL: out_fast[i] = rho(x[i]) = 1 / (1 + exp(x[i])) as the kernels evaluate it, out_ref[i] = the same through `/` and the literal e_exp.
 * den != NULL: out_fast[i] = x[i] / den[i] through the reciprocal form, out_ref[i] = x[i] / den[i].  Both pairs must be equal bit for bit. */
int rl_debug_rho(const double *x, const double *den, int32_t n, double *out_fast, double *out_ref);
/* The exact parallel evaluation of Java float running sums (`float s = 0; for (k) s += x[k];`, learning/tree/LambdaMART.java:401-408,
 * :474-483) on arbitrary data: n doubles cut into n_seg segments (seg_start[0] = 0 ... seg_start[n_seg] = n), out[s] = the float
 * sum of segment s.  stats (may be null): int32[4] = segments evaluated, window misses repaired, segments finished serially, 0. */
int rl_debug_float_chain(int32_t device, const double *x, int64_t n, const int64_t *seg_start, int32_t n_seg, float *out, int32_t *stats);
/* RL_FLAG_FAST_LEAF's reduction on arbitrary data, by the trainer's own two kernels over the identity sample list: n doubles cut into n_seg
 * segments as above, out_f64[s] = R of segment s (0.0 for an empty one), out_f32[s] = (float) out_f64[s], the value a leaf
 * output is computed from.  Either output may be NULL. */
int rl_debug_fast_sum(int32_t device, const double *x, int64_t n, const int64_t *seg_start, int32_t n_seg, double *out_f64, float *out_f32);
int rl_bin_stride(const rl_trainer *t, int32_t *stride);
/* Histogram features of an initialised trainer and the column (0-based position in feature_ids) behind each.  Equal to the data set's features
 * unless a threshold table has more than 4095 entries (-tc -1 on a column with that many distinct values, or -tc N > 4095: learning/tree/
 * LambdaMART.java:135-149): such a feature is split into runs of 4094 thresholds (HISTORY.md 10.4) and RL_ARR_NBINS / THRESHOLDS / BINS /
 * ROOT_* are shaped by THIS count.  columns may be NULL; at most cap entries are written. */
int rl_hist_features(const rl_trainer *t, int32_t *n, int32_t *columns, int32_t cap);
int rl_quant_exponent(const rl_trainer *t, int32_t *e);   /* q = rint(lambda * 2^e) in the last round */
int rl_get_array(rl_trainer *t, int32_t which, void *out, int64_t cap_bytes);

enum { RL_KERNEL_HIST_ROOT = 0, RL_KERNEL_HIST_NODE = 1, RL_KERNEL_LAMBDA = 2, RL_KERNEL_COUNT_ = 3 };
/* With RL_FLAG_TIMING: accumulated HIP-event time (ms), launch count and algorithmic bytes of a kernel
 * since the last rl_reset_timing. */
int rl_get_timing(rl_trainer *t, int32_t kernel, double *total_ms, int64_t *launches, double *alg_bytes);
/* Switch the RL_FLAG_TIMING / RL_FLAG_TIMING_NODES bits of a live trainer (bench.py times the headline region without the 30
 * per-step event pairs, then a few more rounds with them). */
int rl_set_timing_flags(rl_trainer *t, int32_t flags);
/* Memory micro-benchmarks with this library's own access patterns ("re-measure with the build's own copy kernel"),
 * also the known byte counts that calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE (tools/calib_fetch.sh):
 * mode 0 = copy (16 B per lane; reads + writes `bytes`), 1 = streaming read of `bytes`, 2 = streaming write, 3 = 32-byte row
 * gathers through an ascending index list that takes one row in `stride` (the child-node histogram pattern; 32 B row + 4 B
 * index per entry).  avg_ms = mean HIP-event time of `iters` launches, alg_bytes = algorithmic bytes of one launch.
 * Modes 4..9 = LDS atomic throughput in the histogram kernels' own LDS layout (three 256-thread blocks per CU, 16 rows of 264 int64
 * accumulators): 4 consecutive bins per wavefront, 5 a random bin of 256 per lane, 6 one bin per wavefront (same address), 7 = 5 plus the
 * 32-bit count atomic of the child passes, 8 three 32-bit atomics instead of one 64-bit one, 9 one 32-bit atomic; `bytes` = atomic groups per
 * thread, alg_bytes returns the groups of one launch (the calibration behind bench.py's lds_atomics_frac_of_measured_peak). */
int rl_debug_membench(int32_t device, int32_t mode, int64_t bytes, int32_t stride, int32_t iters, double *avg_ms, double *alg_bytes);
int rl_reset_timing(rl_trainer *t);

/* ---- Coordinate Ascent (-ranker 4, learning/CoorAscent.java) ------------------------------------------------------------
 * A linear ranker trained by rl_ca_learn: the whole learn() loop of CoorAscent.java:67-202 with the Java's double arithmetic kept
 * bit for bit.  The trials of one search direction are evaluated in one pass on the GPU (rl_ca.hip); the keep / restore
 * decisions, the weights and the feature shuffle (java.util.Random(seed), Collections.shuffle) live on the host.
 * Train metrics: RL_METRIC_NDCG / DCG / MAP / ERR and P@k and RR@k (the tree trainer and the linear rankers take these two as well;
 * LambdaRank does not). */
enum { RL_METRIC_P = 4, RL_METRIC_RR = 5 };

typedef struct rl_ca rl_ca;             /* opaque */

typedef struct {
    int32_t  n_restart;         /* CoorAscent.nRestart      default 5     (< 1: RL_ERR_INVALID; the Java ends in a NullPointerException) */
    int32_t  n_max_iteration;   /* CoorAscent.nMaxIteration default 25 */
    double   step_base;         /* CoorAscent.stepBase      default 0.05 */
    double   step_scale;        /* CoorAscent.stepScale     default 2.0 */
    double   tolerance;         /* CoorAscent.tolerance     default 0.001 */
    int32_t  regularized;       /* CoorAscent.regularized   default 0 */
    double   slack;             /* CoorAscent.slack         default 0.001 */
    int32_t  metric;            /* RL_METRIC_*: NDCG, DCG, MAP, ERR, P, RR */
    int32_t  metric_k;          /* the scorer's k (10; 0 for MAP) */
    int32_t  device;            /* HIP device ordinal */
    int64_t  seed;              /* the shuffles of one rl_ca_learn are drawn from ONE java.util.Random(seed) (the Java's is unseeded) */
    double   err_max;           /* ERRScorer.MAX (-gmax): default 16 */
} rl_ca_params;

/* One record of rl_ca_learn's trace, in the order the Java does the work. */
enum { RL_CA_RESTART = 0, RL_CA_PASS = 1, RL_CA_TRIAL = 2, RL_CA_SUCCESS = 3, RL_CA_VALID = 4 };
typedef struct {
    int32_t kind;               /* RL_CA_* */
    int32_t restart;            /* 0-based restart */
    int32_t feature;            /* index into the feature list (TRIAL / SUCCESS), else -1 */
    int32_t dir;                /* 1, -1 or 0 (TRIAL), else 0 */
    int32_t j;                  /* trial of the direction (TRIAL); pass number (PASS); else 0 */
    int32_t improved;           /* TRIAL: the score beat the restart's best (the Java prints a log line) */
    double  weight;             /* TRIAL: the feature's trial weight; SUCCESS: its weight after the L1 normalisation */
    double  score;              /* RESTART: startScore; TRIAL: the score after any -reg penalty; SUCCESS: bestScore; VALID: the restart's
                                   validation score */
} rl_ca_trace_rec;

void rl_ca_params_default(rl_ca_params *p);         /* CoorAscent.java:37-43, NDCG@10, device 0, seed 0, err_max 16 */
int  rl_ca_create(const rl_ca_params *p, rl_ca **out);
void rl_ca_destroy(rl_ca *c);
/* X: [n_docs][n_features] row-major, column f = DataPoint.getFeatureValue(features[f]), as rl_set_train.  A +-Infinity cell is
 * RL_ERR_UNSUPPORTED (the Java's cached scores turn NaN through 0 * Infinity). */
int  rl_ca_set_train(rl_ca *c, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                     int32_t n_queries, const int32_t *qkey);
int  rl_ca_set_validation(rl_ca *c, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                          const int32_t *qkey);
int  rl_ca_set_external_judgments(rl_ca *c, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count);
int  rl_ca_learn(rl_ca *c);
int  rl_ca_get_weights(const rl_ca *c, double *w, int32_t cap);
/* train: scorer.score(rank(samples)) of the final weights (not rounded); valid: the same on the validation set (0 without one) */
int  rl_ca_scores(const rl_ca *c, double *train, double *valid);
/* out may be NULL (only *n is set); at most cap records are written */
int  rl_ca_trace(const rl_ca *c, rl_ca_trace_rec *out, int64_t cap, int64_t *n);
/* CoorAscent.eval on the GPU: out[i] = 0.0 + w[0] * x[fid[0]] + w[1] * x[fid[1]] + ... in f64, feature order (CoorAscent.java:229-235).
 * X rows as rl_model_predict's (column f holds feature ID f); an ID at or beyond row_stride reads 0. */
int  rl_ca_predict(int32_t device, const int32_t *feature_ids, const double *weights, int32_t n_weights, const float *X, int64_t n_docs,
                   int32_t row_stride, double *out);

/* ---- AdaRank (-ranker 3, learning/boosting/AdaRank.java) ---------------------------------------------------------------
 * A linear ensemble of single-feature weak rankers trained by rl_ada_learn: the whole learn() loop of AdaRank.java:97-262 (both phases,
 * rollbacks, "F. REM." removals, the best model on validation data) with the Java's double arithmetic kept bit for bit.
 * The GPU builds the weak rankers' metric table once (each feature's metric on each list, the list ranked by utilities/Sorter's selection
 * sort), evaluates the candidate sums of every round and ranks / scores the ensemble after each new term (rl_ca.hip's trial kernel);
 * the selection, alpha (log), the sample weights (exp) and every decision live on the host.  Train metrics as rl_ca: NDCG, DCG, MAP, ERR,
 * P, RR (BEST is RL_ERR_UNSUPPORTED).  A round whose alpha is not finite is RL_ERR_UNSUPPORTED (the Java goes on with Infinity / NaN). */
typedef struct rl_ada rl_ada;           /* opaque */

typedef struct {
    int32_t  n_iteration;       /* AdaRank.nIteration       default 500 (-round) */
    double   tolerance;         /* AdaRank.tolerance        default 0.002 (-tolerance) */
    int32_t  train_with_enqueue;/* AdaRank.trainWithEnqueue default 1 (-noeq clears it) */
    int32_t  max_sel_count;     /* AdaRank.maxSelCount      default 5 (-max) */
    int32_t  metric;            /* RL_METRIC_*: NDCG, DCG, MAP, ERR, P, RR */
    int32_t  metric_k;          /* the scorer's k (10; 0 for MAP) */
    int32_t  device;            /* HIP device ordinal */
    double   err_max;           /* ERRScorer.MAX (-gmax): default 16 */
} rl_ada_params;

/* One record of rl_ada_learn's trace, in the order the Java does the work. */
enum { RL_ADA_ROUND = 0, RL_ADA_ROLLBACK = 1, RL_ADA_PHASE = 2 };
enum { RL_ADA_OK = 0, RL_ADA_DAMN = 1, RL_ADA_FREM = 2 };
typedef struct {
    int32_t iteration;          /* the Java's t */
    int32_t kind;               /* RL_ADA_* */
    int32_t feature;            /* index into the feature list: ROUND / ROLLBACK the selected feature; PHASE the feature taken off the
                                   queue (-1 for the first call of learn(t, withEnqueue)) */
    int32_t status;             /* ROUND: RL_ADA_OK / DAMN / FREM; PHASE: withEnqueue (1 / 0); ROLLBACK: 0 */
    double  alpha;              /* ROUND: alpha_t */
    double  train_score;        /* ROUND: trainedScore (the ensemble's metric on the training data, not rounded) */
    double  valid_score;        /* ROUND: scorer.score(rank(validationSamples)) (0 without a validation set) */
} rl_ada_trace_rec;

void rl_ada_params_default(rl_ada_params *p);       /* AdaRank.java:37-40, NDCG@10, device 0, err_max 16 */
int  rl_ada_create(const rl_ada_params *p, rl_ada **out);
void rl_ada_destroy(rl_ada *a);
/* X as rl_ca_set_train (column f = DataPoint.getFeatureValue(features[f])); NaN and +-Infinity cells are refused as there */
int  rl_ada_set_train(rl_ada *a, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                      int32_t n_queries, const int32_t *qkey);
int  rl_ada_set_validation(rl_ada *a, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                           const int32_t *qkey);
int  rl_ada_set_external_judgments(rl_ada *a, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count);
int  rl_ada_learn(rl_ada *a);
/* the final model: n_rankers (fid = feature index, repeats allowed) and weights in ensemble order; fid / weight may be NULL (only
 * *n is set); at most cap entries are written */
int  rl_ada_get_model(const rl_ada *a, int32_t *fid, double *weight, int32_t cap, int32_t *n);
/* train: scorer.score(rank(samples)) of the final model (not rounded); valid: the same on the validation set (0 without one) */
int  rl_ada_scores(const rl_ada *a, double *train, double *valid);
int  rl_ada_trace(const rl_ada *a, rl_ada_trace_rec *out, int64_t cap, int64_t *n);
/* debug: the weak-ranker table, out[f * n_queries + q] = scorer.score(WeakRanker(f).rank(list q)) (cap >= n_features * n_queries) */
int  rl_ada_debug_weak_table(const rl_ada *a, double *out, int64_t cap);

/* ---- RankBoost (-ranker 2, learning/boosting/RankBoost.java) -----------------------------------------------------------
 * An ensemble of threshold weak rankers h(x) = [x[fid] > threshold] trained by rl_rb_learn: all of RankBoost.init() and learn()
 * (:143-346) with the Java's double arithmetic kept bit for bit.  The training lists are put into getCorrectRanking()'s
 * order (utilities/Sorter's unstable selection sort on the labels) by rl_rb_set_train; pair indices, the train metric's tie order and
 * rl_rb_debug_potentials refer to that order.  The GPU keeps one weight per crucial pair (label_j > label_k), computes the potentials,
 * the candidates' serial r chains (one per feature, staged through LDS), the pair update with the Z_t chain and both metrics of every
 * round; the arg-max over (feature, threshold), alpha_t (log) and exp(+-alpha_t) live on the host.  Train metrics as rl_ca.  A training
 * set without a crucial pair, a round whose alpha_t, Z_t or exp(alpha_t) is not finite (or Z_t == 0) and a pair table that does not
 * fit are RL_ERR_UNSUPPORTED. */
typedef struct rl_rb rl_rb;             /* opaque */

typedef struct {
    int32_t  n_iteration;       /* RankBoost.nIteration default 300 (-round) */
    int32_t  n_threshold;       /* RankBoost.nThreshold default 10 (-tc); <= 0: every feature value is a candidate */
    int32_t  metric;            /* RL_METRIC_*: NDCG, DCG, MAP, ERR, P, RR */
    int32_t  metric_k;          /* the scorer's k (10; 0 for MAP) */
    int32_t  device;            /* HIP device ordinal */
    int32_t  keep_potentials;   /* debug: the potentials of rounds 1 .. keep_potentials stay readable (default 0) */
    double   err_max;           /* ERRScorer.MAX (-gmax): default 16 */
} rl_rb_params;

/* One record per round of rl_rb_learn. */
typedef struct {
    int32_t iteration;          /* the Java's t */
    int32_t feature;            /* index into the feature list of the selected weak ranker */
    double  threshold;          /* its threshold */
    double  max_r;              /* maxR of learnWeakRanker (:96-141) */
    double  r_t;                /* R_t = Z_{t-1} * maxR */
    double  alpha;              /* alpha_t */
    double  z_t;                /* Z_t: the serial sum of the updated pair weights */
    double  train_score;        /* scorer.score(rank(samples)) after the round (not rounded) */
    double  valid_score;        /* the same on the validation set (0 without one) */
} rl_rb_trace_rec;

void rl_rb_params_default(rl_rb_params *p);         /* RankBoost.java:38-39, NDCG@10, device 0, err_max 16 */
int  rl_rb_create(const rl_rb_params *p, rl_rb **out);
void rl_rb_destroy(rl_rb *r);
/* X as rl_ca_set_train (column f = DataPoint.getFeatureValue(features[f])); NaN and +-Infinity cells are refused as there */
int  rl_rb_set_train(rl_rb *r, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                     int32_t n_queries, const int32_t *qkey);
int  rl_rb_set_validation(rl_rb *r, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                          const int32_t *qkey);
int  rl_rb_set_external_judgments(rl_rb *r, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count);
int  rl_rb_learn(rl_rb *r);
/* the final model: n weak rankers (fid = feature index, repeats allowed), thresholds and weights in ensemble order; the arrays may be
 * NULL (only *n is set); at most cap entries are written */
int  rl_rb_get_model(const rl_rb *r, int32_t *fid, double *threshold, double *weight, int32_t cap, int32_t *n);
/* train: scorer.score(rank(samples)) of the final model (not rounded); valid: the same on the validation set (0 without one) */
int  rl_rb_scores(const rl_rb *r, double *train, double *valid);
int  rl_rb_trace(const rl_rb *r, rl_rb_trace_rec *out, int64_t cap, int64_t *n);
/* debug: potential[list][doc] as updatePotential (:75-89) left it in round `round` (1 .. keep_potentials), n_docs doubles, the
 * documents of each list in getCorrectRanking()'s order */
int  rl_rb_debug_potentials(const rl_rb *r, int32_t round, double *out, int64_t cap);
/* RankBoost.eval on the GPU: out[i] = 0.0 + w[0] * [x[fid[0]] > thr[0]] + w[1] * [x[fid[1]] > thr[1]] + ... in f64, ensemble order
 * (RankBoost.java:348-355).  X rows as rl_ca_predict's; an ID at or beyond row_stride reads 0. */
int  rl_rb_predict(int32_t device, const int32_t *feature_ids, const double *thresholds, const double *weights, int32_t n_rankers,
                   const float *X, int64_t n_docs, int32_t row_stride, double *out);

/* ---- Linear Regression (-ranker 9, learning/LinearRegRank.java) ---------------------------------------------------------
 * The least-squares ranker trained by rl_lr_learn: all of LinearRegRank.learn() (:44-100) and solve() (:188-239) with the Java's double
 * arithmetic kept bit for bit.  With nVar = the training set's column count, the regressors are columns 0 .. nVar - 2 plus
 * a constant: the LAST of the nVar columns is not fitted (the Java's nVar is the largest feature id, not one more), and weight[nVar - 1]
 * is the constant's.  The GPU accumulates xTx (its upper triangle: the matrix is bitwise symmetric) and xTy, every cell its own serial
 * f64 sum over the documents in order, and scores / ranks both sets; the ridge term and the elimination without pivoting run on the
 * host.  Train metrics as rl_ca.  A pivot that is 0 or not finite and weights that are not all finite are RL_ERR_UNSUPPORTED. */
typedef struct rl_lr rl_lr;             /* opaque */

typedef struct {
    double   lambda;            /* LinearRegRank.lambda default 1E-10 (-L2); added to the diagonal unless it is 0.0 */
    int32_t  metric;            /* RL_METRIC_*: NDCG, DCG, MAP, ERR, P, RR */
    int32_t  metric_k;          /* the scorer's k (10; 0 for MAP) */
    int32_t  device;            /* HIP device ordinal */
    double   err_max;           /* ERRScorer.MAX (-gmax): default 16 */
} rl_lr_params;

void rl_lr_params_default(rl_lr_params *p);         /* LinearRegRank.java:26, NDCG@10, device 0, err_max 16 */
int  rl_lr_create(const rl_lr_params *p, rl_lr **out);
void rl_lr_destroy(rl_lr *r);
/* X: [n_docs][n_features] row-major, column f = DataPoint.getFeatureValue(f + 1) (NOT the feature list: the fit ignores it); NaN and
 * +-Infinity cells are refused as in rl_ca_set_train */
int  rl_lr_set_train(rl_lr *r, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                     int32_t n_queries, const int32_t *qkey);
int  rl_lr_set_validation(rl_lr *r, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                          const int32_t *qkey);
int  rl_lr_set_external_judgments(rl_lr *r, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count);
/* optional, after rl_lr_set_train.  n_var: the Java's nVar when the sets carry more columns than that (1 .. n_features; 0 = n_features).
 * eval_cols: the columns eval() reads, features[i] - 1 in feature-list order (-1 reads 0: an id no row has, under -missingZero);
 * NULL = columns 0 .. n_features - 1.  More eval columns than n_var is RL_ERR_UNSUPPORTED in rl_lr_learn (the Java ends in an
 * ArrayIndexOutOfBoundsException). */
int  rl_lr_set_features(rl_lr *r, int32_t n_var, const int32_t *eval_cols, int32_t n_eval);
int  rl_lr_learn(rl_lr *r);
/* weight[0 .. nVar): w may be NULL (only *n is set); at most cap entries are written */
int  rl_lr_get_weights(const rl_lr *r, double *w, int32_t cap, int32_t *n);
/* train: scorer.score(rank(samples)) of the weights (not rounded); valid: the same on the validation set (0 without one) */
int  rl_lr_scores(const rl_lr *r, double *train, double *valid);
/* debug: xTx [nVar][nVar] and xTy [nVar] as accumulated, BEFORE the ridge term (readable also after a refused solve); both may be NULL
 * (only *n_var is set); cap = the nVar the buffers were sized for */
int  rl_lr_debug_gram(const rl_lr *r, double *xtx, double *xty, int32_t cap, int32_t *n_var);
/* debug: ms of the accumulation kernel (device events), of the host solve and of scoring + ranking both sets; the register block used */
int  rl_lr_debug_times(const rl_lr *r, double *gram_ms, double *solve_ms, double *score_ms, int32_t *register_block);
/* LinearRegRank.eval on the GPU: out[i] = weights[n_weights - 1], then += weights[t] * x[feature_ids[t]] for t < n_features, in f64
 * (LinearRegRank.java:103-109: it starts from the bias).  X rows as rl_ca_predict's; an ID at or beyond row_stride reads 0;
 * n_features > n_weights is RL_ERR_UNSUPPORTED. */
int  rl_lr_predict(int32_t device, const int32_t *feature_ids, int32_t n_features, const double *weights, int32_t n_weights, const float *X,
                   int64_t n_docs, int32_t row_stride, double *out);

/* ---- Neural-net models (RankNet -ranker 1, LambdaRank 5, ListNet 7: learning/neuralnet/) ---------------------------------
 * Scoring only: the forward pass RankNet.eval (RankNet.java:336-349), which LambdaRank and ListNet inherit, with the Java's double
 * arithmetic kept bit for bit.  Training is built for ListNet and RankNet (below), not for LambdaRank.  The network is the one RankNet.wire() (:87-110)
 * makes: layer 0 holds the n_features inputs and a bias neuron of output 1.0, then come the hidden layers, then one output neuron;
 * every neuron past layer 0 computes 1.0 / (1.0 + exp(-wsum)) (LogiFunction.java:18-20) of wsum = 0.0, += source.output * weight over
 * its inLinks in order (Neuron.computeOutput, Neuron.java:68-76): the previous layer's neurons in order, the bias LAST. */
typedef struct rl_net rl_net;           /* opaque */

/* which kernel the last rl_net_predict / rl_net_predict_device of a handle took (rl_net_debug_path) */
enum { RL_NET_PATH_NONE = 0, RL_NET_PATH_LDS = 1, RL_NET_PATH_GLOBAL = 2 };

/* feature_ids[k] = the feature ID input neuron k reads (RankNet.java:339-341: p.getFeatureValue(features[k])).  hidden_sizes: the
 * n_hidden layer sizes (NULL when n_hidden is 0).  weights, in INPUT order: for each layer l = 1 .. n_hidden + 1 a row-major matrix
 * [n_l][n_{l-1} + 1], row j = the weights of neuron j's inLinks (sources in order, the bias last), n_0 = n_features and the last
 * n_l = 1 -- not the order of a model file, whose lines follow the outLinks (RankNet.toString :356-372).  The weights are uploaded
 * once.  A wrong n_weights, n_features < 1 or a layer size < 1 is RL_ERR_INVALID; no gfx950 device is RL_ERR_NO_DEVICE. */
int  rl_net_create(int32_t device, const int32_t *feature_ids, int32_t n_features, const int32_t *hidden_sizes, int32_t n_hidden,
                   const double *weights, int32_t n_weights, rl_net **out);
void rl_net_destroy(rl_net *net);
/* RankNet.eval (:336-349) of every row: out[i] = the output neuron's output, a double in [0, 1].  X rows as rl_lr_predict's and
 * rl_model_predict's (column f holds feature ID f); an ID at or beyond row_stride reads 0. */
int  rl_net_predict(rl_net *net, const float *X, int64_t n_docs, int32_t row_stride, double *out);
/* The same on device pointers (dX: n_docs * row_stride floats, dOut: n_docs doubles), enqueued on `stream` (a hipStream_t, NULL = the
 * default stream) without any synchronisation.  Calls on one handle must be ordered by the caller (a network too large for the
 * LDS kernel keeps its hidden outputs in a scratch of the handle). */
int  rl_net_predict_device(rl_net *net, const float *dX, int64_t n_docs, int32_t row_stride, double *dOut, void *stream);
/* debug: RL_NET_PATH_* of the last predict call (Neuron.computeOutput :68-76 is the same arithmetic in both kernels) */
int  rl_net_debug_path(const rl_net *net, int32_t *path);

/* ---- ListNet training (-ranker 7, learning/neuralnet/ListNet.java, ListNeuron.java) --------------------------------------
 * ListNet.learn() (:101-140) with the Java's double arithmetic kept bit for bit: n_features inputs and a bias neuron feed
 * one logistic output neuron, and the n_features + 1 weights are updated once per ranked list, list after list, for n_epochs epochs.
 * After every epoch both sets are scored and ranked; with a validation set the weights of the epoch whose score is strictly above every
 * earlier one (and above 0.0) are kept and restored after the last epoch.  The Java draws the start weights from an unseeded Random:
 * here the caller gives them (rl_ln_set_weights), the library never sees a seed.  Train metrics as rl_ca.  Weights that are not all
 * finite after an epoch are RL_ERR_UNSUPPORTED (the message names the epoch); a validation set on which no epoch scores above 0.0 is
 * RL_ERR_NO_BEST (the Java's restoreBestModelOnValidation throws). */
typedef struct rl_ln rl_ln;             /* opaque */

typedef struct {
    int32_t  n_epochs;          /* ListNet.nIteration       default 1500 (-epoch); < 0: RL_ERR_INVALID */
    double   learning_rate;     /* Neuron.learningRate as ListNet.init() sets it, default 0.00001; not finite: RL_ERR_INVALID */
    int32_t  metric;            /* RL_METRIC_*: NDCG, DCG, MAP, ERR, P, RR */
    int32_t  metric_k;          /* the scorer's k (10; 0 for MAP) */
    int32_t  device;            /* HIP device ordinal */
    double   err_max;           /* ERRScorer.MAX (-gmax): default 16 */
} rl_ln_params;

typedef struct {
    int32_t epoch;              /* 1 .. n_epochs */
    int32_t saved;              /* 1 if this epoch became the best on validation */
    double  train;              /* scorer.score(rank(samples)) after the epoch, not rounded */
    double  valid;              /* the same on the validation set (0 without one) */
} rl_ln_trace_rec;

void rl_ln_params_default(rl_ln_params *p);         /* 1500, 0.00001, NDCG@10, device 0, err_max 16 */
int  rl_ln_create(const rl_ln_params *p, rl_ln **out);
void rl_ln_destroy(rl_ln *h);
/* X: [n_docs][n_features] row-major, column k = the value input neuron k reads (getFeatureValue(features[k])); cells as rl_ca_set_train */
int  rl_ln_set_train(rl_ln *h, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                     int32_t n_queries, const int32_t *qkey);
int  rl_ln_set_validation(rl_ln *h, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                          const int32_t *qkey);
int  rl_ln_set_external_judgments(rl_ln *h, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count);
/* the start weights in inLinks order: inputs 0 .. n_features - 1, the bias last.  n != n_features + 1 is RL_ERR_INVALID.  Required
 * before the handle learns (without them, or without a training set, learning is RL_ERR_INVALID); a later set_train discards them */
int  rl_ln_set_weights(rl_ln *h, const double *w, int32_t n);
int  rl_ln_learn(rl_ln *h);
/* after learning: the restored best on validation, or the last epoch's.  w may be NULL (only *n is set); at most cap entries are written */
int  rl_ln_get_weights(const rl_ln *h, double *w, int32_t cap, int32_t *n);
/* train / valid: scorer.score(rank(.)) of those weights (not rounded; valid is 0 without a validation set) */
int  rl_ln_scores(const rl_ln *h, double *train, double *valid);
/* one record per epoch; out may be NULL (only *n is set); at most cap records are written */
int  rl_ln_trace(const rl_ln *h, rl_ln_trace_rec *out, int64_t cap, int64_t *n);
/* debug: the final weights' output for every document of the training (validation != 0: validation) set, as the scoring kernel wrote it */
int  rl_ln_debug_doc_scores(const rl_ln *h, int32_t validation, double *out, int64_t cap);
/* debug: ms of all epoch kernels together (device events) and of scoring + ranking both sets after every epoch (host clock) */
int  rl_ln_debug_times(const rl_ln *h, double *epoch_ms, double *score_ms);

/* ---- RankNet and LambdaRank training (-ranker 1 / 5, learning/neuralnet/RankNet.java, LambdaRank.java, Neuron.java) ------
 * RankNet.learn() (:290-334) with the Java's double arithmetic kept bit for bit: the network of rl_net_create (n_features
 * inputs and a bias neuron, n_hidden hidden layers, one output neuron).  Per epoch every ranked list is walked in order: the outputs of
 * all its documents are computed with the weights as they are (batchFeedForward), then the weights are updated once per document, in
 * order, from the pairs (i, j) with label_i > label_j (batchBackPropagate: Neuron.computeDelta / updateDelta / updateWeight).  After
 * every epoch both sets are scored and ranked and the mis-ordered pairs of the training set are counted (estimateLoss :230-252, the
 * count only); the best-on-validation rule, the restore and the refusals are rl_ln's.  The caller gives the start weights
 * (rl_rn_set_weights); the library never sees a seed.
 *
 * The same handle trains LambdaRank after rl_rn_set_lambdarank(h, 1): learn() is RankNet's, and per list the documents
 * are first re-ranked by the current weights (stable, descending); the pairs of a document are then every j whose label differs, with
 * target 1 where label_i > label_j and 0 elsewhere, and every pair carries the float weight |swapChange[i][j]| * sign of the train
 * metric's scorer (NDCG, DCG, MAP or ERR) on the re-ranked list.  Its messages say "LambdaRank".  With this, every ranker of RankLib
 * trains. */
typedef struct rl_rn rl_rn;             /* opaque */

typedef struct {
    int32_t  n_epochs;          /* RankNet.nIteration       default 100 (-epoch); < 0: RL_ERR_INVALID */
    double   learning_rate;     /* Neuron.learningRate as RankNet.init() sets it, default 0.00005 (-lr); not finite: RL_ERR_INVALID */
    int32_t  n_hidden;          /* RankNet.nHiddenLayer     default 1 (-layer); < 0: RL_ERR_INVALID */
    const int32_t *hidden_sizes;/* [n_hidden] neurons per hidden layer (-node), copied by rl_rn_create; NULL: 10 each, the default of
                                   RankNet.nHiddenNodePerLayer; a size < 1: RL_ERR_INVALID */
    int32_t  metric;            /* RL_METRIC_*: NDCG, DCG, MAP, ERR, P, RR */
    int32_t  metric_k;          /* the scorer's k (10; 0 for MAP) */
    int32_t  device;            /* HIP device ordinal */
    double   err_max;           /* ERRScorer.MAX (-gmax): default 16 */
} rl_rn_params;

typedef struct {
    int32_t epoch;              /* 1 .. n_epochs */
    int32_t saved;              /* 1 if this epoch became the best on validation */
    int64_t misordered;         /* estimateLoss's misorderedPairs on the training set after the epoch */
    int64_t total_pairs;        /* init()'s totalPairs: the training pairs with different labels (the same in every record) */
    double  train;              /* scorer.score(rank(samples)) after the epoch, not rounded */
    double  valid;              /* the same on the validation set (0 without one) */
} rl_rn_trace_rec;

void rl_rn_params_default(rl_rn_params *p);         /* 100, 0.00005, 1 hidden layer of 10, NDCG@10, device 0, err_max 16 */
int  rl_rn_create(const rl_rn_params *p, rl_rn **out);
void rl_rn_destroy(rl_rn *h);
/* X, labels, qoff, qkey as rl_ln_set_train's; the lists are walked in the given order */
int  rl_rn_set_train(rl_rn *h, const float *X, int64_t n_docs, int32_t n_features, const float *labels, const int32_t *qoff,
                     int32_t n_queries, const int32_t *qkey);
int  rl_rn_set_validation(rl_rn *h, const float *X, int64_t n_docs, const float *labels, const int32_t *qoff, int32_t n_queries,
                          const int32_t *qkey);
int  rl_rn_set_external_judgments(rl_rn *h, int32_t validation, const double *ideal_dcg, const int32_t *rel_doc_count);
/* the start weights in rl_net_create's layout: per layer l = 1 .. n_hidden + 1 a row-major [n_l][n_{l-1} + 1], the bias last.  A wrong n
 * is RL_ERR_INVALID.  Required before the handle learns (without them, or without a training set, learning is RL_ERR_INVALID); a later
 * set_train discards them */
int  rl_rn_set_weights(rl_rn *h, const double *w, int32_t n);
/* on != 0: the handle trains LambdaRank (LambdaRank.java) instead of RankNet; 0 switches back.  A null handle is RL_ERR_INVALID, a call
 * after rl_rn_learn RL_ERR_STATE; on with a train metric other than NDCG, DCG, MAP and ERR (P, RR: their swap changes are not built) is
 * RL_ERR_UNSUPPORTED.  None of these looks at the device */
int  rl_rn_set_lambdarank(rl_rn *h, int32_t on);
int  rl_rn_learn(rl_rn *h);
/* after learning, in the same layout: the restored best on validation, or the last epoch's.  w may be NULL (only *n is set) */
int  rl_rn_get_weights(const rl_rn *h, double *w, int32_t cap, int32_t *n);
int  rl_rn_scores(const rl_rn *h, double *train, double *valid);
/* one record per epoch; out may be NULL (only *n is set); at most cap records are written */
int  rl_rn_trace(const rl_rn *h, rl_rn_trace_rec *out, int64_t cap, int64_t *n);
/* debug: the final weights' output for every document of the training (validation != 0: validation) set, as the scoring kernel wrote it */
int  rl_rn_debug_doc_scores(const rl_rn *h, int32_t validation, double *out, int64_t cap);
/* debug: ms of all epoch kernels together (device events) and of scoring, ranking and pair counting after every epoch (host clock) */
int  rl_rn_debug_times(const rl_rn *h, double *epoch_ms, double *score_ms);

/* ---- the Analyzer's Fisher randomisation test (stats/RandomPermutationTest.java:23-53) ------------------------------
 * base [n] and targets [n_targets][n] hold the per-ranked-list performances in the iteration order of the baseline's HashMap, the
 * "all" entry included.  Permutations perm_begin .. perm_begin + perm_count - 1 of every target are evaluated on the device, one lane
 * each: permutation p draws its n / 10 + 1 ten-bit chunks from java.util.Random(seed)'s nextDouble draws [p D, (p + 1) D), D = n / 10 + 1
 * (the Java's Random is unseeded: the seed is this library's extension); where a bit is 1, b[j] and t[j] swap places; the two means are
 * serial f64 sums from 0.0 in array order and one IEEE division by n; pDiff = |mean(pb) - mean(pt)|.
 * out_count[k]: permutations of target k with pDiff >= trueDiff (a NaN on either side never counts).  out_true_diff[k] =
 * |mean(base) - mean(target k)|, computed on the host by the same literal loop.  out_pdiff: NULL, or every pDiff, [n_targets][perm_count].
 * perm_begin splits a large run over several calls: the counts of the pieces add up to the whole run's.
 * RL_ERR_INVALID: a null pointer, n < 1, n_targets < 1 or > 65535, perm_count < 1 or > 2^31 - 1, perm_begin < 0, or
 * (perm_begin + perm_count) * 2 * (n / 10 + 1) LCG steps not below 2^63.  RL_ERR_NO_DEVICE without a gfx950 device: there is no CPU
 * fallback. */
int  rl_perm_test(int device, const double *base, const double *targets, int n, int n_targets, int64_t seed, int64_t perm_begin,
                  int64_t perm_count, int64_t *out_count, double *out_true_diff, double *out_pdiff);
/* debug (tools/perm_bench.py): add_ns = ns per f64 add of one dependent chain on the device (one wavefront; chain_adds and 2 * chain_adds
 * adds between device events, the difference); with base and target not NULL also host_ms / host_count: the time and the count of the
 * Java's loop as written (digit strings, copies into pb / pt) over permutations 0 .. perm_count - 1 on one host thread, the tool's
 * yardstick.  The host part runs first and needs no device. */
int  rl_debug_perm_calib(int device, const double *base, const double *target, int n, int64_t seed, int64_t perm_count, int64_t chain_adds,
                         double *add_ns, double *host_ms, int64_t *host_count);

/* ---- test-time evaluation: rank and score every list of a file in one pass (eval/Evaluator.java:915-944) --------------
 * scores [n_docs] (f64) and labels [n_docs] hold the documents of n_lists ranked lists, list q at qoff[q] .. qoff[q + 1] - 1.  Every list is
 * ranked stable and descending by score (MergeSorter.sort(double[], false): -0.0 ties with 0.0, +-Infinity are ordinary values) and its
 * metric is taken on the device as the Java scorer's serial f64 chain over the ranked labels, bit for bit:
 * RL_METRIC_NDCG / DCG / MAP / ERR / P / RR and RL_METRIC_BEST (Best@k, reporting only: no trainer accepts it).  k is the scorer's k (MAP
 * ignores it; plain RR has k = 0 and scores 0, as written), err_max is ERRScorer.MAX.
 * qkey, ideal_dcg, rel_doc_count: NULL, or [n_lists] with the meaning they have in the trainers' external judgments: for NDCG a list
 * whose ideal_dcg entry is not NaN is scored against it, and otherwise the FIRST list with its qkey decides the ideal DCG of every later
 * list with the same key (NDCGScorer's idealGains cache; without qkey every list is its own key); for MAP rel_doc_count replaces the
 * list's own count of relevant documents.
 * out_metric [n_lists]: the value of every list; their mean is the caller's (the Java adds them serially in list order).  out_pos: NULL,
 * or [n_docs], the 0-based position of every document in its list's ranking.  out_ideal: NULL, or [n_lists], the ideal DCG every list was
 * scored against (NaN for the other metrics).
 * Checked on the host before any device call -- RL_ERR_INVALID: a null scores / labels / qoff / out_metric, n_lists or n_docs < 1, qoff
 * not starting at 0, not ending at n_docs or not strictly increasing, an unknown metric, a negative label, a negative rel_doc_count, a NaN
 * score (the message names the list: the counting rank is undefined on NaN, rank such a list on the host); RL_ERR_UNSUPPORTED: a label of
 * 2^24 or more.  RL_ERR_NO_DEVICE without a gfx950 device: there is no CPU fallback. */
enum { RL_METRIC_BEST = 6 };
int  rl_eval_lists(int32_t device, int32_t metric, int32_t k, double err_max, const double *scores, const float *labels, int64_t n_docs,
                   const int32_t *qoff, int32_t n_lists, const int32_t *qkey, const double *ideal_dcg, const int32_t *rel_doc_count,
                   double *out_metric, int32_t *out_pos, double *out_ideal);
/* debug (tools/eval_bench.py): ms between two device events around the kernel launches of this thread's last rl_eval_lists call (the
 * uploads before them and the copies back after them are not in it) */
int  rl_debug_eval_times(double *kernel_ms);

/* ---- feature normalisation: -norm sum | zscore | linear over every list of a file in one pass (features/SumNormalizor.java,
 * ZScoreNormalizor.java, LinearNormalizer.java) -------------------------------------------------------------------------
 * X is [n_docs][stride] float32, row-major, on the host; it is normalised in place (upload, one kernel, one copy back).  Row d is a
 * DataPoint's fVals: column 0 is never a feature, and with row_len (NULL, or [n_docs]) row d holds features 1 .. row_len[d] - 1 only.
 * List q is rows qoff[q] .. qoff[q + 1] - 1, the rules of rl_eval_lists.  cols [n_cols] are the feature ids to normalise = column indices
 * into a row, without duplicates (the caller removes them, as Normalizer.removeDuplicateFeatures does); their order is irrelevant.
 * Every list is normalised on its own, column by column, operation by operation as the Java does it: a NaN cell reads as 0.0f
 * (getFeatureValue), the sums are serial f64 sums over the list's documents in order, linear is float arithmetic with Math.min / Math.max
 * (-0.0f below +0.0f) from Float.MAX_VALUE / Float.MIN_VALUE.  times >= 1 applies the normaliser that many times in a row to every list,
 * each pass reading what the one before wrote (the -kcv flow normalises every list nFold * nFold times).
 * Only the cells the Java would setFeatureValue change; every other cell keeps its bits (a NaN's payload too): column 0, columns not in
 * cols, cells past a row's row_len, and the columns of a list the Java leaves alone (sum: norm > 0 false; zscore: std > 0 false, NaN
 * included -- a list of one document).
 * Checked on the host before any device call -- RL_ERR_INVALID: a null X / qoff / cols; n_docs, n_lists, n_cols or times < 1;
 * stride < 2; qoff not starting at 0, not ending at n_docs or not strictly increasing; an unknown kind; a column < 1 or >= stride; a
 * duplicate column; a row_len entry < 1 or > stride; a requested column at or past some row's row_len (the message names the first such
 * row and feature: -missingZero and the Java's error texts stay with the caller).  RL_ERR_NO_DEVICE without a gfx950 device: there is
 * no CPU fallback. */
enum { RL_NORM_SUM = 0, RL_NORM_ZSCORE = 1, RL_NORM_LINEAR = 2 };
int  rl_normalize_lists(int32_t device, int32_t kind, float *X, int64_t n_docs, int32_t stride, const int32_t *row_len, const int32_t *qoff,
                        int32_t n_lists, const int32_t *cols, int32_t n_cols, int32_t times);
/* debug (tools/norm_bench.py): ms between two device events around the kernel launch of this thread's last rl_normalize_lists call (the
 * upload before it and the copy back after it are not in it) */
int  rl_debug_normalize_times(double *kernel_ms);

/* ---- a tree model after every requested number of trees, one pass over a file ----------------------------------------
 * A model of T trees has stages t = 1 .. T: stage t is the ensemble of its first t trees with their weights.  A document's stage score
 * is the prefix of Ensemble.eval's float chain (learning/tree/Ensemble.java:110-116): s_t = (float)((double)s_{t-1} + (double)out_t *
 * (double)w_t), s_0 = 0.0f, out_t the leaf Split.eval reaches (a column at or beyond row_stride reads 0).  stages [n_stages] holds tree
 * counts, strictly increasing, each in [1, T].  X and labels are HOST pointers, as in rl_model_predict.
 * rl_model_predict_stages: out [n_stages][n_docs], the stage scores.
 * rl_model_eval_stages: out_metric [n_stages][n_lists] is what rl_eval_lists returns for the stage's scores widened to f64 -- the stable
 * descending rank (-0.0 ties with 0.0, +-Infinity are ordinary values) and the scorer's serial f64 chain, all seven metrics, bit for
 * bit; qoff, qkey, ideal_dcg, rel_doc_count, metric, k, err_max and out_ideal are rl_eval_lists' arguments with its rules and error
 * texts, and the ideal DCGs are resolved once per call.  A (stage, list) cell whose scores hold a NaN has out_nan = 1 and value 0.0 and
 * is not ranked (the caller ranks it on the host); every other cell has out_nan = 0.  The stages are processed in chunks whose device
 * scratch -- 4 bytes per document and stage, 16 where a list is longer than 6 144 documents -- stays within scratch_bytes (0 = 256 MiB);
 * a chunk holds at least one stage.  The result does not depend on the chunking.
 * RL_ERR_INVALID, the message naming the argument: a null pointer, n_stages < 1, a stage out of range or out of order, row_stride < 1,
 * scratch_bytes < 0, a model without trees. */
int  rl_model_predict_stages(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *stages, int32_t n_stages,
                             float *out);
int  rl_model_eval_stages(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const float *labels, const int32_t *qoff,
                          int32_t n_lists, const int32_t *qkey, const double *ideal_dcg, const int32_t *rel_doc_count, int32_t metric,
                          int32_t k, double err_max, const int32_t *stages, int32_t n_stages, int64_t scratch_bytes, double *out_metric,
                          uint8_t *out_nan, double *out_ideal);
/* debug (tools/stages_bench.py): ms between device events around the tree-walking and around the ranking launches of this thread's
 * last rl_model_predict_stages / rl_model_eval_stages call, summed over its chunks */
int  rl_debug_stage_times(double *walk_ms, double *rank_ms);

/* ---- permutation feature importance of a tree model, one pass over a file --------------------------------------------
 * A cell (c, r), c < n_columns, r < n_repeats, is column columns[c] under repeat r; donor [n_repeats][n_docs] holds document indices
 * in [0, n_docs).  The permuted score of document i in cell (c, r) is Ensemble.eval's float chain (learning/tree/Ensemble.java:110-116,
 * s = (float)((double)s + (double)out * (double)w), s_0 = 0.0f) on row i with the value of column columns[c] taken from row
 * donor[r][i]; a column at or beyond row_stride reads 0 on both sides, so such a cell equals the base.  The base is the unpermuted
 * scores (and their per-list values); it goes through the same kernels as one extra cell.  donor[r] need not be a permutation: any
 * in-range map is legal, and the same donor[r] serves every column of repeat r.  columns may repeat and need no order.  X, labels,
 * columns and donor are HOST pointers; rows, labels and tables are uploaded once per call.
 * rl_model_predict_permuted: out [n_columns][n_repeats][n_docs], out_base [n_docs] (may be NULL).
 * rl_model_eval_permuted: out_metric [n_columns][n_repeats][n_lists] is what rl_eval_lists returns for the cell's scores widened to f64
 * -- all seven metrics, the stable descending rank with -0.0 tying 0.0, bit for bit what the materialised permuted matrix gives through
 * rl_model_predict and rl_eval_lists; out_base [n_lists] likewise for the base.  A (cell, list) whose scores hold a NaN has out_nan
 * (out_base_nan) = 1 and value 0.0 and is not ranked, exactly as rl_model_eval_stages treats a (stage, list).  The list arguments are
 * rl_eval_lists' with its rules and error texts.  The cells are processed in chunks whose device scratch -- 4 bytes per document and
 * cell, 16 where a list is longer than 6 144 documents -- stays within scratch_bytes (0 = 256 MiB); a chunk holds at least one cell.
 * The result does not depend on the chunking.  Inside a chunk the kernel takes RL_PERMUTED_BATCH cells per document at a time.
 * RL_ERR_INVALID, the message naming the argument: a null pointer, n_columns < 1, n_repeats < 1, a negative column, a donor entry
 * outside [0, n_docs), row_stride < 1, scratch_bytes < 0, a model without trees (the model is looked at after the other arguments).
 * rl_model_debug_path reports RL_MODEL_PATH_PERMUTED after either call: one kernel serves packed and unpacked models. */
#ifndef RL_PERMUTED_BATCH
#define RL_PERMUTED_BATCH 16
#endif
enum { RL_MODEL_PATH_PERMUTED = 3 };
int  rl_model_predict_permuted(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                               const int32_t *donor, int32_t n_repeats, float *out_base, float *out);
int  rl_model_eval_permuted(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const float *labels, const int32_t *qoff,
                            int32_t n_lists, const int32_t *qkey, const double *ideal_dcg, const int32_t *rel_doc_count, int32_t metric,
                            int32_t k, double err_max, const int32_t *columns, int32_t n_columns, const int32_t *donor, int32_t n_repeats,
                            int64_t scratch_bytes, double *out_base, uint8_t *out_base_nan, double *out_metric, uint8_t *out_nan,
                            double *out_ideal);
/* debug (tools/importance_bench.py): as rl_debug_stage_times, for this thread's last rl_model_predict_permuted / rl_model_eval_permuted
 * call */
int  rl_debug_permuted_times(double *walk_ms, double *rank_ms);

/* ---- per-document feature contributions of a tree model, one pass over a file ----------------------------------------
 * Which features put a document where it is: Saabas path attribution, as XGBoost's pred_contribs with approx_contribs has it.  The
 * model has trees t = 0 .. T-1 with float weights w_t; the nodes j of a tree are numbered in the pre-order of the model text; a leaf
 * has feature -1 and a float `out`.
 * WALK: Split.eval as everywhere.  At a split on feature id f: v = (f < row_stride) ? row[f] : 0, left iff v <= thr (a NaN goes right).
 * COVER: c[t][j], uint64, counts the background rows whose walk in tree t visits node j; c[t][0] is the number of background rows.
 * Model text holds no counts, so rl_model_cover counts them on a background file; with accumulate != 0 the call's counts are added to
 * those the model has.  n_docs == 0 is legal: it leaves all counts zero, or with accumulate as they were.
 * NODE VALUE: val[t][j], f64, children first.  A leaf's is (double)out.  A split's, with children l, r and a = c[l], b = c[r] (a = b = 1
 * where a + b == 0: the background never reached the node), is ((double)a * val[l] + (double)b * val[r]) / (double)(a + b), the
 * operations in that order, each rounded (no FMA).  The values are made again after every rl_model_cover call.
 * CONTRIBUTIONS of a row, f64: the requested feature ids are columns[0 .. C-1]; there are C + 2 slots, 0 .. C-1, rest = C, bias = C + 1.
 *     acc[0 .. C+1] = +0.0
 *     for t = 0 .. T-1:  W = (double)w_t;  acc[bias] = acc[bias] + W * val[t][0];  j = 0
 *         while j is a split on feature f and the walk goes on to node n:
 *             d = W * (val[t][n] - val[t][j]);  s = the place of f in columns, or rest;  acc[s] = acc[s] + d;  j = n
 * so every slot is one serial f64 chain, in tree order, then path order.  out is [n_docs][C + 2], row-major.  columns == NULL (then
 * n_columns only has to be >= 0): the columns are the model's features in rl_model_features' order, and rest is exactly +0.0.  A requested
 * id the model never splits on gets +0.0.
 * The slots of a row sum to the f64 sum over the trees of (double)w_t * (double)out of the leaf reached, up to f64 rounding (a
 * telescoping sum).  That is NOT rl_model_predict's score, which is Ensemble.eval's float chain: the two differ by float rounding.
 * X, columns and out are HOST pointers.  The rows are processed in chunks whose device buffers -- the rows and 8 (C + 2) bytes of
 * output per row -- stay within scratch_bytes (0 = 256 MiB); a chunk holds at least one row.  The result does not depend on the
 * chunking, nor on the number of column passes the kernel needs when C + 2 slots do not fit its LDS (rl_debug_contrib_passes).
 * rl_model_get_cover: *n_nodes is the tree's node count; count and value [cap] receive its covers and node values (either may be NULL).
 * RL_ERR_INVALID, the message naming the argument, before the device is touched: a null model / X / out, n_docs < 0, row_stride < 1,
 * n_columns < 0, columns given with n_columns < 1, a negative column, a column listed twice, scratch_bytes < 0, a model without trees,
 * tree out of range, cap below the tree's node count (*n_nodes is still set).  RL_ERR_STATE: rl_model_predict_contribs or
 * rl_model_get_cover before any rl_model_cover.  RL_ERR_UNSUPPORTED: more than 2^31 rows per call, a tree of more than 5 103 nodes (the LDS).
 * rl_model_debug_path reports RL_MODEL_PATH_COVER / RL_MODEL_PATH_CONTRIBS after rl_model_cover / rl_model_predict_contribs. */
int  rl_model_cover(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, int32_t accumulate);
int  rl_model_cover_rows(const rl_model *m, int64_t *n_rows);
int  rl_model_get_cover(const rl_model *m, int32_t tree, uint64_t *count, double *value, int32_t cap, int32_t *n_nodes);
int  rl_model_predict_contribs(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns,
                               int32_t n_columns, int64_t scratch_bytes, double *out);
enum { RL_MODEL_PATH_COVER = 4, RL_MODEL_PATH_CONTRIBS = 5 };
/* out [n_docs]: per row the f64 sum over the trees, in tree order, s = s + (double)w_t * (double)out of the leaf the walk reaches -- what
 * the row's contributions sum to up to f64 rounding (local accuracy), from a walk of its own.  Needs no cover.  The same row checks. */
int  rl_model_predict_leaf_sums(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, double *out);
/* debug (tools/contrib_bench.py): ms between device events around the k_model_cover launches of this thread's last rl_model_cover call
 * and around the k_model_contribs launches of its last rl_model_predict_contribs call, summed over the chunks */
int  rl_debug_contrib_times(double *cover_ms, double *walk_ms);
/* debug: the column passes of this thread's last rl_model_predict_contribs call */
int  rl_debug_contrib_passes(int32_t *passes);

/* ---- exact TreeSHAP contributions of a tree model, one pass over a file ------------------------------------------------
 * rl_model_predict_contribs with the Shapley values themselves in place of Saabas' path attribution: XGBoost's pred_contribs without
 * approx_contribs, path-dependent TreeSHAP.  WALK, COVER c[t][j], NODE VALUE val[t][j], W = (double)w_t, the slots (columns[0 .. C-1],
 * rest = C, bias = C + 1, columns == NULL) and the row rule v = (f < row_stride) ? row[f] : 0 are those of the section above.
 * VALUE OF A FEATURE SET: for tree t, a row and a set S of feature ids, v_S(j) of a node j is (double)out at a leaf; at a split on f in S
 * v_S of the child the row's walk takes; at a split on f not in S (a v_S(l) + b v_S(r)) / (a + b), a = c[l], b = c[r], a = b = 1 where
 * a + b == 0.  v_{}(0) = val[t][0]; v_all(0) is the row's leaf output.  The contribution of feature i in tree t is its Shapley value
 * phi_i(t) in the game S -> v_S(0) over the features the tree splits on; the model's is the sum over t of W phi_i(t); the bias slot is the
 * sum over t of W val[t][0], the chain of rl_model_predict_contribs' bias slot and therefore its bits.
 * COMPUTED FORM (path form: every row meets every leaf).  Every slot is one serial f64 chain, in tree order, then leaf order (the
 * pre-order of the model text), then element order.  The ELEMENTS e = 1 .. d of a leaf are the distinct features of its root-to-leaf
 * path in order of first appearance, each with its slot, with z_e -- the f64 product, in root-to-leaf order, of the ratios
 * (double)c[child on the path] / (double)(a + b) of the path's splits on the feature (a = b = 1 where a + b == 0: a split the background
 * never reached gives 1/2) -- and with those splits' conditions.  Per row o_e = 1.0 if the row's own decision (v <= thr goes left,
 * anything else, a NaN included, goes right) is the path's direction at EVERY split of the element, else 0.0.  Tables, one f64 quotient
 * each: A[l][i] = (i+1)/(l+1), B[l][i] = (l-i)/(l+1), U[l][i] = (l+1)/(i+1), R[l][i] = (l+1)/(l-i).  Per (row, leaf):
 *     w[0] = 1.0
 *     for l = 1 .. d:   w[l] = 0.0;   for i = l-1 .. 0:   w[i+1] = w[i+1] + o_l * (w[i] * A[l][i]);   w[i] = (z_l * w[i]) * B[l][i]
 *     for e = 1 .. d, unless o_e == z_e (possible only at 0 and 1: the term is zero, and a division by a zero cover stays out):
 *         o_e == 1:   tot = 0; nxt = w[d];   for i = d-1 .. 0:   tmp = nxt * U[d][i];  tot = tot + tmp;  nxt = w[i] - (tmp * z_e) * B[d][i]
 *         o_e == 0:   tot = 0;               for i = d-1 .. 0:   tot = tot + w[i] * R[d][i];             then tot = tot / z_e
 *         acc[slot_e] = acc[slot_e] + ((tot * (o_e - z_e)) * (double)out_leaf) * W
 * every operation rounded, no FMA.  (The o_e == 0 arm is the sum of w[i] / (z_e B[d][i]) with the division by z_e taken out of the sum
 * and 1 / B as a table: one division per element instead of d.)  A single-leaf tree adds to bias only.  out is [n_docs][C + 2] as
 * rl_model_predict_contribs has it; a requested id the model never splits on gets +0.0, and rest is exactly +0.0 under columns == NULL.
 * The slots of a row sum to rl_model_predict_leaf_sums' value up to f64 rounding (local accuracy: a property, not a definition).
 * ACCURACY: the unwind subtracts.  Against the same form in exact arithmetic, a row's slots were together within 1 x 2^-52 x (the sum
 * over trees and leaves of |W out|) on ordinary models, but 3 856 of those units off on a chain of 30 DISTINCT features: twelve of the
 * 52 mantissa bits, fourteen in the worst row seen.  Less than half the mantissa, but worth knowing.
 * The result does not depend on the grid, the block width, the chunking under scratch_bytes or the number of column passes
 * (rl_debug_shap_passes).  rl_model_shap_limits: *max_path is the model's longest element list, *limit the most the kernel takes (32:
 * every tree of up to 33 leaves whatever its shape); it needs no cover.
 * RL_ERR_INVALID: the cases of rl_model_predict_contribs, the message naming this entry point.  RL_ERR_STATE: before any
 * rl_model_cover.  RL_ERR_UNSUPPORTED, before the device is touched: more than 2^31 rows per call; a path of more than *limit distinct
 * features, the message naming tree and leaf.  rl_model_debug_path reports RL_MODEL_PATH_SHAP afterwards. */
int  rl_model_predict_shap(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns,
                           int32_t n_columns, int64_t scratch_bytes, double *out);
enum { RL_MODEL_PATH_SHAP = 6 };
int  rl_model_shap_limits(const rl_model *m, int32_t *max_path, int32_t *limit);
/* debug (tools/shap_bench.py): ms between device events around the k_model_shap launches of this thread's last rl_model_predict_shap
 * call, summed over the chunks; and the column passes of that call */
int  rl_debug_shap_times(double *walk_ms);
int  rl_debug_shap_passes(int32_t *passes);

/* ---- SHAP interaction values of a tree model, one pass over a file ------------------------------------------------------
 * Which features work together: XGBoost's pred_interactions beside pred_contribs.  WALK, COVER, NODE VALUE, W = (double)w_t, the slots
 * (columns[0 .. C-1], rest = C, bias = C + 1, columns == NULL), the row rule, the ELEMENTS of a leaf with z_e, o_e and their conditions,
 * the tables A, B, U, R and the three steps start / extend / unwind are those of the two sections above; no FMA.
 * MEANING: for tree t with player set N, the features it splits on, k = |N|, and features p != q,
 *     PHI_pq(t) = sum over S in N without {p, q} of |S|! (k - |S| - 2)! / (2 (k - 1)!) * (v_{S+p+q} - v_{S+p} - v_{S+q} + v_S)
 * with the v_S(0) of rl_model_predict_shap; the model's value is the sum over t of W PHI_pq(t), added into the cell [slot_p][slot_q].
 * Pairs whose two features share a slot are not walked at all (without columns == NULL that can only happen in rest).
 * RESULT: out [n_docs][C + 2][C + 2] f64.  Cell [i][j], i != j, both <= C, has i as the CONDITIONED slot and j as the ATTRIBUTED slot
 * (XGBoost's layout).
 * OFF-DIAGONAL CELL: one serial f64 chain from +0.0, in tree order, then leaf order (the pre-order of the model text), then conditioned
 * element c in element order, then attributed element e in element order.  For a leaf with elements 1 .. d, d >= 2, and a conditioned
 * element c with o_c != z_c: the reduced list is the leaf's elements without c, in order, of length d - 1; start and extend run on it
 * with the tables at l = 1 .. d - 1; the unwind runs with the tables at d - 1 for every e != c of the reduced list with o_e != z_e and
 * slot_e != slot_c and gives tot; then, each rounded and in this order,
 *     x = (tot * (o_e - z_e)) * (double)out_leaf;   x = x * ((o_c - z_c) * 0.5);   x = x * W;   cell[slot_c][slot_e] = cell[slot_c][slot_e] + x
 * The conditioned element is never divided by, so z_c == 0 with o_c == 1 is taken.  A leaf with one element, and a single-leaf tree,
 * add nothing here.
 * DIAGONAL CELL, i <= C: r = phi_i, the bits rl_model_predict_shap gives for that slot and row with the same columns; for j = 0 .. C
 * ascending, j != i: r = r - out[i][j]; out[i][i] = r.
 * BIAS: out[C+1][C+1] is the bits of the SHAP bias slot; every other cell of row C + 1 and column C + 1 is +0.0.  A requested id the
 * model never splits on has +0.0 in its whole row and column; under columns == NULL so has rest.
 * PROPERTIES, not definitions: row i sums to phi_i and the matrix to rl_model_predict_leaf_sums' value up to f64 rounding; out[i][j]
 * and out[j][i] are equal in exact arithmetic but are two f64 chains and may differ in their last bits: both are kept as computed,
 * nothing is symmetrised (that would change what a restricted column list gives).
 * The result does not depend on the grid, the block width, the chunking -- per row the row itself, 8 (C + 2)^2 bytes of result and
 * 8 (C + 2) bytes of SHAP values stay within scratch_bytes (0 = 256 MiB), a chunk holds at least one row -- or the number of column
 * passes (rl_debug_interact_passes).
 * RL_ERR_INVALID: the cases of rl_model_predict_contribs, the message naming this entry point.  RL_ERR_STATE: before any
 * rl_model_cover.  RL_ERR_UNSUPPORTED, before the device is touched: more than 2^31 rows per call; a path of more than 32 distinct
 * features (rl_model_shap_limits); more than 65 535 conditioned slots (C + 1).  n_docs == 0 is legal and launches nothing.
 * rl_model_debug_path reports RL_MODEL_PATH_INTERACT afterwards. */
int  rl_model_predict_interactions(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns,
                                   int32_t n_columns, int64_t scratch_bytes, double *out);
enum { RL_MODEL_PATH_INTERACT = 8 };
/* debug (tools/interact_bench.py): ms between device events around the k_model_interact and k_interact_finish launches, and around the
 * k_model_shap launches, of this thread's last rl_model_predict_interactions call, summed over the chunks; and the column passes of
 * k_model_interact in that call */
int  rl_debug_interact_times(double *walk_ms, double *shap_ms);
int  rl_debug_interact_passes(int32_t *passes);

/* ---- partial dependence and ICE curves of a tree model, one pass over a file -------------------------------------------
 * How the score moves as one feature moves.  columns[0 .. C-1] are feature ids, each >= 0, in any order, repeats allowed; grid_off
 * [C + 1] is a CSR offset array, grid_off[0] == 0, strictly increasing; grid [grid_off[C]] holds f32 grid values.  CELL j, grid_off[c] <=
 * j < grid_off[c+1], is column columns[c] set to grid[j].  The grid values of one column are strictly ascending under <: no NaN, no equal
 * values, not -0.0 beside 0.0; +-Infinity are ordinary values.
 * The ICE score of document i in cell j is Ensemble.eval's float chain (learning/tree/Ensemble.java:110-116, s = (float)((double)s +
 * (double)out * (double)w), s_0 = 0.0f; v <= thr goes left, a NaN in another column goes right) on row i TAKEN AS PADDED WITH ZEROS TO ANY
 * WIDTH, column columns[c] then set to grid[j]: a column at or beyond row_stride is substituted all the same (unlike the permuted cells
 * above, where both sides read 0).  Bit for bit what the matrix materialised on the host, widened with zeros where needed, gives through
 * rl_model_predict.  The BASE is the unsubstituted scores, out_base [n_docs] (may be NULL).
 * Per cell two f64 sums in ONE FIXED ORDER that depends on nothing but n_docs: with RL_PARTIAL_SUM_BLOCK = 256 (part of this
 * definition, not a kernel's block size), partial p is the serial chain over the documents [256 p, 256 p + 256) in document order,
 * starting from +0.0; the total is the serial chain over the partials in order, starting from +0.0.  S1 sums (double)ice; S2 sums d * d,
 * d = (double)ice - (double)base, every operation rounded, no FMA.  out_mean[j] = S1 / (double)n_docs is the partial-dependence value;
 * out_shift2[j] = S2 / (double)n_docs is the mean squared move away from the document's own score.  NaN and Infinity propagate as IEEE
 * gives them; there are no flags.  out_ice [cells][n_docs] f32 may be NULL: then nothing of that size crosses the bus.
 * X, columns, grid_off, grid and the outputs are HOST pointers; rows and tables are uploaded once per call.  The cells are processed in
 * chunks whose device scratch -- 4 bytes per document and cell, plus the base -- stays within scratch_bytes (0 = 256 MiB); a chunk
 * holds at least one cell.  The result does not depend on the chunking.  Inside a chunk the kernel takes up to RL_PARTIAL_BATCH cells
 * of one column per document at a time.
 * RL_ERR_INVALID, the message naming the argument, all checked before the model so that a machine without a device reaches them: null
 * X, columns, grid_off, grid, out_mean or out_shift2; n_docs < 1; row_stride < 1; n_columns < 1; a negative column; grid_off[0] != 0, an
 * empty or descending grid_off; a grid value that is NaN or not greater than its predecessor ("grid[c][g] = ..."); scratch_bytes < 0.
 * Then a null model and a model without trees.  RL_ERR_UNSUPPORTED: more than 2^31 documents or cells per call.
 * rl_model_debug_path reports RL_MODEL_PATH_PARTIAL afterwards: one kernel serves packed and unpacked models. */
#ifndef RL_PARTIAL_BATCH
#define RL_PARTIAL_BATCH 16
#endif
#ifndef RL_PARTIAL_SUM_BLOCK
#define RL_PARTIAL_SUM_BLOCK 256
#endif
enum { RL_MODEL_PATH_PARTIAL = 7 };
int  rl_model_predict_partial(rl_model *m, const float *X, int64_t n_docs, int32_t row_stride, const int32_t *columns, int32_t n_columns,
                              const int32_t *grid_off, const float *grid, int64_t scratch_bytes, float *out_base, double *out_mean,
                              double *out_shift2, float *out_ice);
/* debug (tools/partial_bench.py): ms between device events around the walking and around the reducing launches of this thread's last
 * rl_model_predict_partial call, summed over its chunks */
int  rl_debug_partial_times(double *walk_ms, double *reduce_ms);

#ifdef __cplusplus
}
#endif
#endif
