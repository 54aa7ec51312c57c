// rl_knobs.h -- every RLHIP_* environment knob the library reads, read here and nowhere else (DESIGN.md "Environment knobs").
//
// None of them is API: they select measured-and-kept alternatives, test aids and profiling output.  A handle reads its knobs ONCE, when it
// is created (rl_create, rl_model_from_text, rl_lr_create), and keeps them: a knob set between two handles takes effect for the second one,
// and nothing on a timed path looks at the environment.
//
// Three parse rules, named by the helper an entry uses:
//   present(X)      the knob is set, to anything
//   unless_zero(X)  on by default, off only when set to 0
//   nonzero(X)      off by default, on when set to something other than 0
// and plain values (atoi / atoll / atof) with the clamp written at the entry.  A default that depends on run-time sizes is not known here:
// such a knob is an Opt ("unset", or the parsed value) and its site writes `knob.or_else(default)`.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace rl {

struct Opt {
    bool set = false; int v = 0;
    int or_else(int dflt) const { return set ? v : dflt; }
};

namespace knob {
inline bool present(const char *name) { return getenv(name) != nullptr; }
inline bool unless_zero(const char *name) { const char *e = getenv(name); return !(e && atoi(e) == 0); }
inline bool nonzero(const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; }
inline int value(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
inline Opt opt(const char *name) { const char *e = getenv(name); Opt o; if (e) { o.set = true; o.v = atoi(e); } return o; }
template <class Fn> inline Opt opt(const char *name, Fn clamp) { Opt o = opt(name); if (o.set) o.v = clamp(o.v); return o; }
}  // namespace knob

// the tree trainer's knobs (rl_trainer::knobs, filled by rl_create)
struct Knobs {
    // -- growth step: chunks, grids, kernel choice
    Opt node_div, balance_target, balance_min, balance_cap, fin_split, hist_nt, hist_grid, trace_tree;
    // (the initialisers are the defaults of read(): a trainer that rl_create did not make -- rl_debug_float_chain's -- runs the default paths)
    int node_min = 256, sub_child = 16, p8 = 1, dm_div = 1, csc_dens = 3, crows = -1, step_ahead = 1, dist_ahead = 1, piece_force = 0, lam_side = 1, tiny_min = 4096;
    size_t hist_ldspad = 0, tie_walk_max = 24576, tie_slack = (size_t)64 << 20;
    double dist_timeout_s = 300.0;
    bool balance = true, skip_last = true, step2 = true, sel2_wide = true, fused_quant = true, score_stream = true, dm_root = false, lam_compact = false;
    bool rank_split = false, runs_off = false, jhist_v1 = false, lambda_unfused = false, tie_off = false, tie_no_xdefer = false, tie_walk = false, tie_force_regrow = false;
    bool dist_count_pass = false, dist_host_plan = false, dist_owner_chains = false, tie_prof = false, chain_prof = false, steplog = false, replay_direct = false, refit_direct = false;

    void read()
    {
        using namespace knob;
        node_div = opt("RLHIP_NODE_DIV", [](int v) { return std::max(1, v); });                 // chunks a child node is cut into (default: by the feature count)
        node_min = std::max(256, value("RLHIP_NODE_MIN", 256) & ~255);                          // smallest chunk of a child node, a multiple of 256
        balance = unless_zero("RLHIP_BALANCE");                                                 // balanced chunks for the steps that fill the chip
        balance_target = opt("RLHIP_BALANCE_TARGET", [](int v) { return std::max(8, v & ~7); });   // rows of the balanced child-pass grid (default: by the group count)
        balance_min = opt("RLHIP_BALANCE_MIN", [](int v) { return std::max(1, v); });           // steps of at most this many chunks are not balanced (default: target / 2)
        balance_cap = opt("RLHIP_BALANCE_CAP", [](int v) { return std::max(1024, v & ~255); }); // largest balanced chunk (the site caps it at kChunk, its default)
        skip_last = unless_zero("RLHIP_SKIP_LAST");                                             // no histogram for the children of a tree's last split (one GPU only)
        step2 = unless_zero("RLHIP_STEP2");                                                     // k_fin2 + k_select2 (rl_step2.inc); 0: the fused finish / bookkeeping kernel
        sel2_wide = unless_zero("RLHIP_SELECT2_WIDE");                                          // k_select2<true> on 161 .. 768 histogram features; 0: k_select
        fin_split = opt("RLHIP_FIN_SPLIT", [](int v) { return v != 0 ? 1 : 0; });               // k_hist_finish_wide + k_select forced on / off (default: by live features per CU)
        sub_child = value("RLHIP_SUB_CHILD", 16); if (sub_child != 4 && sub_child != 8) sub_child = 16;   // features per child-pass block: 4 or 8 spread a group over more blocks
        hist_nt = opt("RLHIP_HIST_NT");                                                         // threads per child-pass block (512 / 1024 have instantiations; default kThreads)
        hist_grid = opt("RLHIP_HIST_GRID");                                                     // blocks of the bounded child-pass grid (default 1024); set: also no balanced grid
        hist_ldspad = (size_t)value("RLHIP_HIST_LDSPAD", 0);                                    // extra dynamic LDS per child-pass block, a measuring aid (28 KB caps a CU at two blocks)
        fused_quant = unless_zero("RLHIP_FUSED_QUANT");                                         // the root pass quantises the lambdas itself; 0: a pass of its own
        score_stream = unless_zero("RLHIP_SCORE_STREAM");                                       // score update streams the documents; 0: it walks the leaves' lists
        step_ahead = std::max(0, value("RLHIP_STEP_AHEAD", 1));                                 // growth steps in flight beyond the progress word; 0: enqueue all L-1 blindly
        // -- data layout chosen by rl_init
        p8 = value("RLHIP_P8", 1);                                                              // packed rows: 0 none, 1 root pass, 2 child passes too
        dm_root = nonzero("RLHIP_DM_ROOT");                                                     // document-major rows for the root pass as well
        dm_div = std::max(0, value("RLHIP_DM_DIV", 1));                                         // document-major rows for a node of cnt documents when cnt * dm_div <= N; 0: never
        runs_off = present("RLHIP_RUNS_OFF");                                                   // never take the instantiation for columns whose bins come in runs
        crows = value("RLHIP_CROWS", -1);                                                       // compact rows for the child passes: 0 off, 1 on for every group, unset (< 0): per group by density
        csc_dens = value("RLHIP_CSC_DENS", 3);                                                  // sparse root pass for groups with at most 1 / dens of their cells outside the mode bins; 0: never
        jhist_v1 = present("RLHIP_JHIST_V1");                                                   // RL_FLAG_JAVA_ORDER: the first Java-order histogram kernel on every table
        // -- ranking and lambdas
        tiny_min = std::max(0, value("RLHIP_TINY_MIN", 4096));                                  // lists of <= 16 documents get kernels of their own from this many of them
        rank_split = present("RLHIP_RANK_SPLIT");                                               // k_rank_wave + k_rank_block instead of k_rank_mixed
        lambda_unfused = present("RLHIP_LAMBDA_UNFUSED");                                       // pair-term matrix instead of the LDS-resident fused lambda kernel
        lam_side = std::max(0, std::min(3, value("RLHIP_LAMBDA_SIDE", 1)));                     // side streams the lambda kernels of the length classes use
        lam_compact = nonzero("RLHIP_LAMBDA_COMPACT");                                          // NDCG / DCG pair terms from per-wavefront lists of the active pairs
        // -- resume (rl_resume.inc)
        replay_direct = present("RLHIP_REPLAY_DIRECT");                                         // k_replay_scores reads the rows from global memory instead of an LDS tile (cross-check, tools/resume_bench.py)
        // -- refit (rl_refit.inc)
        refit_direct = present("RLHIP_REFIT_DIRECT");                                           // k_refit_route reads the rows from global memory instead of an LDS tile (cross-check, tools/refit_bench.py)
        // -- lazy Java-order tie-break (rl_tie.inc, rl_tie_host.inc)
        tie_off = present("RLHIP_TIE_OFF");                                                     // keep the first candidate of an exact tie
        tie_no_xdefer = present("RLHIP_TIE_NO_XDEFER");                                         // stall on ties over several features instead of deferring them
        tie_walk = present("RLHIP_TIE_WALK");                                                   // always the literal walk (the cross-check of the speculative chains)
        tie_walk_max = (size_t)(getenv("RLHIP_TIE_WALK_MAX") ? atoll(getenv("RLHIP_TIE_WALK_MAX")) : 24576ll);   // chains up to this many documents take the literal walk
        tie_slack = (size_t)std::max(0ll, getenv("RLHIP_TIE_SLACK") ? atoll(getenv("RLHIP_TIE_SLACK")) : 64ll << 20);   // test aid: bytes the scratch arena's first reservation adds to its fixed part; 0: a speculative resolution grows the arena
        tie_force_regrow = present("RLHIP_TIE_FORCE_REGROW");                                  // test aid: every verified batch reports a miss, the tree is grown again
        // -- sharded runs (rl_dist.inc)
        dist_ahead = std::max(0, value("RLHIP_DIST_STEP_AHEAD", 1));                            // growth steps enqueued beyond the last one the host has seen
        dist_timeout_s = getenv("RLHIP_DIST_TIMEOUT_S") ? std::max(1.0, atof(getenv("RLHIP_DIST_TIMEOUT_S"))) : 300.0;   // operational: a rank gives up waiting for its own device
        dist_count_pass = present("RLHIP_DIST_COUNT_PASS");                                     // count pass + two-pass partition instead of this rank's own root counts
        dist_host_plan = present("RLHIP_DIST_HOST_PLAN");                                       // the leaf exchange's plan on the host, behind a stream synchronisation
        dist_owner_chains = present("RLHIP_DIST_OWNER_CHAINS");                                 // the leaf-owner exchange instead of the distributed float chains
        piece_force = value("RLHIP_PIECE_FORCE_MISS", 0);                                       // test aid: every piece behind a rank's first is re-evaluated
        // -- profiling output
        tie_prof = present("RLHIP_TIE_PROF");                                                   // host microseconds per phase of resolve_ties, printed by rl_destroy
        chain_prof = present("RLHIP_CHAIN_PROF");                                               // float-chain counters, printed by rl_destroy
        steplog = present("RLHIP_STEPLOG");                                                     // per-step log on the device (RL_ARR_STEPLOG)
        trace_tree = opt("RLHIP_TRACE_TREE");                                                   // block time stamps of this tree (RL_ARR_TRACE)
    }
};

// the scoring-only model's knobs (rl_model::knobs, filled by rl_model_from_text: set the variable before the model is created)
struct EvalKnobs {
    bool deal = true, phased = true, generic = false;
    void read()
    {
        using namespace knob;
        deal = unless_zero("RLHIP_EVAL_DEAL");          // a tile's trees, sorted by depth, dealt round the walkers; 0: eight consecutive ranks to each walker
        phased = unless_zero("RLHIP_EVAL_PHASED");      // walkers drop finished trees in phases; 0: every walk as long as the deepest
        generic = present("RLHIP_EVAL_GENERIC");        // k_model_eval instead of the tiled kernel (cross-checks in the tests)
    }
};

// Linear Regression (rl_lr::rb_knob, read by rl_lr_create): the register block of k_lr_gram, 1 / 2 / 4; anything else: chosen by lr_pick_rb's model
inline int read_lr_rb_knob() { const int v = knob::value("RLHIP_LR_RB", 0); return (v == 1 || v == 2 || v == 4) ? v : 0; }

// ListNet training (rl_ln::skip, read by rl_ln_create): a measuring aid of tools/ln_bench.py -- k_ln_epoch without its forward pass (1), its
// sum chain (2) or its update (4); the weights such a run leaves are meaningless.  Anything else: the whole kernel
inline int read_ln_skip_knob() { const int v = knob::value("RLHIP_LN_SKIP", 0); return (v == 1 || v == 2 || v == 4) ? v : 0; }

// RankNet training (rl_rn::skip, read by rl_rn_create): a measuring aid of tools/rn_bench.py -- k_rn_epoch without its forward pass (1), its
// deltas (2) or its update (4); the weights such a run leaves are meaningless.  Anything else: the whole kernel
inline int read_rn_skip_knob() { const int v = knob::value("RLHIP_RN_SKIP", 0); return (v == 1 || v == 2 || v == 4) ? v : 0; }

}  // namespace rl
