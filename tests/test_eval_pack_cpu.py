"""The tiled scoring kernel's packed format without a GPU: rl_eval_pack_host.h's eval_pack through
tools/eval_pack_host_check.cpp on hand-built models of tests/tree_models.py, under both settings of RLHIP_EVAL_DEAL and RLHIP_EVAL_PHASED.
tests/eval_pack_restatement.py holds what the program prints against the trees rule by rule and replays k_model_eval_tiled's walk on it in
numpy; the scores must be tree_models.eval_ensemble_np's, bit for bit.  Neither the library nor a device is needed."""
import os
import subprocess

import numpy as np
import pytest

import eval_pack_restatement as EP
import tree_models as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = ["count_1", "count_8", "count_33", "count_39", "count_57", "count_65", "depth_extremes", "depth_0_31", "depth_equal", "deep_at_0",
      "deep_at_7", "deep_at_31", "accum_specials", "thresholds", "col0_garbage", "nodes_79", "feat_254"]
REFUSED = {"nan_leaf": "a leaf output is NaN", "feature_0": "a feature id is below 1",
           "nodes_81": "a tile of trees is more than a block prefetches", "feat_255": "a column offset does not fit 16 bits"}
SETTINGS = [(1, 1), (1, 0), (0, 1), (0, 0)]              # (deal, phased)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_pack")
    exe = str(d / "eval_pack_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "eval_pack_host_check.cpp"),
                           os.path.join(ROOT, "ranklib_amd", "csrc", "rl_model.cpp"), "-o", exe])
    texts = {}

    def packed(name, deal, phased):
        if name not in texts:
            c = TM.case(name)[0]
            texts[name] = str(d / (name + ".txt"))
            with open(texts[name], "w") as f:
                f.write(TM.model_text(c.trees, c.weights))
        out = subprocess.run([exe, texts[name], str(deal), str(phased)], capture_output=True, text=True, check=True).stdout
        return EP.parse(out)
    return packed


@pytest.mark.parametrize("deal,phased", SETTINGS)
@pytest.mark.parametrize("name", OK)
def test_a_packed_model_is_well_formed_and_walks_to_the_reference_scores(run, name, deal, phased):
    c, want = TM.case(name)
    pk = run(name, deal, phased)
    assert pk["ok"] and c.tiled, pk["why"]
    assert (pk["docs"], pk["tile"], pk["per"], pk["parts"], pk["phases"]) == (TM.DOCS, TM.TILE, TM.PER, TM.PARTS, TM.PHASES)
    EP.check_structure(pk, c.trees, phased)
    got = EP.replay(pk, c.weights, c.rows)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), TM.same_scores(got, want)


@pytest.mark.parametrize("name", OK)
def test_the_settings_change_the_walkers_not_the_nodes(run, name):
    pks = [run(name, d, p) for d, p in SETTINGS]
    assert all(np.array_equal(pk["nodes"], pks[0]["nodes"]) for pk in pks)
    assert np.array_equal(pks[0]["perm"], pks[1]["perm"]) and np.array_equal(pks[2]["perm"], pks[3]["perm"])      # phased moves no tree
    for a, b in zip(pks[0]["perm"], pks[2]["perm"]):
        if (a != EP.NONE).all():                         # dealt: walker p holds the ranks p, p + parts, .. of the undealt order
            assert a.reshape(TM.PARTS, TM.PER).T.reshape(-1).tolist() == b.tolist()
        else:
            assert a.tolist() == b.tolist()              # a partial tile is not dealt


@pytest.mark.parametrize("deal,phased", SETTINGS)
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_model_the_packing_refuses(run, name, deal, phased):
    c = TM.case(name)[0]
    pk = run(name, deal, phased)
    assert not pk["ok"] and not c.tiled
    assert pk["why"] == REFUSED[name]
    assert pk["maxcol"] == max(int(t["feature"].max()) for t in c.trees)
    assert pk["nodes"].size == 0 and pk["perm"].size == 0 and pk["meta"].size == 0
