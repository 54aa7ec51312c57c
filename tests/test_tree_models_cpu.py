"""The two references of the tree-ensemble scoring tests against each other, without a GPU: for every model and row set that
tests/test_gpu_model_eval.py scores, `tree_models.eval_ensemble_np` (numpy) and the oracle's `ro_eval_flat_model` (C) agree -- bit for
bit outside NaN results, NaN where the other is NaN.  Also the builder itself: the text it writes, and what the cases are meant to hold."""
import numpy as np
import pytest

import oracle_ffi as O
import tree_models as TM


@pytest.mark.parametrize("name", sorted(TM.CASES))
def test_numpy_reference_equals_the_oracle(name):
    c, want = TM.case(name)
    got = O.eval_flat_model(c.trees, c.rows, n_threads=8 if len(c.rows) > 100000 else 1, weights=c.weights)
    assert TM.same_scores(got, want) is None, TM.same_scores(got, want)
    # the comparison is not empty: most documents end on a number, and the documents do not all end on the same one
    assert np.count_nonzero(~np.isnan(want)) * 2 >= len(want), "%d of %d scores are NaN" % (np.count_nonzero(np.isnan(want)), len(want))
    assert c.rows.shape[1] == 1 or len(np.unique(want.view(np.uint32))) > 1      # (one column: every feature reads 0)


def test_the_vectorised_reference_is_the_literal_one():
    """Split.eval and Ensemble.eval written out per document and node, on the cases with the special values"""
    for name in ("thresholds", "accum_specials", "width_5", "feature_0"):
        c, want = TM.case(name)
        ref = np.zeros(len(c.rows), np.float32)
        with np.errstate(all="ignore"):
            for i, row in enumerate(c.rows):
                s = np.float32(0)
                for t, w in zip(c.trees, c.weights):
                    nd = 0
                    while t["feature"][nd] != -1:
                        f = int(t["feature"][nd])
                        v = row[f] if f < len(row) else np.float32(0)
                        nd = int(t["left"][nd]) if v <= t["threshold"][nd] else int(t["right"][nd])
                    s = np.float32(np.float64(s) + np.float64(t["output"][nd]) * np.float64(w))
                ref[i] = s
        assert TM.same_scores(want, ref) is None, (name, TM.same_scores(want, ref))


def test_same_scores_rule():
    a = np.array([1.0, -0.0, np.nan, np.inf], np.float32)
    assert TM.same_scores(a, a.copy()) is None
    assert TM.same_scores(-a, a) is not None                                      # 0.0 is not -0.0
    assert TM.same_scores(np.array([1.0, -0.0, -np.nan, np.inf], np.float32), a) is None       # a NaN's sign is not compared
    assert TM.same_scores(np.array([1.0, -0.0, 5.0, np.inf], np.float32), a) is not None
    assert TM.same_scores(np.array([np.nan, -0.0, np.nan, np.inf], np.float32), a) is not None  # NaN where the reference has a number
    assert TM.same_scores(np.nextafter(a, np.float32(2)), a) is not None


def test_shapes():
    g = TM.Gen(np.random.default_rng(3))
    assert len(TM.single_leaf(g)["feature"]) == 1 and TM.depth_of(TM.single_leaf(g)) == 0
    assert len(TM.stump(g)["feature"]) == 3 and TM.depth_of(TM.stump(g)) == 1
    assert len(TM.balanced(g, 4)["feature"]) == 31 and TM.depth_of(TM.balanced(g, 4)) == 4
    for side in ("left", "right"):
        t = TM.chain(g, 39, side)
        assert len(t["feature"]) == 79 and TM.depth_of(t) == 39
        inner = np.nonzero(t["feature"] != -1)[0]
        assert np.all(t["feature"][t[side][inner[:-1]]] != -1)                    # every split's `side` child is the next split
    t = TM.random_tree(g, 17)
    assert np.count_nonzero(t["feature"] == -1) == 17 and len(t["feature"]) == 33


def test_text_is_what_java_prints():
    t = TM.flatten(TM.S(3, np.float32(1.4e-45), TM.L(-0.0), TM.S(1, np.nan, TM.L(np.inf), TM.L(TM.F32_MAX))))
    text = TM.model_text([t, TM.flatten(TM.L(0.1))], [np.float32(1e-40), np.float32(-0.25)])
    for piece in ('<tree id="1" weight="1.0E-40">', '<tree id="2" weight="-0.25">', "<feature>3 </feature>", "<threshold> 1.4E-45 </threshold>",
                  "<threshold> NaN </threshold>", "<output>-0.0 </output>", "<output>Infinity </output>", "<output>3.4028234663852886E38 </output>",
                  "<output>0.10000000149011612 </output>", '<split pos="left">', '<split pos="right">'):
        assert piece in text, piece
    assert text.count("<split") == 2 + 4 and text.endswith("</ensemble>\n")


def test_cases_hold_what_they_are_for():
    depth = lambda name: [TM.depth_of(t) for t in TM.case(name)[0].trees]
    assert sorted(depth("depth_0_31")) == list(range(32)) and set(depth("depth_equal")) == {4}
    assert sorted(depth("depth_extremes"))[-3:] == [1, 39, 39] and 0 in depth("depth_extremes")
    assert [depth("deep_at_%d" % p).index(39) for p in range(32)] == list(range(32))
    for nt in TM.COUNTS:
        d = depth("count_%d" % nt)
        assert len(d) == nt and (nt < 7 or len(set(d)) >= 4)
    # documents leave a chain at every level: the deepest leaf of the deep tree is reached, and so are most of the others
    c, _ = TM.case("deep_at_0")
    t = c.trees[0]
    nd = np.zeros(len(c.rows), np.int64)
    for _ in range(39):
        f = t["feature"][nd]
        v = c.rows[np.arange(len(nd)), np.maximum(f, 0)]
        nd = np.where(f == -1, nd, np.where(v <= t["threshold"][nd], t["left"][nd], t["right"][nd]))
    assert np.all(t["feature"][nd] == -1) and len(np.unique(nd)) >= 30 and 77 in nd      # (node 77: the leaf below 39 left turns)
    c, want = TM.case("accum_specials")
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    assert TM.max_tiled_cols(3) == TM.case("lds_in")[0].rows.shape[1] == TM.case("lds_out")[0].rows.shape[1] - 1
    assert TM.tiled_lds_bytes(TM.max_tiled_cols(3), 3) <= TM.LDS_BUDGET < TM.tiled_lds_bytes(TM.max_tiled_cols(3) + 1, 3)


@pytest.mark.parametrize("fid", ["-5", "-2147483649", "4294967297", "2147483648"])
def test_bad_feature_ids_are_refused_before_any_device_is_looked_at(fid):
    """the text is parsed first, so this needs no GPU (tests/test_gpu_model_eval.py repeats it where a model can also be created)"""
    from ranklib_amd import _native as N
    text = TM.model_text([TM.flatten(TM.S(7, 0.5, TM.L(1.0), TM.L(2.0)))], [1.0]).replace("<feature>7 ", "<feature>%s " % fid)
    assert "<feature>%s </feature>" % fid in text
    with pytest.raises(N.RankLibError) as e:
        N.Model(text)
    assert "Error in Emsemble(xmlRepresentation): bad feature id '%s'" % fid in str(e.value)
