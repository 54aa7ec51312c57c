"""Interventional TreeSHAP on the GPU (rl_model_predict_shap_background: k_interv_masks, k_interv_bias, k_model_interv, rl_interv.inc;
DESIGN.md 34) against the f64 run of tests/interv_restatement.py.  Everything is compared as bit patterns; no tolerance anywhere but
local accuracy (where the reference value is NaN the kernel's is NaN: contrib_restatement.same_f64)."""
import functools

import numpy as np
import pytest

import contrib_restatement as CR
import interv_restatement as IV
import shap_restatement as SR
import test_gpu_shap as GS
import tree_models as TM
from ranklib_amd import _native as N
from ranklib_amd import contribs as CL
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import LambdaMART, MART, RankerFactory, java_double_str, java_float_str
from test_gpu_shap import _restore_statics, u64      # noqa: F401  (the fixture is autouse)

pytestmark = pytest.mark.gpu

MODELS = ["count_37", "nodes_81", "single_leaves", "nan_leaf", "accum_specials", "chain_left", "and_tree", "distinct_30"]
BG_COUNTS = (1, 2, 65, 300)                      # one mask, a padded row of the buffer, more than a wavefront, more than a block of lanes
WHO = "rl_model_predict_shap_background: "


@functools.lru_cache(maxsize=None)
def background():
    """narrower than the documents: the chains' last features are beyond bg_stride"""
    rows = CR.grid_rows(np.random.default_rng(43), max(BG_COUNTS), 29)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def reference(name, n_bg):
    """what the chains of GS.doc_rows() add against the background's first n_bg rows: made once, whatever the columns"""
    trees, w, _ = GS.model(name)
    mag = []
    return IV.terms(trees, w, GS.doc_rows(), background()[:n_bg], abs_leaf=mag), sum(mag)


@functools.lru_cache(maxsize=None)
def wanted(name, n_bg, what):
    """(the columns asked for, the ids of the slots, the restatement's values of all of GS.doc_rows(), sum |W out|)"""
    trees = GS.model(name)[0]
    cols = GS.column_choices(trees)[what]
    ids = CR.model_features(trees) if cols is None else cols
    terms, mag = reference(name, n_bg)
    return cols, ids, IV.accumulate(terms, len(GS.doc_rows()), ids), mag


# ---- 1. the kernel is the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GS.ROW_COUNTS)
@pytest.mark.parametrize("n_bg", BG_COUNTS)
@pytest.mark.parametrize("name, what", [(name, what) for name in MODELS for what in GS.column_choices(GS.MODELS[name]()[0])])
def test_interv_equals_the_restatement(name, what, n_bg, n):
    m = GS.model(name)[2]
    cols, ids, want, mag = wanted(name, n_bg, what)
    got, gids = m.predict_shap_background(GS.doc_rows()[:n], background()[:n_bg], cols)
    assert m.path() == N.MODEL_PATH_INTERV and N.interv_passes() == 1
    assert gids == ids and got.shape == (n, len(ids) + 2) and got.dtype == np.float64
    assert CR.same_f64(got, want[:n]) is None, CR.same_f64(got, want[:n])
    assert len(set(u64(got[:, -1]).tolist())) == 1                             # one bias for every row
    if what == "unused":
        assert not u64(want[:, 0]).any()                                       # a feature the model never splits on: +0.0
    if what == "none":
        assert not u64(want[:, len(ids)]).any()                                # every feature has its slot: rest is +0.0, the bits
        leaf = m.leaf_sums(GS.doc_rows()[:n])                                  # local accuracy, within the bound of the CPU test's (c)
        total = np.zeros(n)
        with np.errstate(all="ignore"):
            for c in range(got.shape[1]):
                total = total + got[:, c]
            ok = np.isfinite(leaf) & np.isfinite(total)
            gap = np.abs(total - leaf)[ok]
            print("the slots' sum is %.3f x 2^-52 x sum |W out| from the leaf sum at most" % (gap.max(initial=0.0) / mag / IV.U))
            # (a NaN or infinite leaf is met by every row, so those two models may leave no finite row to measure)
            assert (gap <= IV.BOUND * mag).all() and (ok.all() or name in ("nan_leaf", "accum_specials"))


# ---- 2. column passes, 3. tree chunks and row chunks, a handle without covers ---------------------------------------------------------------
def test_more_slots_than_the_lds_holds_take_several_column_passes():
    trees, w, rows, _, m = GS.wide()
    bg = CR.grid_rows(np.random.default_rng(44), 5, 401)
    terms = IV.terms(trees, w, rows, bg)
    got, ids = m.predict_shap_background(rows, bg)
    assert N.interv_passes() == 2 and ids == list(range(1, 401))               # 402 slots: blocks of 64 hold 296 beside s[2][64]
    assert CR.same_f64(got, IV.accumulate(terms, len(rows), ids)) is None
    for pick in (sorted(np.random.default_rng(3).choice(400, 20, replace=False) + 1), list(range(400, 262, -1))):      # blocks of 256, of 128
        one, _ = m.predict_shap_background(rows, bg, pick)
        assert N.interv_passes() == 1
        assert np.array_equal(u64(one[:, :len(pick)]), u64(got[:, [p - 1 for p in pick]])) and np.array_equal(u64(one[:, -1]), u64(got[:, -1]))
        assert CR.same_f64(one, IV.accumulate(terms, len(rows), pick)) is None


def test_tree_chunks_and_row_chunks_change_no_bit_and_no_cover_is_needed():
    trees, w, _ = GS.model("count_37")
    m = N.Model(TM.model_text(trees, w))                                   # a handle that never saw rl_model_cover
    rows, feats = GS.doc_rows(), CR.model_features(trees)
    bg = background()[:65]
    whole, _ = m.predict_shap_background(rows, bg)
    assert m.path() == N.MODEL_PATH_INTERV and min(N.interv_times()) >= 0.0
    assert CR.same_f64(whole, IV.accumulate(reference("count_37", 65)[0], len(rows), feats)) is None
    # a tree's masks and leaf indices are 4 (leaves x 68 + 65) bytes: no chunk holds more than a third of them all, so there are three
    # chunks at least, and the rows go in several chunks beside them; then 100 + 100 + 57 rows through one tree chunk; then a tree and
    # a row a chunk
    third = sum(4 * (len(IV.elements(t)) * 68 + 65) for t in trees) // 3
    for n, scratch in ((len(rows), third), (len(rows), (GS.WIDTH * 4 + 8 * (len(feats) + 2)) * 100), (3, 1)):
        cut, _ = m.predict_shap_background(rows[:n], bg, scratch_bytes=scratch)
        assert np.array_equal(u64(cut), u64(whole[:n])), scratch
    with pytest.raises(N.RankLibError, match="rl_model_predict_shap: no rl_model_cover call has been made on this model"):
        m.predict_shap(rows)


# ---- 4. the path limit and the refusals ----------------------------------------------------------------------------------------------------
def test_a_path_of_32_distinct_features_is_taken_and_the_refusals_by_message():
    rows, bg = GS.doc_rows()[:65], background()[:65]
    trees, w = SR.distinct_chain(SR.P_LIMIT, seed=13)
    m = N.Model(TM.model_text(trees, w))
    got, ids = m.predict_shap_background(rows, bg)
    assert len(ids) == 32 and CR.same_f64(got, IV.interv(trees, w, rows, bg, ids)) is None
    trees, w = SR.distinct_chain(SR.P_LIMIT + 1, seed=14)
    far = N.Model(TM.model_text(trees, w))
    lib, out = N.lib(), np.zeros((65, 35))
    X, G, O = rows.ctypes.data, np.ascontiguousarray(bg).ctypes.data, out.ctypes.data

    def err(rc_want, rc, text):
        assert rc == rc_want and lib.rl_last_error().decode() == WHO + text, (rc, lib.rl_last_error().decode())
    err(-4, lib.rl_model_predict_shap_background(far.h, X, 65, GS.WIDTH, G, 65, 29, None, 0, 0, O),
        "the path to leaf 0 (node 33) of tree 0 holds 33 distinct features, more than 32")
    assert far.path() == N.MODEL_PATH_NONE and not out.any()                 # refused before any launch
    for args, rc, text in (((m.h, X, 65, GS.WIDTH, G, 0, 29, None, 0, 0, O), -1, "n_background must be >= 1"),
                           ((m.h, X, 65, GS.WIDTH, G, 16385, 29, None, 0, 0, O), -4, "more than 16384 background rows")):
        err(rc, lib.rl_model_predict_shap_background(*args), text)
    assert not out.any() and m.predict_shap_background(rows[:0], bg)[0].shape == (0, 34)      # no rows: legal, nothing to do


# ---- 5. against the public path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head, cls", [("## LambdaMART", LambdaMART), ("## MART", MART)])
def test_the_rankers_and_the_command_line(head, cls, tmp_path):
    trees, w, _ = GS.model("count_37")
    rng = np.random.default_rng(17)
    text = TM.model_text(trees, w).replace("## LambdaMART", head, 1)
    files = {}
    for nm, lens in (("bg", [40, 3, 77, 30]), ("test", [5, 1, 64, 20])):
        qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        rows = rng.choice(TM.GRID, (int(qoff[-1]), 13)).astype(np.float32)
        rows[:, 0] = 0.0
        files[nm] = (str(tmp_path / (nm + ".txt")), rows, qoff)
        with open(files[nm][0], "w") as f:
            f.write(GS.letor_text(rows, rng.integers(0, 5, len(rows)), qoff))
    mpath, fpath, out, summ = (str(tmp_path / n) for n in ("model.txt", "features.txt", "contribs.tsv", "summary.tsv"))
    open(mpath, "w").write(text)
    open(fpath, "w").write("7\n2\n30\n")
    ranker = RankerFactory().loadRankerFromString(text)
    assert type(ranker) is cls
    direct, test = N.Model(text), files["test"][1]
    read = FeatureManager.readInput
    for feats, nbg, seed in ((None, 100, 1), ([7, 2, 30], 60, 5), (None, 150, 1)):
        ref = files["bg"][1][np.sort(np.random.default_rng(seed).choice(150, nbg, replace=False))] if nbg < 150 else files["bg"][1]
        want, wids = direct.predict_shap_background(test, ref, feats)
        kw = dict(nBackground=nbg, backgroundSeed=seed) if nbg != 100 else {}
        got, ids = ranker.contributions(read(files["test"][0]), read(files["bg"][0]), features=feats, interventional=True, **kw)
        assert ids == wids and np.array_equal(u64(got), u64(want))
    with pytest.raises(N.RankLibError, match="need a background with at least one document"):
        ranker.contributions(read(files["test"][0]), None, interventional=True)
    want = direct.predict_shap_background(test, files["bg"][1][np.sort(np.random.default_rng(5).choice(150, 60, replace=False))], [7, 2, 30])[0]
    assert CL.main(["-load", mpath, "-background", files["bg"][0], "-test", files["test"][0], "-feature", fpath, "-interventional", "-nbg", "60",
                    "-bgseed", "5", "-out", out, "-summary", summ]) == 0
    scores, qoff, lines = direct.predict_rows(test), files["test"][2], open(out).read().splitlines()
    assert len(lines) == len(scores)
    for d, (q, k) in enumerate((q, k) for q in range(len(qoff) - 1) for k in range(qoff[q + 1] - qoff[q])):
        assert lines[d].split("\t") == ["q%d" % q, str(k), java_float_str(scores[d])] + [
            "%s:%s" % (nm, java_double_str(float(v))) for nm, v in zip(["7", "2", "30", "rest", "bias"], want[d])]
    assert open(summ).read().splitlines() == CL.summary_lines([7, 2, 30], want)
