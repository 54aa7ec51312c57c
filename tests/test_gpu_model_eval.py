"""Tree-ensemble scoring (rl_model_*: k_model_eval_tiled and k_model_eval) on hand-built models: `Model.predict_rows` / `predict_device`
against `tree_models.eval_ensemble_np`, bit for bit outside NaN results and NaN where the reference is NaN.  tests/tree_models.py builds
the models and rows (CASES) and says what each is for; tests/test_tree_models_cpu.py holds its reference to the oracle's without a GPU.

Unless a case says otherwise it runs twice from the same text: the default build of the model, which must report MODEL_PATH_TILED, and
with RLHIP_EVAL_GENERIC set before the model is created, which must report MODEL_PATH_GENERIC.  The knobs are read inside
rl_model_from_text, so the environment is set before N.Model(...)."""
import functools

import numpy as np
import pytest

import tree_models as TM
from ranklib_amd import _native as N

pytestmark = pytest.mark.gpu

KNOBS = ("RLHIP_EVAL_GENERIC", "RLHIP_EVAL_DEAL", "RLHIP_EVAL_PHASED")
BOTH = pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
WALKS = pytest.mark.parametrize("deal,phased", [(1, 1), (0, 1), (1, 0), (0, 0)], ids=["dealt-phased", "nodeal", "nophases", "nodeal-nophases"])
PATH_NAME = {N.MODEL_PATH_NONE: "none", N.MODEL_PATH_TILED: "tiled", N.MODEL_PATH_GENERIC: "generic"}


@functools.lru_cache(maxsize=None)
def _text(name):
    c, _ = TM.case(name)
    return TM.model_text(c.trees, c.weights)


def _model(monkeypatch, text, generic=False, deal=1, phased=1):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if generic:
        monkeypatch.setenv("RLHIP_EVAL_GENERIC", "1")
    if not deal:
        monkeypatch.setenv("RLHIP_EVAL_DEAL", "0")
    if not phased:
        monkeypatch.setenv("RLHIP_EVAL_PHASED", "0")
    m = N.Model(text)
    assert m.path() == N.MODEL_PATH_NONE
    return m


def _expect(m, rows, want, path, what):
    got = m.predict_rows(rows)
    assert PATH_NAME[m.path()] == PATH_NAME[path], what
    diff = TM.same_scores(got, want)
    assert diff is None, "%s (%s kernel): %s" % (what, PATH_NAME[path], diff)


def _run(monkeypatch, name, generic=False, deal=1, phased=1, n=None):
    c, want = TM.case(name)
    m = _model(monkeypatch, _text(name), generic, deal, phased)
    assert m.num_trees() == len(c.trees)
    path = N.MODEL_PATH_TILED if c.tiled and not generic else N.MODEL_PATH_GENERIC
    rows = c.rows if n is None else np.ascontiguousarray(c.rows[:n])
    _expect(m, rows, want if n is None else want[:n], path, name if n is None else "%s, %d documents" % (name, n))
    m.close()


# ---- tree count against the tile of 32 trees and the walkers' 8 ---------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("nt", TM.COUNTS)
def test_tree_counts_round_the_tile_and_the_walkers(monkeypatch, nt, generic):
    _run(monkeypatch, "count_%d" % nt, generic)


@pytest.mark.parametrize("nt", [33, 36, 38, 39, 41, 57])
@WALKS
def test_partial_last_tiles_under_every_walk(monkeypatch, nt, deal, phased):
    _run(monkeypatch, "count_%d" % nt, False, deal, phased)


# ---- depth mixes inside one tile ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth_extremes", "depth_0_31", "depth_equal"])
@WALKS
def test_depth_mixes_inside_one_tile(monkeypatch, name, deal, phased):
    _run(monkeypatch, name, False, deal, phased)


@pytest.mark.parametrize("name", ["depth_extremes", "depth_0_31", "depth_equal"])
def test_depth_mixes_generic(monkeypatch, name):
    _run(monkeypatch, name, True)


@WALKS
def test_the_deep_tree_at_every_place_of_the_tile(monkeypatch, deal, phased):
    for pos in range(TM.TILE):
        _run(monkeypatch, "deep_at_%d" % pos, False, deal, phased)


def test_the_deep_tree_at_every_place_generic(monkeypatch):
    for pos in range(TM.TILE):
        _run(monkeypatch, "deep_at_%d" % pos, True)


# ---- accumulation order, weights, special outputs -----------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("name", ["accum_order", "accum_specials"])
def test_accumulation_in_tree_order(monkeypatch, name, generic):
    _run(monkeypatch, name, generic)


@pytest.mark.parametrize("name", ["accum_order", "accum_specials"])
@WALKS
def test_accumulation_under_every_walk(monkeypatch, name, deal, phased):
    _run(monkeypatch, name, False, deal, phased)


def test_a_nan_leaf_output_takes_the_generic_kernel(monkeypatch):
    _run(monkeypatch, "nan_leaf")            # tiled=False in the case: the DEFAULT build must report MODEL_PATH_GENERIC
    assert not TM.case("nan_leaf")[0].tiled


# ---- values at the comparison -------------------------------------------------------------------------------------------------------
@BOTH
def test_thresholds_and_row_values_at_the_comparison(monkeypatch, generic):
    _run(monkeypatch, "thresholds", generic)


# ---- column 0 and row width ---------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("name", ["col0_garbage", "width_20", "width_13", "width_12", "width_5", "width_2", "width_1", "feature_0"])
def test_column_0_and_row_width(monkeypatch, name, generic):
    _run(monkeypatch, name, generic)
    if name == "feature_0":
        assert not TM.case(name)[0].tiled and 0 in {int(f) for t in TM.case(name)[0].trees for f in t["feature"]}


def test_a_split_on_feature_minus_one_is_a_leaf(monkeypatch):
    """Split.eval (:116) returns at a node whose feature is -1 whatever hangs below it: such a node scores its own output, 0"""
    text = ('<ensemble>\n<tree id="1" weight="1.0">\n<split>\n<feature>-1 </feature>\n<threshold> 0.5 </threshold>\n<split pos="left">\n<output>5.0 </output>\n'
            '</split>\n<split pos="right">\n<output>7.0 </output>\n</split>\n</split>\n</tree>\n<tree id="2" weight="2.0">\n<split>\n<feature>1 </feature>\n'
            '<threshold> 0.5 </threshold>\n<split pos="left">\n<output>1.5 </output>\n</split>\n<split pos="right">\n<output>-1.0 </output>\n</split>\n</split>\n'
            '</tree>\n</ensemble>\n')
    rows = np.array([[0, 0.5], [0, 0.75], [0, np.nan]], np.float32)
    for generic in (False, True):
        m = _model(monkeypatch, text, generic)
        _expect(m, rows, np.array([3.0, -2.0, -2.0], np.float32), N.MODEL_PATH_GENERIC if generic else N.MODEL_PATH_TILED, "feature -1")
        m.close()


# ---- the boundaries of kernel selection ---------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("name", ["nodes_79", "nodes_81", "feat_254", "feat_255", "lds_in", "lds_out"])
def test_selection_boundaries(monkeypatch, name, generic):
    """79 nodes a tree: 32 * 79 packed nodes are what a block prefetches per tile, 81 are more; feature id 254: (254 + 1) * 256 is the last
    16-bit column offset; stumps on rows of max_tiled_cols(3) columns: the last tile that fits 160 KiB of LDS.  The case says which kernel
    the default build takes (tiled=), _run asserts it through path()."""
    c, _ = TM.case(name)
    assert c.tiled == (name in ("nodes_79", "feat_254", "lds_in"))
    _run(monkeypatch, name, generic)


def test_the_lds_boundary_is_the_formula_s():
    cols = TM.case("lds_in")[0].rows.shape[1]
    maxn = max(len(t["feature"]) for t in TM.case("lds_in")[0].trees)
    assert maxn == 3 and cols == TM.max_tiled_cols(maxn)
    assert TM.tiled_lds_bytes(cols, maxn) <= 160 * 1024 < TM.tiled_lds_bytes(cols + 1, maxn)


def test_one_handle_alternating_between_the_kernels(monkeypatch):
    """the row width decides per call: a tiled width, a generic one, the tiled one again, in both orders on fresh handles"""
    (cin, win), (cout, wout) = TM.case("lds_in"), TM.case("lds_out")
    assert _text("lds_in") == _text("lds_out")
    for order in ("in out in", "out in out in"):
        m = _model(monkeypatch, _text("lds_in"))
        for which in order.split():
            c, want, path = (cin, win, N.MODEL_PATH_TILED) if which == "in" else (cout, wout, N.MODEL_PATH_GENERIC)
            _expect(m, c.rows, want, path, "order %r, %s" % (order, which))
        m.close()


# ---- document counts ----------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_document_counts(monkeypatch, n, generic):
    _run(monkeypatch, "docs", generic, n=n)


@BOTH
def test_more_documents_than_either_grid(monkeypatch, generic):
    """65536 * 64 + 65 rows of two columns (33 MB): the tiled kernel's 65 536 blocks and the generic one's 8192 * 256 threads both go
    round again, and the last tile is partial"""
    assert len(TM.case("grid_stride")[0].rows) == 65536 * 64 + 65
    _run(monkeypatch, "grid_stride", generic)


# ---- loader errors: load only, never scored -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", ["-5", "-2147483649", "4294967297", "-2", "2147483648", "99999999999999999999"])
def test_bad_feature_ids_are_refused(fid):
    """below -1 the Java would index before the row when scoring (ArrayIndexOutOfBoundsException); what does not fit an int is a
    NumberFormatException of Integer.parseInt.  Neither may load."""
    c, _ = TM.case("count_7")
    text = _text("count_7")
    old = "<feature>%d </feature>" % next(int(f) for t in c.trees for f in t["feature"] if f != -1)
    assert old in text
    with pytest.raises(N.RankLibError) as e:
        N.Model(text.replace(old, "<feature>%s </feature>" % fid, 1))
    assert "Error in Emsemble(xmlRepresentation): bad feature id '%s'" % fid in str(e.value)


def test_the_largest_feature_id_still_loads(monkeypatch):
    """Integer.MAX_VALUE is an int: the model loads, takes the generic kernel, and the column no row has reads 0"""
    trees = [TM.flatten(TM.S(2147483647, -0.5, TM.L(1.0), TM.L(2.0))), TM.flatten(TM.S(1, 0.5, TM.L(0.25), TM.L(-3.0)))]
    rows = np.array([[0, 0.5], [0, 0.75], [0, np.nan]], np.float32)
    m = _model(monkeypatch, TM.model_text(trees, [1.0, 1.0]))
    assert list(m.features()) == [1, 2147483647]
    _expect(m, rows, TM.eval_ensemble_np(trees, [1.0, 1.0], rows), N.MODEL_PATH_GENERIC, "feature id 2^31 - 1")
    m.close()


# ---- predict_device (last: it hands the library a stream that torch made) -----------------------------------------------------------
def _hip_runtimes():
    with open("/proc/self/maps") as f:
        return {ln.split()[-1] for ln in f if "libamdhip64" in ln}


@BOTH
def test_predict_device_on_a_stream_of_its_own(monkeypatch, generic):
    """a non-default stream; rows that start one 13-column row (52 bytes) into a larger tensor, so the base is not 16-byte aligned; fewer
    documents than the tensor holds -- the output entries behind them stay as they were"""
    import torch
    assert len(_hip_runtimes()) == 1, "torch's stream is a handle of another HIP runtime than the library's: %r" % _hip_runtimes()
    c, want = TM.case("device")
    n_all, width = c.rows.shape
    n = n_all - 1 - 20                       # skip the first row, leave the last 20 alone
    m = _model(monkeypatch, _text("device"), generic)
    dX = torch.from_numpy(np.array(c.rows)).cuda()
    dO = torch.full((n_all,), -7.0, dtype=torch.float32, device="cuda")
    assert (dX.data_ptr() + width * 4) % 16 != 0
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        m.predict_device(dX.data_ptr() + width * 4, n, width, dO.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = dO.cpu().numpy()
    assert m.path() == (N.MODEL_PATH_GENERIC if generic else N.MODEL_PATH_TILED)
    diff = TM.same_scores(got[:n], want[1:1 + n])
    assert diff is None, diff
    assert (got[n:] == -7.0).all()
    m.close()
