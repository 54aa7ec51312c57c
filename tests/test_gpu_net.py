"""RankNet / LambdaRank / ListNet models on the GPU: rl_net_predict against the literal restatement of the Java objects
(tests/net_restatement.py), bit for bit (the scores are compared as uint64), over both kernel variants; the device-pointer entry, two
handles side by side, the three classes, and the command line on a loaded model."""
import functools

import numpy as np
import pytest

import net_restatement as NR
from ranklib_amd import _native as N
from ranklib_amd import evaluator, normalizer
from ranklib_amd.features import FeatureManager
from ranklib_amd.learning import DataPoint, RankerFactory, RankList, stable_desc_order, java_double_str, java_round
from ranklib_amd.metric import MetricScorerFactory

pytestmark = pytest.mark.gpu

BLOCK = 256                       # documents of a block of k_net_forward; its tile takes 32 inputs of them at a time
DOCS = (1, 63, 64, 65, BLOCK + 1, 2 * BLOCK + 1)
PATHS = set()                     # kernel variants the cases below took (checked last)


def _u64(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def _same(got, want, what=""):
    bad = np.nonzero(_u64(got) != _u64(want))[0]
    assert bad.size == 0, "%s: %d of %d scores differ, first at %d: %r != %r" % (what, bad.size, len(want), bad[0], got[bad[0]], want[bad[0]])


def _rows(rng, n, width):
    X = rng.standard_normal((n, width)).astype(np.float32)
    X[rng.random(X.shape) < 0.15] = 0.0
    X[:, 0] = 0.0                 # column 0 is no feature
    return X


@functools.lru_cache(maxsize=None)
def _case(F, hidden, n):
    """(restatement, rows [n][F + 1], expected scores): computed once per network, shared and never written to"""
    rng = np.random.default_rng(1000 * F + 10 * len(hidden) + sum(hidden))
    net = NR.random_net("RankNet", list(range(1, F + 1)), list(hidden), rng, scale=1.5 / np.sqrt(F))
    X = _rows(rng, n, F + 1)
    want = net.eval_rows(X)
    want.setflags(write=False)
    X.setflags(write=False)
    return net, X, want


def _model(net):
    return N.NetModel(net.features, net.hidden(), net.abi_weights())


def _predict(m, X):
    out = m.predict_rows(X)
    PATHS.add(m.path())
    return out


def test_the_vectorised_restatement_is_the_literal_one():
    net, X, want = _case(2, (3, 2), 2 * BLOCK + 1)
    _same(net.eval_rows(X[:40], literal=True), want[:40])


@pytest.mark.parametrize("hidden", [(), (1,), (10,), (3, 2), (33,)], ids=str)
@pytest.mark.parametrize("F", [1, 2, 136])
def test_scores_bit_for_bit(F, hidden):
    net, X, want = _case(F, hidden, 2 * BLOCK + 1)
    m = _model(net)
    for n in DOCS:                # every count is its own launch: a lone document, a wavefront +- 1, a block + 1, two tiles + 1
        _same(_predict(m, X[:n]), want[:n], "F=%d hidden=%s n=%d" % (F, hidden, n))
    assert m.path() == (N.NET_PATH_GLOBAL if hidden == (33,) else N.NET_PATH_LDS)      # 33 > the 32 register-resident chains of layer 1
    m.close()


@pytest.mark.parametrize("F,hidden", [(700, (50,)), (700, (12,)), (40, (30, 31, 5))], ids=str)
def test_networks_past_the_lds_budget(F, hidden):
    # 700 x 50 is too wide for the registers and too large for LDS; 701 x 12 doubles alone (as 12 chains) are 67 KB > the 64 KB budget;
    # two scratch columns of 31 hidden outputs for 256 lanes are 124 KB
    net, X, want = _case(F, hidden, 130)
    m = _model(net)
    _same(_predict(m, X), want, "F=%d hidden=%s" % (F, hidden))
    assert m.path() == N.NET_PATH_GLOBAL
    m.close()


def test_three_hidden_layers_in_lds():
    net, X, want = _case(20, (7, 5, 3), BLOCK + 1)         # both scratch buffers of k_net_forward in turn
    m = _model(net)
    _same(_predict(m, X), want)
    assert m.path() == N.NET_PATH_LDS
    m.close()


@pytest.mark.parametrize("hidden", [(), (4,)], ids=str)
def test_row_stride_and_feature_list(hidden):
    rng = np.random.default_rng(77)
    features = [9, 2, 40, 5, 5, 33, 12]                    # out of order, with gaps, one id twice
    net = NR.random_net("RankNet", features, list(hidden), rng, scale=0.5)
    m = _model(net)
    for width in (41, 64, 34, 10, 3, 1):                   # as needed, wider, and narrower: ids >= row_stride read 0
        X = _rows(rng, 70, width)
        if width > 1:
            X[:, 1:] += 0.25                               # no cell the test depends on is 0 by accident
        want = net.eval_rows(X)
        _same(_predict(m, X), want, "row_stride %d" % width)
        if width < 41:                                     # the ids that fell off DO change the score
            wide = np.zeros((70, 41), np.float32)
            wide[:, :width] = X
            wide[:, width:] = 1.0
            assert (_u64(net.eval_rows(wide)) != _u64(want)).any()
    m.close()


# wsum of the output neuron, exactly: one feature x (a float), its weight w, bias weight 0.0: wsum = x * w + 1.0 * 0.0
EXTREME = [(1.0, 0.0), (1.0, -0.0), (0.5, 1.0), (36.0, 1.0), (700.5, 1.0), (1.0, 709.9), (1.0, 745.2), (800.0, 1.0), (2.0 ** -30, 1.0),
           (1.0, 708.3), (1.0, 744.4), (0.25, 2.0 ** -1070)]


@pytest.mark.parametrize("hidden", [(), (1,)], ids=str)
def test_sums_at_the_ends_of_exp(hidden):
    groups = {}                                            # one network per weight (0.0 and -0.0 are two), its documents +-x
    for x, w in EXTREME:
        groups.setdefault(repr(w), (w, []))[1].extend([x, -x])
    for w, docs in groups.values():
        X = np.zeros((len(docs), 2), np.float32)
        X[:, 1] = docs
        net = NR.Net().build([1], list(hidden))
        first = net.layers[1][0]
        first.inLinks[0].weight, first.inLinks[1].weight = w, 0.0
        if hidden:
            net.outputLayer[0].inLinks[0].weight, net.outputLayer[0].inLinks[1].weight = 1400.0, -700.0      # the output's sum spans +-700 too
        want = net.eval_rows(X)
        for i, x in enumerate(docs):                       # the restatement's sum is the product, exactly
            net.eval_rows(X[i:i + 1], literal=True)
            assert first.wsum == float(np.float32(x)) * w
        m = _model(net)
        _same(_predict(m, X), want, "w=%r" % w)
        m.close()
        if not hidden and w == 1.0:
            got = dict(zip(docs, want))
            assert got[0.5] == 1.0 / (1.0 + NR.jexp(-0.5)) and got[800.0] == 1.0 and got[-800.0] == 0.0 and got[-700.5] > 0.0
        if not hidden and w == 745.2:
            assert want.tolist() == [1.0, 0.0]             # exp(-745.2) underflows to 0, exp(745.2) is Infinity
        if not hidden and w == 744.4:
            assert want[0] == 1.0 and 0.0 < NR.jexp(-744.4) < 2.3e-308 and want[1] == 0.0      # a subnormal exp


def test_the_class_of_model_does_not_change_the_scores(tmp_path):
    net, X, want = _case(2, (3, 2), 2 * BLOCK + 1)
    body = net.model().split("\n", 6)[6]                   # the feature line, the layer sizes and the weight lines
    assert body.startswith("1 2\n2\n3\n2\n0 0 ")
    rl = RankList([DataPoint.from_parsed(0.0, "q", "", X[i]) for i in range(70)])
    for kind in ("RankNet", "LambdaRank", "ListNet"):
        r = RankerFactory().loadRankerFromString("## %s\n%s" % (kind, body))
        _same(r.evalList(rl), want[:70], kind)
        assert _u64([r.eval(rl.get(3))])[0] == _u64(want[3:4])[0]
        PATHS.add(r._model().path())


def test_predict_device_equals_predict_rows():
    import torch
    for F, hidden in ((136, (10,)), (136, (33,))):
        net, X, want = _case(F, hidden, 2 * BLOCK + 1)
        m = _model(net)
        dX = torch.from_numpy(np.array(X)).cuda()
        dO = torch.full((X.shape[0],), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        m.predict_device(dX.data_ptr(), X.shape[0] - 3, X.shape[1], dO.data_ptr())
        torch.cuda.synchronize()
        got = dO.cpu().numpy()
        _same(got[:-3], want[:-3], "predict_device")
        assert (got[-3:] == -1.0).all()                    # nothing is written past n_docs
        _same(m.predict_rows(X), want)
        m.close()


def test_two_handles_do_not_disturb_each_other():
    a, Xa, wa = _case(136, (10,), 2 * BLOCK + 1)
    b, Xb, wb = _case(136, (33,), 2 * BLOCK + 1)
    c, Xc, wc = _case(2, (3, 2), 2 * BLOCK + 1)
    ma, mb, mc = _model(a), _model(b), _model(c)
    for _ in range(2):
        _same(ma.predict_rows(Xa), wa)
        _same(mb.predict_rows(Xb), wb)
        _same(mc.predict_rows(Xc), wc)
    mb.close()
    _same(ma.predict_rows(Xa[:65]), wa[:65])
    assert (ma.path(), mc.path()) == (N.NET_PATH_LDS, N.NET_PATH_LDS)


def _letor(path, rng, lists=(5, 1, 9), F=3):
    """a tiny LETOR file; returns per list (qid, labels, rows [n][F + 1], document names)"""
    out, text = [], []
    for q, n in enumerate(lists):
        X = np.zeros((n, F + 1), np.float32)
        X[:, 1:] = rng.integers(-8, 9, (n, F)) / np.float32(4.0)
        lab = rng.integers(0, 3, n)
        names = ["d%d_%d" % (q, i) for i in range(n)]
        for i in range(n):
            text.append("%d qid:q%d %s # %s" % (lab[i], q, " ".join("%d:%s" % (f, X[i, f]) for f in range(1, F + 1)), names[i]))
        out.append(("q%d" % q, lab.astype(np.float32), X, names))
    path.write_text("\n".join(text) + "\n")
    return out


@pytest.mark.parametrize("kind", ["RankNet", "LambdaRank", "ListNet"])
def test_command_line_on_a_loaded_model(tmp_path, kind):
    rng = np.random.default_rng(5)
    lists = _letor(tmp_path / "t.txt", rng)
    net = NR.random_net(kind, [3, 1, 2], [] if kind == "ListNet" else [4], rng)
    (tmp_path / "m.txt").write_text(net.model())
    model, data = str(tmp_path / "m.txt"), str(tmp_path / "t.txt")
    scores = [net.eval_rows(X) for _, _, X, _ in lists]
    # -rank -score: qid \t index \t Double.toString(score)
    assert evaluator.main(["-load", model, "-rank", data, "-score", str(tmp_path / "s.txt"), "-feature", "unused.txt"]) == 0
    want = "".join("%s\t%d\t%s\n" % (qid, j, java_double_str(float(v))) for (qid, _, _, _), sc in zip(lists, scores) for j, v in enumerate(sc))
    assert (tmp_path / "s.txt").read_text() == want
    # -rank -indri: the list in stable descending order of the scores
    assert evaluator.main(["-load", model, "-rank", data, "-indri", str(tmp_path / "i.txt")]) == 0
    want = ""
    for (qid, _, _, names), sc in zip(lists, scores):
        for i, j in enumerate(stable_desc_order(sc)):
            want += "%s Q0 %s %d %s indri\n" % (qid, names[int(j)], i + 1, java_double_str(java_round(float(sc[int(j)]), 5)))
    assert (tmp_path / "i.txt").read_text() == want
    # -test with -idv: the host metric of the restatement's ranking, per list and averaged
    for metric in ("NDCG@3", "MAP", "ERR@10"):
        assert evaluator.main(["-load", model, "-test", data, "-metric2T", metric, "-idv", str(tmp_path / "p.txt")]) == 0
        scorer = MetricScorerFactory().createScorer(metric)
        per = []
        for (qid, lab, X, _), sc in zip(lists, scores):
            rl = RankList([DataPoint.from_parsed(float(lab[i]), qid, "", X[i]) for i in range(len(lab))])
            per.append(scorer.score(RankList(rl, list(stable_desc_order(sc)))))
        avg = 0.0
        for v in per:
            avg += v
        avg /= len(per)
        want = "".join("%s   %s   %s\n" % (scorer.name(), qid, java_double_str(v)) for (qid, _, _, _), v in zip(lists, per))
        assert (tmp_path / "p.txt").read_text() == want + "%s   all   %s\n" % (scorer.name(), java_double_str(avg))
    # -qrel reaches the test scorer: judgments that differ from the file's labels change NDCG's ideal gains
    qrel = str(tmp_path / "q.txt")
    (tmp_path / "q.txt").write_text("".join("q%d 0 d%d_%d %d\n" % (q, q, i, 3 - int(l)) for q, (_, lab, _, _) in enumerate(lists) for i, l in enumerate(lab)))
    assert evaluator.main(["-load", model, "-test", data, "-metric2T", "NDCG@3", "-qrel", qrel, "-idv", str(tmp_path / "p2.txt")]) == 0
    evaluator.Evaluator.qrelFile = ""
    scorer = MetricScorerFactory().createScorer("NDCG@3")
    scorer.loadExternalRelevanceJudgment(qrel)
    want = ""
    for (qid, lab, X, _), sc in zip(lists, scores):
        rl = RankList([DataPoint.from_parsed(float(lab[i]), qid, "", X[i]) for i in range(len(lab))])
        want += "NDCG@3   %s   %s\n" % (qid, java_double_str(scorer.score(RankList(rl, list(stable_desc_order(sc))))))
    got = (tmp_path / "p2.txt").read_text()
    assert got.startswith(want) and got != (tmp_path / "p.txt").read_text()
    # -norm normalises the loaded model's features (getFeatures()) before scoring
    assert evaluator.main(["-load", model, "-rank", data, "-score", str(tmp_path / "s2.txt"), "-norm", "sum"]) == 0
    evaluator.Evaluator.normalize = False
    normed = FeatureManager.readInput(data)
    normalizer.SumNormalizor().normalizeAll(normed, [3, 1, 2])
    want = ""
    for rl in normed:
        rows = np.array([np.where(np.isnan(dp.fVals), np.float32(0), dp.fVals) for dp in rl.rl], np.float32)
        want += "".join("%s\t%d\t%s\n" % (rl.getID(), j, java_double_str(float(v))) for j, v in enumerate(net.eval_rows(rows)))
    assert (tmp_path / "s2.txt").read_text() == want and want != (tmp_path / "s.txt").read_text()


def test_both_kernel_variants_ran():
    assert {N.NET_PATH_LDS, N.NET_PATH_GLOBAL} <= PATHS, PATHS
