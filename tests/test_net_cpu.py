"""RankNet / LambdaRank / ListNet models without a GPU: the wiring of the restatement against tables written by hand, the loader and the
model text of ranklib_amd.learning against the restatement, every parse error, the refusals that stay, and the refusal without a device."""
import numpy as np
import pytest

import net_restatement as NR
from conftest import has_gpu
from np_restatement import jexp
from ranklib_amd import _native as N
from ranklib_amd import learning
from ranklib_amd._native import RankLibError
from ranklib_amd.learning import LambdaRank, ListNet, RankerFactory, RankerType, RankNet

KINDS = {"RankNet": RankNet, "LambdaRank": LambdaRank, "ListNet": ListNet}


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def test_wiring_without_a_hidden_layer_by_hand():
    net = NR.Net().build([7, 8], [])
    # layer 0 = inputs 0, 1 and the bias 2; layer 1 = the output neuron: inputs in order, the bias last
    assert net.in_links(1, 0) == [(0, 0), (0, 1), (0, 2)]
    assert [net.out_links(0, j) for j in range(3)] == [[(1, 0)], [(1, 0)], [(1, 0)]]
    assert net.out_links(1, 0) == []


def test_wiring_with_one_hidden_layer_by_hand():
    net = NR.Net().build([1, 2], [3])
    for j in range(3):
        assert net.in_links(1, j) == [(0, 0), (0, 1), (0, 2)]
    assert net.in_links(2, 0) == [(1, 0), (1, 1), (1, 2), (0, 2)]          # the bias neuron of layer 0 is the output's last source too
    assert net.out_links(0, 0) == [(1, 0), (1, 1), (1, 2)] and net.out_links(0, 1) == [(1, 0), (1, 1), (1, 2)]
    assert net.out_links(0, 2) == [(1, 0), (1, 1), (1, 2), (2, 0)]         # the bias: all of layer 1, then the output neuron
    assert [net.out_links(1, j) for j in range(3)] == [[(2, 0)]] * 3


def test_wiring_with_two_hidden_layers_by_hand():
    net = NR.Net().build([5], [3, 2])
    assert [net.in_links(1, j) for j in range(3)] == [[(0, 0), (0, 1)]] * 3
    assert [net.in_links(2, j) for j in range(2)] == [[(1, 0), (1, 1), (1, 2), (0, 1)]] * 2
    assert net.in_links(3, 0) == [(2, 0), (2, 1), (0, 1)]
    assert net.out_links(0, 0) == [(1, 0), (1, 1), (1, 2)]
    assert net.out_links(0, 1) == [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0)]
    assert [net.out_links(1, j) for j in range(3)] == [[(2, 0), (2, 1)]] * 3
    assert [net.out_links(2, j) for j in range(2)] == [[(3, 0)]] * 2


def test_eval_of_the_restatement_by_hand():
    # one input, no hidden layer: wsum = x * w + 1 * b
    net = NR.Net().loadFromString("## RankNet\n3\n0\n0 0 2.0\n0 1 -1.0\n")
    assert net.eval(lambda f: {3: np.float32(0.5)}[f]) == 0.5 and net.outputLayer[0].wsum == 0.0
    assert net.eval(lambda f: np.float32(1.5)) == 1.0 / (1.0 + jexp(-2.0)) and net.outputLayer[0].wsum == 2.0
    # the input is a float widened: 0.1f, not 0.1
    assert net.eval(lambda f: np.float32(0.1)) == 1.0 / (1.0 + jexp(-(float(np.float32(0.1)) * 2.0 + -1.0)))


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("features,hidden", [([1, 2], []), ([4, 2, 9], [3]), ([3], [3, 2]), ([1, 2, 3, 4, 5], [1])])
def test_loader_layout_against_the_restatement(kind, features, hidden):
    ref = NR.random_net(kind, features, hidden, np.random.default_rng(11))
    src = ref.model()
    if kind == "ListNet" and hidden:                      # ListNet.model() writes a literal 0 and no sizes: put them back to load the network
        src = src.replace("\n0\n", "\n%d\n%s" % (len(hidden), "".join("%d\n" % h for h in hidden)), 1)
    r = RankerFactory().loadRankerFromString(src)
    assert type(r) is KINDS[kind] and r.name() == kind
    assert r.getFeatures() == features and r.hidden == hidden
    # the file's outLinks layout turned into the ABI's inLinks layout
    assert _bits(np.concatenate([w.ravel() for w in r.weights])) == _bits(ref.abi_weights())
    assert r.toString() == ref.toString()
    assert r.model() == ref.model()                       # byte for byte, ListNet's literal 0 included
    assert NR.Net(kind).loadFromString(src).model() == ref.model()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_model_text_by_hand(kind):
    head = {"RankNet": "## RankNet\n## Epochs = 100\n## No. of features = 2\n## No. of hidden layers = 1\n## Layer 1: 2 neurons\n",
            "LambdaRank": "## LambdaRank\n## Epochs = 100\n## No. of features = 2\n## No. of hidden layers = 1\n## Layer 1: 2 neurons\n",
            "ListNet": "## ListNet\n## Epochs = 1500\n## No. of features = 2\n"}[kind]
    body = "0 0 0.5 1.0E-5\n0 1 -1.0 12345.678\n0 2 0.1 0.2 -0.001\n1 0 1.23456785E7\n1 1 -0.0\n"
    given = head + "7 3\n1\n2\n" + body                   # a feature list that is not 1 .. F
    r = RankerFactory().loadRankerFromString(given)
    assert r.getFeatures() == [7, 3] and r.hidden == [2]
    assert r.weights[0].tolist() == [[0.5, -1.0, 0.1], [1.0E-5, 12345.678, 0.2]] and r.weights[1][0, :2].tolist() == [12345678.5, -0.0]
    assert r.weights[1][0, 2] == -0.001
    # ListNet.model() prints the literal 0 and no layer sizes whatever the network is (ListNet.java:170)
    want = given if kind != "ListNet" else head + "7 3\n0\n" + body
    assert r.model() == want and r.toString() == body
    assert NR.Net(kind).loadFromString(given).model() == want


def test_lines_in_any_order_duplicates_and_extra_tokens():
    base = "## RankNet\n1 2\n1\n2\n"
    lines = ["0 0 1.0 2.0", "0 1 3.0 4.0", "0 2 5.0 6.0 7.0", "1 0 8.0", "1 1 9.0"]
    a = RankerFactory().loadRankerFromString(base + "\n".join(lines) + "\n")
    shuffled = [lines[3], "0 1 -3.0 -4.0", lines[2], "", "  " + lines[0] + " 99.0 98.0  ", "## a comment", lines[4], lines[1], "2 0 5.0 6.0"]
    b = RankerFactory().loadRankerFromString(base + "\r\n".join(shuffled))
    assert a.toString() == b.toString()                   # the later "0 1" line wins, tokens beyond the outLinks and the output neuron's line are ignored
    assert b.toString() == NR.Net().loadFromString(base + "\r\n".join(shuffled)).toString()


@pytest.mark.parametrize("kind,prefix", [("RankNet", "Error in RankNet::load(): "), ("LambdaRank", "Error in RankNet::load(): "),
                                         ("ListNet", "Error in ListNet::load(): ")])
def test_every_parse_error_carries_the_java_prefix(kind, prefix):
    ok = "1 2\n1\n2\n0 0 1.0 2.0\n0 1 3.0 4.0\n0 2 5.0 6.0 7.0\n1 0 8.0\n1 1 9.0\n"
    RankerFactory().loadRankerFromString("## %s\n%s" % (kind, ok))
    bad = {
        "nothing but comments": "## x\n\n",
        "no layer count": "1 2\n",
        "bad feature id": ok.replace("1 2\n", "1 two\n", 1),
        "two spaces in the feature line": ok.replace("1 2\n", "1  2\n", 1),
        "bad layer count": ok.replace("1 2\n1\n", "1 2\n1.0\n", 1),
        "negative layer count": ok.replace("1 2\n1\n", "1 2\n-1\n", 1),
        "missing layer size": "1 2\n1\n",
        "bad layer size": ok.replace("1 2\n1\n2\n", "1 2\n1\nx\n", 1),
        "empty layer": ok.replace("1 2\n1\n2\n", "1 2\n1\n0\n", 1),
        "too few weights": ok.replace("0 2 5.0 6.0 7.0", "0 2 5.0 6.0"),
        "no weight at all": ok.replace("1 1 9.0", "1 1"),
        "bad weight": ok.replace("8.0", "8,0"),
        "bad layer index": ok.replace("1 1 9.0", "x 1 9.0"),
        "layer out of range": ok.replace("1 1 9.0", "3 0 9.0"),
        "negative layer": ok.replace("1 1 9.0", "-1 0 9.0"),
        "neuron out of range": ok.replace("1 1 9.0", "1 2 9.0"),
        "neuron beyond the bias": ok.replace("0 2 5.0 6.0 7.0", "0 3 5.0 6.0 7.0"),
        "negative neuron": ok.replace("1 1 9.0", "1 -1 9.0"),
        "a neuron line is missing": ok.replace("0 1 3.0 4.0\n", ""),
        "the bias line is missing": ok.replace("0 2 5.0 6.0 7.0\n", ""),
    }
    for what, body in bad.items():
        with pytest.raises(RankLibError) as e:
            RankerFactory().loadRankerFromString("## %s\n%s" % (kind, body))
        assert str(e.value).startswith(prefix), what
        if "missing" in what and "line" in what:
            assert "neuron %d of layer 0" % (1 if what.startswith("a neuron") else 2) in str(e.value), what
        else:                                             # the Java refuses these as well (an empty layer excepted: see DESIGN.md 13)
            if what != "empty layer":
                with pytest.raises(NR.LoadError) as e2:
                    NR.Net(kind).loadFromString("## %s\n%s" % (kind, body))
                assert str(e2.value).startswith(prefix), what
    # what the Java leaves at its random weight, the restatement can name too
    assert NR.Net(kind).loadFromString(bad["a neuron line is missing"]).unset() == [(0, 1)]


def test_factory_names_and_the_refusals_that_stay():
    f = RankerFactory()
    for kind, cls in KINDS.items():
        r = f.loadRankerFromString("## %s\n1\n0\n0 0 1.0\n0 1 0.0\n" % kind)
        assert type(r) is cls and type(r.createNew()) is cls
        r2 = f.loadRankerFromString("## %s  \n1\n0\n0 0 1.0\n0 1 0.0\n" % kind.upper())       # name().toUpperCase(), trimmed
        assert type(r2) is cls
        for call in (r.learn, r.init, cls().learn):
            with pytest.raises(RankLibError) as e:
                call()
            assert "out of scope" in str(e.value) and "neural-net" in str(e.value) and kind.upper() in str(e.value)
        with pytest.raises(RankLibError) as e:
            f.createRanker(RankerType[kind.upper()])
        assert "out of scope" in str(e.value) and kind.upper() in str(e.value)
    with pytest.raises(RankLibError) as e:
        f.loadRankerFromString("## NeuralNet\n1\n0\n")
    for name in ("'## RankNet'", "'## LambdaRank'", "'## ListNet'", "'## Linear Regression'"):
        assert name in str(e.value)
    assert (RankNet.nIteration, LambdaRank.nIteration, ListNet.nIteration) == (100, 100, 1500)


def test_jexp_is_the_oracles_exp():
    import oracle_ffi as O
    xs = [0.0, -0.0, 0.5, -0.5, 36.0, -36.0, 700.5, -700.5, 709.9, -709.9, 745.2, -745.2, 800.0, -800.0, 1e-300, 0.34, -1.04, 2.0 ** -29]
    xs += list(np.random.default_rng(3).standard_normal(200) * 30)
    for x in xs:
        assert _bits(jexp(float(x))) == _bits(O.lib().ro_exp(float(x))), x


def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    for args in (([1, 2], [], [0.0] * 4), ([1, 2], [3], [0.0] * 12), ([], [], [0.0]), ([1], [0], [0.0] * 2), ([1], [2, -1], [0.0] * 5)):
        with pytest.raises(RankLibError) as e:
            N.NetModel(*args)
        assert "status -1" in str(e.value), args          # RL_ERR_INVALID


@pytest.mark.skipif(has_gpu(), reason="the refusal without a device")
def test_no_device_fails_with_no_cpu_fallback():
    with pytest.raises(RankLibError) as e:
        N.NetModel([1, 2], [], [0.5, 0.25, 0.0])
    assert "no CPU fallback" in str(e.value)
    for kind in KINDS:
        r = RankerFactory().loadRankerFromString("## %s\n1 2\n0\n0 0 0.5\n0 1 0.25\n0 2 0.0\n" % kind)
        with pytest.raises(RankLibError) as e:
            r.eval(learning.DataPoint("1 qid:1 1:1.0 2:2.0"))
        assert "no CPU fallback" in str(e.value)
        with pytest.raises(RankLibError) as e:
            r.evalList(learning.RankList([learning.DataPoint("1 qid:1 1:1.0 2:2.0")]))
        assert "no CPU fallback" in str(e.value)
