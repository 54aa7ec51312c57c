"""The host side of a set of ranked lists (ranklib_amd/csrc/rl_lists_host.h: check_lists, ListSetHost, ideal_cache) without a GPU:
tools/lists_host_check.cpp is built with the host compiler and its fixed table of cases is recomputed here from the inputs it prints --
the idealGains rule as a literal dict, its DCGs from ranklib_amd.metric.NDCGScorer, and where the scorer can express the case
(NDCGScorer's own cut-off) NDCGScorer.scoreOne driven list by list in the same order.  Every comparison is bit for bit."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from ranklib_amd import metric as M
from ranklib_amd.learning import DataPoint, RankList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFUSALS = {    # case -> (code, the whole message)
    "f.start": (-1, "qoff must start at 0"),
    "f.empty": (-1, "rl_x: qoff must be strictly increasing (empty ranked list 1)"),
    "f.past": (-1, "qoff must end at n_docs (list 1 runs past it)"),
    "f.end": (-1, "rl_x: qoff must end at n_docs"),
    "f.negative": (-1, "Relevance label cannot be negative. System will now exit."),
    "f.nan": (-1, "rl_x: Relevance label cannot be negative. System will now exit."),
    "f.big": (-4, "relevance label of 2^24 or more"),
    "f.rd": (-1, "negative relevant-document count"),
    "f.rd.prep": (-1, "rl_x: negative relevant-document count"),
}
IDEAL_CASES = ["a", "a.trainer", "b", "b.trainer", "c", "c.trainer", "c.one_set"] + \
              ["d.k%d.%s" % (k, r) for k in (10, 3, 0) for r in ("trainer", "eval")] + ["e", "e.trainer"]


def hexbits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("lists_host") / "lists_host_check")
    subprocess.check_call([cxx, "-std=c++17", os.path.join(ROOT, "tools", "lists_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    parsed, cur = {}, None
    for line in out.stdout.splitlines():
        head, _, rest = line.partition(" ")
        if head == "case":
            cur = parsed.setdefault(rest.split(" ")[0], {"args": dict(a.split("=") for a in rest.split(" ")[1:])})
        elif head == "rc":
            code, _, msg = rest.partition(" ")
            cur["rc"] = (int(code), msg)
        else:
            cur[head] = rest.split(" ") if rest else []
    return parsed


def sets_of(c):
    """the printed inputs: per set (labels, qoff, ids, external table or None); a list without a qkey has an id of its own"""
    out = []
    for s in (0, 1):
        if "qoff%d" % s not in c:
            break
        qoff = [int(v) for v in c["qoff%d" % s]]
        labels = [float(np.float32(float(v))) for v in c["labels%d" % s]]
        ids = [int(v) for v in c["qkey%d" % s]] if "qkey%d" % s in c else [("anonymous", s, q) for q in range(len(qoff) - 1)]
        ext = [float(v) for v in c["ext%d" % s]] if "ext%d" % s in c else None
        out.append((labels, qoff, ids, ext))
    return out


def restate(sets, k, rule):
    """NDCGScorer.java:114-122,134-143 with idealGains as a dict: the external entries first, then the first list of an id decides"""
    scorer = M.NDCGScorer(k)
    size_of = (lambda n: min(n, k)) if rule == "trainer" else (lambda n: n if (k > n or k <= 0) else k)
    gains = {}
    for labels, qoff, ids, ext in sets:
        for q, qid in enumerate(ids):
            if ext is not None and not math.isnan(ext[q]):
                gains[qid] = ext[q]
    external = dict(gains)
    own, cached = [], []
    for labels, qoff, ids, ext in sets:
        own.append([])
        cached.append([])
        for q, qid in enumerate(ids):
            rel = [int(l) for l in labels[qoff[q]:qoff[q + 1]]]
            mine = external[qid] if qid in external else scorer.getIdealDCG(rel, size_of(len(rel)))
            gains.setdefault(qid, mine)
            own[-1].append(mine)
            cached[-1].append(gains[qid])
    return own, cached, external


def by_scorer(sets, k, external):
    """NDCGScorer.scoreOne list by list, training set first: what idealGains holds for a list's id once the list has been scored"""
    scorer = M.NDCGScorer(k)
    scorer.idealGains = {str(i): v for i, v in external.items()}
    cached = []
    for labels, qoff, ids, ext in sets:
        cached.append([])
        for q, qid in enumerate(ids):
            rl = RankList([DataPoint.from_parsed(l, str(qid), "# d%d" % i, np.zeros(2, np.float32)) for i, l in enumerate(labels[qoff[q]:qoff[q + 1]])])
            scorer.scoreOne(rl)
            cached[-1].append(scorer.idealGains[rl.getID()])
    return cached


def test_the_table_of_cases_is_the_expected_one(cases):
    assert list(cases) == IDEAL_CASES + list(REFUSALS)


@pytest.mark.parametrize("name", IDEAL_CASES)
def test_own_and_cached_ideals_bit_for_bit(cases, name):
    c = cases[name]
    assert c["rc"] == (0, "")
    k, rule = int(c["args"]["k"]), c["args"]["rule"]
    sets = sets_of(c)
    own, cached, external = restate(sets, k, rule)
    for s in range(len(sets)):
        assert c["own%d" % s] == [hexbits(v) for v in own[s]], (name, "own", s)
        assert c["cached%d" % s] == [hexbits(v) for v in cached[s]], (name, "cached", s)
    if rule == "eval":       # the scorer's own cut-off: the scorer itself agrees, and so does eval_prepare_lists where the tool ran it
        assert by_scorer(sets, k, external) == cached
        if "prep0" in c:
            assert c["prep0"] == c["cached0"]


def test_the_cases_show_what_they_are_there_for(cases):
    a, b, c = cases["a"], cases["b"], cases["c"]
    assert a["cached1"][0] == a["cached0"][0] and a["own1"][0] != a["cached1"][0]      # the shared key: the training list's ideal
    assert all(b["own%d" % s] == b["cached%d" % s] for s in (0, 1)) and b["own1"][0] == a["own1"][0]      # without keys nothing is shared
    assert c["cached0"][0] == c["cached1"][0] == c["own1"][0] == hexbits(2.5) and c["cached0"][1] == a["cached0"][1]
    assert cases["d.k0.trainer"]["cached0"] == [hexbits(0.0)] * 3 and cases["d.k0.eval"]["cached0"] == cases["d.k10.eval"]["cached0"]
    assert cases["d.k3.trainer"]["cached0"] == cases["d.k3.eval"]["cached0"] != cases["d.k10.eval"]["cached0"]
    # 1.7 -> 1, (1 << 31) - 1, 1 << 32 wraps to 1 << 0, 1 << 33 to 1 << 1, 16777215 & 31 == 31
    assert cases["e"]["cached0"][1:] == [hexbits(v) for v in (0.0, 1.0, 2147483647.0, 0.0, 1.0, 2147483647.0)]


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_have_their_code_and_whole_message(cases, name):
    assert cases[name]["rc"] == REFUSALS[name]
