"""The branch classifiers and data sets of tests/pr_cases.py, without a GPU: the classifiers against the matrices of tests/pr_restatement.py
and against hand-derived lists, the set of cases each k can reach, the condition under which tests/test_gpu_tree_pr_branches.py is not
vacuous (every compared round reaches every case, moves a quarter of the documents and splits), and scorers with one branch broken, which the
round-0 lambdas of that data tell from the right ones."""
import numpy as np
import pytest

import np_restatement as R
import pr_cases as C
from pr_restatement import P, RR

SCORERS = {"P": P, "RR": RR}
F32 = np.float32


# ---- 1. the classifiers against the matrices ------------------------------------------------------------------------------------------------
def _p_expect(lab, k, a, b):
    """(case, the value PrecisionScorer.java:71-73 stores) of the pair a < b, None where it stores nothing"""
    n = len(lab)
    size = k if n > k else n
    if not a < size <= b:
        return None
    c = (1 if lab[b] > 0.0 else 0) - (1 if lab[a] > 0.0 else 0)
    return {0: "c0", -1: "top_rel", 1: "tail_rel"}[c], float(F32(c) / F32(size))


def _rr_expect(lab, k, a, b):
    """(case, the value of the assignment of ReciprocalRankScorer.java that stands at the end) of the pair a < b, None where none is made"""
    n = len(lab)
    size = k if n > k else n
    first = second = -1
    for i in range(size):
        if lab[i] > 0.0:
            if first == -1:
                first = i
            elif second == -1:
                second = i
    rr = 1.0 / (first + 1) if first != -1 else 0.0
    feff = first if first != -1 else size
    if a < feff <= b and lab[b] > 0:                                     # :99-105, the last loop
        return ("L3:nofirst" if first == -1 else "L3:j=first" if b == first else "L3:j>first" if b < size else "L3:j>=size"), 1.0 / (a + 1) - rr
    if first != -1 and a == first and int(lab[b]) == 0:
        half = ":half" if lab[b] == 0.5 else ""
        if b < size:                                                     # :74-83
            if second == -1:
                return "L1:nosec" + half, 1.0 / (b + 1) - rr
            return ("L1:j<sec" + half, 1.0 / (b + 1) - rr) if b < second else ("L1:j>=sec" + half, 1.0 / (second + 1) - rr)
        return ("L2:nosec" + half, -rr) if second == -1 else ("L2:sec" + half, 1.0 / (second + 1) - rr)      # :84-93
    return None


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("metric", ["P", "RR"])
def test_a_case_is_named_exactly_where_the_matrix_holds_its_entry(metric, k):
    X, labels, qoff = C.enumerated(k)
    expect = {"P": _p_expect, "RR": _rr_expect}[metric]
    scorer = SCORERS[metric](k)
    for q in range(len(qoff) - 1):
        lab = [float(v) for v in labels[qoff[q]:qoff[q + 1]]]
        n = len(lab)
        m = scorer.swap_change(lab, "q")
        want = set()
        for a in range(n):
            for b in range(a + 1, n):
                assert m[a][b] == m[b][a]
                e = expect(lab, k, a, b)
                if e is None:
                    assert m[a][b] == 0.0, (lab, a, b)                   # no entry goes unnamed
                    continue
                name, value = e
                assert m[a][b] == value and (value != 0.0) == (name != "c0"), (lab, a, b, name, value, m[a][b])
                if lab[a] != lab[b]:                                     # a pair LambdaMART takes
                    want.add(name)
        if metric == "P":
            want = {"n<=k"} if n <= k else want
        elif want:
            size = min(n, k)
            rel = [i for i in range(size) if lab[i] > 0.0]
            want |= {"first" if rel else "first-1", "second" if len(rel) > 1 else "second-1"}
        assert C.BRANCHES[metric](lab, k) == want, (lab, k)
        assert want <= C.NAMES[metric]


# derived by hand from PrecisionScorer.java:57-77
P_KNOWN = [
    (10, [1, 0, 2, 0.5, 0, 3, 0, 1], {"n<=k"}),
    (8, [1, 0, 2, 0.5, 0, 3, 0, 1], {"n<=k"}),
    (1, [2], {"n<=k"}),
    # top 1 0 2 | tail 0.5 0 3 0 1: (1, 0.5) and (1, 3) are relevant both; (1, 0) loses; (0, 0.5) gains; (1, 1) and (0, 0) are no pairs
    (3, [1, 0, 2, 0.5, 0, 3, 0, 1], {"c0", "top_rel", "tail_rel"}),
    (1, [2, 1, 0], {"c0", "top_rel"}),
    (2, [0, 0, 0, 1], {"tail_rel"}),
    (2, [0, 0, 0.5, 0], {"tail_rel"}),                                   # 0.5 > 0.0: relevant
    (2, [1, 2, 0, 0], {"top_rel"}),
    (2, [2, 2, 1, 0.5], {"c0"}),
    (1, [1, 1, 1], set()),                                               # equal labels: LambdaMART takes no pair
    (1, [0, 0, 0], set()),
]

# derived by hand from ReciprocalRankScorer.java:48-107
RR_KNOWN = [
    # no relevant document below size: rows 0 .. size - 1 against the relevant columns from size on
    (3, [0, 0, 0, 2, 0, 1], {"first-1", "second-1", "L3:nofirst"}),
    (2, [0, 0, 0.5, 0], {"first-1", "second-1", "L3:nofirst"}),
    (2, [0, 0, 1, 0.5], {"first-1", "second-1", "L3:nofirst"}),
    # first 1, no second, size 4: columns 2, 3 in loop 1; 4 and 6 (0.5) in loop 2; row 0 against 1 (first), 5 and 6 (past size)
    (4, [0, 2, 0, 0, 0, 1, 0.5], {"first", "second-1", "L1:nosec", "L2:nosec", "L2:nosec:half", "L3:j=first", "L3:j>=size"}),
    # first 1, second 3, size 6: column 2 before second, 4 and 5 (0.5) from it on, 7 past size; row 0 against 1, 3 and 5 (inside), 6 (past size)
    (6, [0, 1, 0, 2, 0, 0.5, 3, 0], {"first", "second", "L1:j<sec", "L1:j>=sec", "L1:j>=sec:half", "L2:sec", "L3:j=first", "L3:j>first", "L3:j>=size"}),
    # size 2, first 1: loop 1 is empty; the 0.5 past size is non-relevant to loop 2 and relevant to loop 3
    (2, [0, 3, 0.5, 0], {"first", "second-1", "L2:nosec", "L2:nosec:half", "L3:j=first", "L3:j>=size"}),
    # the 0.5 at 2 is second: itself and the columns 3, 4 take 1 / (second + 1) - rr, so do 5 and 6 (0.5) past size
    (5, [0, 1, 0.5, 0, 0, 0, 0.5, 0], {"first", "second", "L1:j>=sec", "L1:j>=sec:half", "L2:sec", "L2:sec:half", "L3:j=first", "L3:j>first", "L3:j>=size"}),
    (1, [1, 0, 0.5], {"first", "second-1", "L2:nosec", "L2:nosec:half"}),
    (3, [2, 0, 1, 0], {"first", "second", "L1:j<sec", "L2:sec"}),
    (3, [1, 0, 0, 0], {"first", "second-1", "L1:nosec", "L2:nosec"}),
    (2, [0.5, 0.5, 0], {"first", "second", "L2:sec"}),                   # (first, 1): equal labels, no pair
    (2, [1, 2, 0.5], {"first", "second", "L2:sec:half"}),
    (10, [0, 1, 0, 2], {"first", "second", "L1:j<sec", "L3:j=first", "L3:j>first"}),       # n <= k: size 4, no loop 2
    (3, [0.5, 0.5, 0.5, 0.5], set()),                                    # entries, and no pair that takes one
    (3, [0, 0, 0, 0], set()),
]


def test_classifiers_known_answers():
    for k, lab, want in P_KNOWN:
        assert C.p_branches(lab, k) == want, (k, lab)
    for k, lab, want in RR_KNOWN:
        assert C.rr_branches(lab, k) == want, (k, lab)
    for names, known in ((C.P_NAMES, P_KNOWN), (C.RR_NAMES, RR_KNOWN)):
        for name in names:                                               # two lists at least for every name
            assert sum(name in want for _, _, want in known) >= 2, name


# ---- 2. what a k can reach ---------------------------------------------------------------------------------------------------------------------
RR_ALL = {"first-1", "first", "second-1", "second", "L1:nosec", "L1:j<sec", "L1:j>=sec", "L1:j>=sec:half", "L2:nosec", "L2:nosec:half", "L2:sec",
          "L2:sec:half", "L3:nofirst", "L3:j=first", "L3:j>first", "L3:j>=size"}
RR_AT = {
    # size <= 1: first is 0 or missing, there is no second, loop 1 has no column and loop 3 no row unless first is missing
    1: {"first-1", "first", "second-1", "L2:nosec", "L2:nosec:half", "L3:nofirst"},
    # size <= 2: the only column of loop 1 is 1; it is non-relevant and no second (label 0), or the second itself (label 0.5).  Loop 3 with a first has
    # first == 1, so every column behind it is past size
    2: RR_ALL - {"L1:j<sec", "L1:j>=sec", "L3:j>first"},
    3: RR_ALL, 4: RR_ALL,
}


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_label_string_reaches_exactly_what_its_k_can(k):
    X, lab, qoff = C.enumerated(k)
    assert (len(qoff) - 1, len(lab)) == {1: (84, 228), 2: (340, 1252), 3: (1364, 6372), 4: (5460, 30948)}[k]
    assert X.shape == (len(lab), 4) and X.dtype == np.float32
    assert C.RR_NAMES == RR_ALL and C.P_NAMES == {"n<=k", "top_rel", "tail_rel", "c0"}
    assert C.reached("RR", k, lab, qoff) == RR_AT[k] == C.reachable("RR", k)
    assert C.reached("P", k, lab, qoff) == C.P_NAMES == C.reachable("P", k)


@pytest.mark.parametrize("k", [10, 16, 17, 20])
def test_structured_lists_reach_every_case_at_round_0(k):
    X, lab, qoff = C.structured(k)
    lengths = set(np.diff(qoff).tolist())
    assert lengths == {k - 1, k, k + 1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 600}
    for metric in ("P", "RR"):
        assert C.reached(metric, k, lab, qoff) == C.NAMES[metric]
    for n in (129, 193, 257, 600):                                       # first / second at every chosen position of the lists of several wavefronts
        got = set()
        for q in np.flatnonzero(np.diff(qoff) == n):
            rel = [i for i in range(k) if lab[qoff[q] + i] > 0.0]
            got.add(tuple((rel + [-1, -1])[:2]))
        h = k // 2
        assert got >= {(-1, -1), (0, -1), (0, 1), (0, k - 1), (1, 2), (1, 3), (k - 2, k - 1), (k - 1, -1), (h, -1), (h, h + 1), (h, h + 2)}, (n, got)


def test_huge_holds_a_list_past_the_block_rank_kernel():
    X, lab, qoff = C.huge()
    assert sorted(set(np.diff(qoff).tolist())) == [64, 257, 600, 5001]
    big = lab[qoff[-2]:]
    assert [i for i in range(20) if big[i] > 0.0] == [3, 12, 14, 15, 16, 18, 19]
    for metric, k in (("P", 10), ("RR", 10), ("RR", 20)):
        assert C.BRANCHES[metric](big, k)


# ---- 3. no round is vacuous ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("metric", ["P", "RR"])
def test_every_round_reaches_every_case_moves_a_quarter_and_splits(metric, k):
    X, lab, qoff = C.enumerated(k)
    m = R.LambdaMART(X, lab, qoff, n_trees=3, n_leaves=6, k=k, metric="NDCG")
    m.scorer = SCORERS[metric](k)
    m.init()
    want = C.reached(metric, k, lab, qoff)
    for r in range(3):
        assert C.reached(metric, k, lab, qoff, m.model_scores) >= want, (metric, k, r)      # the order this round's lambdas are made in
        root, _, _, _ = m.round()
        assert np.count_nonzero(m.pseudo) >= len(lab) / 4, (metric, k, r)
        assert root.feature_id != -1, (metric, k, r)
        if r == 0:                                                       # round 0 is the file's order: the direct evaluation is the restatement's
            lam, w = C.direct_round0(m.scorer, lab, qoff)
            assert np.array_equal(lam.view(np.int64), np.array(m.pseudo).view(np.int64))
            assert np.array_equal(w.view(np.int64), np.array(m.weights).view(np.int64))


# ---- 4. a broken branch shows in round 0 ------------------------------------------------------------------------------------------------------------
def _top(lab, k):
    n = len(lab)
    size = k if n > k else n
    rel = [i for i in range(size) if lab[i] > 0.0]
    return (n, size) + tuple((rel + [-1, -1])[:2])


def _set(m, a, b, v):
    m[a][b] = m[b][a] = v


class PCutoffOff(P):                                                     # `b > size` for `b >= size`
    def swap_change(self, lab, qid):
        m = P.swap_change(self, lab, qid)
        n, size, _, _ = _top(lab, self.k)
        for i in range(size if size < n else 0):
            _set(m, i, size, 0.0)
        return m


class PDoubleDivision(P):                                                # c / size in doubles
    def swap_change(self, lab, qid):
        m = P.swap_change(self, lab, qid)
        size = _top(lab, self.k)[1]
        return [[0.0 if v == 0.0 else (1.0 if v > 0 else -1.0) / size for v in row] for row in m]


class RRLoop2WithoutSecond(RR):                                          # -rr where loop 2 has a second
    def swap_change(self, lab, qid):
        m = RR.swap_change(self, lab, qid)
        n, size, first, second = _top(lab, self.k)
        if second != -1:
            for j in range(size, n):
                if int(lab[j]) == 0:
                    _set(m, first, j, -1.0 / (first + 1))
        return m


class RRHalfIsRelevantOnly(RR):                                          # "non-relevant" as !(label > 0): a 0.5 is skipped by loops 1 and 2
    def swap_change(self, lab, qid):
        m = RR.swap_change(self, lab, qid)
        n, size, first, second = _top(lab, self.k)
        if first != -1:
            for j in range(first + 1, n):
                if lab[j] == 0.5:
                    _set(m, first, j, 0.0)
        return m


class RRLoop3FromFirstPlusOne(RR):                                       # loop 3 without the column `first` itself
    def swap_change(self, lab, qid):
        m = RR.swap_change(self, lab, qid)
        n, size, first, second = _top(lab, self.k)
        for i in range(max(first, 0)):
            _set(m, i, first, 0.0)
        return m


class RRSecondPastSize(RR):                                              # second looked for in the whole list
    def swap_change(self, lab, qid):
        n, size, first, second = _top(lab, self.k)
        if first == -1 or second != -1:
            return RR.swap_change(self, lab, qid)
        later = [j for j in range(size, n) if lab[j] > 0.0]
        if not later:
            return RR.swap_change(self, lab, qid)
        m = RR.swap_change(self, lab, qid)
        for j in range(size, n):
            if int(lab[j]) == 0:
                _set(m, first, j, 1.0 / (later[0] + 1) - 1.0 / (first + 1))
        return m


MUTANTS = [PCutoffOff, PDoubleDivision, RRLoop2WithoutSecond, RRHalfIsRelevantOnly, RRLoop3FromFirstPlusOne, RRSecondPastSize]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m.__name__ for m in MUTANTS])
def test_a_scorer_with_one_branch_broken_gives_other_lambdas_at_round_0(mutant, k=3):
    """what the direct evaluation of tests/test_gpu_tree_pr_branches.py can tell apart: each of these scorers differs from the Java in one branch,
    and the round-0 lambdas of the enumerated lists differ with it (k = 3: 1 / 3 is another number as a float)"""
    X, lab, qoff = C.enumerated(k)
    right = C.direct_round0(mutant.__bases__[0](k), lab, qoff)
    wrong = C.direct_round0(mutant(k), lab, qoff)
    assert not np.array_equal(right[0], wrong[0]) and not np.array_equal(right[1], wrong[1])
