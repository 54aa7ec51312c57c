"""Data sets that put chosen label patterns at chosen ranked positions, and a classifier that names the branches of PrecisionScorer.swapChange
and ReciprocalRankScorer.swapChange a ranked list reaches.

Round 0 of a tree trainer has every model score at 0.0 and the ranking is stable, so the ranked order of round 0 is the file's order: a data
set decides which branch of a swap-change matrix every list takes.  `enumerated(k)` holds every label string over (0, 0.5, 1, 2) of up to
k + 2 documents; `structured(k)` puts the first two relevant documents at chosen positions of lists on both sides of every length class of
the lambda kernels; `huge()` adds a list past the block rank kernel's cap.

The classifiers are written from the two Java files, not from tests/pr_restatement.py: tests/test_tree_pr_branches_cpu.py holds the two
against each other.  A case is reached by a pair LambdaMART takes (`label_j > label_k` as floats, either order: LambdaMART.java:375-381).

P (metric/PrecisionScorer.java:57-77), size = min(n, k), pairs i < size <= j:
    n<=k        the list has no position j >= size: the whole matrix is zero
    top_rel     i relevant, j not
    tail_rel    j relevant, i not
    c0          different labels, the same binary view: the entry is 0 and the pair contributes nothing

RR (metric/ReciprocalRankScorer.java:48-107), first / second = the first two positions below size with label > 0.0:
    first-1 first second-1 second       first == -1, first != -1, second == -1, second != -1, of a list that reaches one of the cases below
    L1:nosec L1:j<sec L1:j>=sec         :74-83, j in (first, size), (int) label_j == 0
    L2:nosec L2:sec                     :84-93, j in [size, n), (int) label_j == 0
    L3:nofirst                          :99-105 with first == -1 (rows below size against the relevant documents from size on)
    L3:j=first L3:j>first L3:j>=size    :99-105 with a first: the column is first itself, between first and size, from size on
    ...:half                            the "non-relevant" document of loop 1 or 2 has label 0.5 ((int) 0.5 == 0, and 0.5 > 0.0)
"""
import functools
import itertools

import numpy as np

ALPHABET = (0.0, 0.5, 1.0, 2.0)
P_NAMES = frozenset(("n<=k", "top_rel", "tail_rel", "c0"))
RR_NAMES = frozenset(("first-1", "first", "second-1", "second", "L1:nosec", "L1:j<sec", "L1:j>=sec", "L1:j>=sec:half", "L2:nosec", "L2:nosec:half",
                      "L2:sec", "L2:sec:half", "L3:nofirst", "L3:j=first", "L3:j>first", "L3:j>=size"))
# what no list can reach at a small k (derived in tests/test_tree_pr_branches_cpu.py)
RR_UNREACHABLE = {1: frozenset(("second", "L1:nosec", "L1:j<sec", "L1:j>=sec", "L1:j>=sec:half", "L2:sec", "L2:sec:half", "L3:j=first", "L3:j>first",
                                "L3:j>=size")),
                  2: frozenset(("L1:j<sec", "L1:j>=sec", "L3:j>first"))}
STRUCTURED_LENGTHS = (63, 64, 65, 128, 129, 192, 193, 256, 257, 600)     # and k - 1, k, k + 1
HUGE_LENGTH = 5001                                                        # past the block rank kernel's cap of 5000 documents


# ---- the classifiers ------------------------------------------------------------------------------------------------------------------------
def p_branches(ranked_labels, k):
    lab = [float(v) for v in ranked_labels]
    n = len(lab)
    size = k if n > k else n
    if n <= k:
        return {"n<=k"}
    out = set()
    for i in range(size):
        for j in range(size, n):
            if lab[i] != lab[j]:
                ri, rj = lab[i] > 0.0, lab[j] > 0.0
                out.add("c0" if ri == rj else "top_rel" if ri else "tail_rel")
    return out


def rr_branches(ranked_labels, k):
    lab = [float(v) for v in ranked_labels]
    n = len(lab)
    size = k if n > k else n
    rel = [i for i in range(size) if lab[i] > 0.0]
    first, second = (rel + [-1, -1])[:2]
    out = set()
    if first != -1:
        for j in range(first + 1, n):
            if int(lab[j]) == 0 and lab[j] != lab[first]:
                if j < size:
                    name = "L1:nosec" if second == -1 else "L1:j<sec" if j < second else "L1:j>=sec"
                else:
                    name = "L2:nosec" if second == -1 else "L2:sec"
                out.add(name + (":half" if lab[j] == 0.5 else ""))
    feff = first if first != -1 else size
    for i in range(feff):
        for j in range(feff, n):
            if lab[j] > 0.0 and lab[j] != lab[i]:
                out.add("L3:nofirst" if first == -1 else "L3:j=first" if j == first else "L3:j>first" if j < size else "L3:j>=size")
    if out:
        out |= {"first-1" if first == -1 else "first", "second-1" if second == -1 else "second"}
    return out


BRANCHES = {"P": p_branches, "RR": rr_branches}
NAMES = {"P": P_NAMES, "RR": RR_NAMES}


def reachable(metric, k):
    """the cases some list can reach at this k"""
    return NAMES[metric] - (RR_UNREACHABLE.get(k, frozenset()) if metric == "RR" else frozenset())


def reached(metric, k, labels, qoff, scores=None):
    """the union of the cases the lists reach when ranked by `scores` (stable, descending; None: the file's order, which is round 0's)"""
    out = set()
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        lab = [float(v) for v in labels[a:b]]
        if scores is not None:
            s = scores[a:b]
            lab = [lab[i] for i in sorted(range(b - a), key=lambda i: -s[i])]      # sorted() is stable
        out |= BRANCHES[metric](lab, k)
    return out


# ---- round 0 without a ranking ----------------------------------------------------------------------------------------------------------------
def direct_round0(scorer, labels, qoff):
    """lambda and weight of round 0 from the scorer's matrix alone: every score is 0.0, so the ranked order is the file's and rho is 0.5 for every
    pair.  The pairs in the order LambdaMART.java:371-393 visits them (j outer, k inner, its break at the cutoff)."""
    lam, w = np.zeros(len(labels), np.float64), np.zeros(len(labels), np.float64)
    cutoff = scorer.k
    for q in range(len(qoff) - 1):
        cur, end = int(qoff[q]), int(qoff[q + 1])
        lab = [float(v) for v in labels[cur:end]]
        changes = scorer.swap_change(lab, "q%d" % q)
        n = end - cur
        for j in range(n):
            row = changes[j]
            for k in range(n):
                if j > cutoff and k > cutoff:
                    break
                if lab[j] > lab[k]:
                    d = abs(row[k])
                    if d > 0:
                        lam[cur + j] += 0.5 * d
                        lam[cur + k] -= 0.5 * d
                        w[cur + j] += 0.5 * (1.0 - 0.5) * d
                        w[cur + k] += 0.5 * (1.0 - 0.5) * d
    return lam, w


# ---- the data ---------------------------------------------------------------------------------------------------------------------------------
def _pack(lists, seed, frozen=()):
    """frozen: lists whose documents all take the feature row of the first, so that every model scores them alike and their ranked order stays
    the file's in every round"""
    qoff = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    lab = np.array([v for l in lists for v in l], np.float32)
    rng = np.random.default_rng(seed)
    X = (rng.integers(0, 8, (len(lab), 4)) / 8).astype(np.float32)
    for q in frozen:
        X[qoff[q]:qoff[q + 1]] = X[qoff[q]]
    for a in (X, lab, qoff):
        a.setflags(write=False)
    return X, lab, qoff


@functools.lru_cache(maxsize=None)
def enumerated(k):
    """every label string over (0, 0.5, 1, 2) of 1 .. k + 2 documents, one list each"""
    return _pack([s for n in range(1, k + 3) for s in itertools.product(ALPHABET, repeat=n)], k)


def _patterns(k):
    h = k // 2
    seen = []
    for p in ((-1, -1), (0, -1), (0, 1), (0, k - 1), (1, 3), (k - 2, k - 1), (k - 1, -1), (h, -1), (h, h + 2)):
        if p not in seen:
            seen.append(p)
    return seen


def _structured_list(n, k, first, second, swap, half=True, head_half=False):
    """label 0 in the top size = min(n, k) except `first` and `second` (1 and 2, or 2 and 1), a 0.5 directly after each where there is room
    (half: a 0.5 inside the top is relevant, so it is the Java's secondRank where it precedes `second`), then (0, 0.5, 1, 2) repeated"""
    size = min(n, k)
    lab = [0.0] * size + [ALPHABET[(i - size) % 4] for i in range(size, n)]
    hi, lo = (2.0, 1.0) if swap else (1.0, 2.0)
    if first != -1:
        lab[first] = hi
        if half and first + 1 < size and first + 1 != second:
            lab[first + 1] = 0.5
    if second != -1:
        lab[second] = lo
        if half and second + 1 < size:
            lab[second + 1] = 0.5
    if head_half:
        lab[0] = 0.5
    return lab


def _structured_lists(k, lengths, frozen_lengths=()):
    """(lists, indices of the frozen ones)"""
    lists, frozen = [], []
    for n in lengths:
        at = len(lists)
        size = min(n, k)
        for first, second in _patterns(k):
            if first >= size or second >= size:
                continue
            swap = len(lists) % 2 == 1
            lists.append(_structured_list(n, k, first, second, swap))
            if first == -1:                                              # a second copy whose 0.5 at position 0 is `first`
                lists.append(_structured_list(n, k, first, second, swap, head_half=True))
            elif second == -1 or second > first + 1:                     # added: without the 0.5s, so that `second` is the Java's secondRank
                plain = _structured_list(n, k, first, second, swap, half=False)
                if plain != lists[-1]:
                    lists.append(plain)
        if n in frozen_lengths:                                          # added: a frozen copy of this length's lists (below)
            lists += [list(l) for l in lists[at:]]
            frozen += range((at + len(lists)) // 2, len(lists))
    return lists, frozen


@functools.lru_cache(maxsize=None)
def structured(k):
    """Two things are added to the lists the patterns give, because the cases they are for were not reached without them: the copies without a
    0.5 (a 0.5 directly after `first` is relevant and so the Java's secondRank: no list reached L1:j<sec in any round, and L1:nosec only with
    a 0.5 as `first`), and frozen copies of the lists of k + 1, 65 and 257 documents (once a model ranks by the
    features, the relevant three quarters of every tail crowd the top: no list without a `first`, and none with a 0.5 past the cutoff and
    no `second`, was left in rounds 1 and 2 of RR@16, 17 and 20)."""
    lists, frozen = _structured_lists(k, sorted({k - 1, k, k + 1} | set(STRUCTURED_LENGTHS)), (k + 1, 65, 257))
    return _pack(lists, k, frozen)


@functools.lru_cache(maxsize=None)
def huge():
    """the structured lists of 64, 257 and 600 documents for k = 10, and one list of 5 001 with first = 3, second = 12 (600: between the
    wavefront rank kernel's 384 documents and the block kernel's 5 000, so that a launch of the block kernel exists to be told from the mixed one)"""
    lists, _ = _structured_lists(10, (64, 257, 600))
    big = [ALPHABET[(i - 13) % 4] if i > 12 else 0.0 for i in range(HUGE_LENGTH)]
    big[3], big[12] = 1.0, 2.0
    return _pack(lists + [big], HUGE_LENGTH)
