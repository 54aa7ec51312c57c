"""metric/PrecisionScorer.java and metric/ReciprocalRankScorer.java, transcribed: score and swapChange as the Java writes them, an explicit
n x n matrix, numpy.float32 where the Java has a float.  Python float == Java double.

Both classes have the interface of the scorers of tests/np_restatement.py (.k, .score(lab_ranked, qid), .swap_change(lab_ranked, qid)), so a
np_restatement.LambdaMART takes one as its scorer:

    m = R.LambdaMART(X, lab, qoff, metric="NDCG", k=k, ...)
    m.scorer = P(k)
"""
import numpy as np

F32 = np.float32


class P:  # metric/PrecisionScorer.java
    def __init__(self, k=10):  # :21-27
        self.k = k

    def score(self, lab_ranked, qid):  # :30-44
        count = 0
        n = len(lab_ranked)
        size = self.k
        if self.k > n or self.k <= 0:
            size = n
        for i in range(size):
            if lab_ranked[i] > 0.0:
                count += 1
        return float(count) / size

    @staticmethod
    def _binary(label):  # :79-84
        return 1 if label > 0.0 else 0

    def swap_change(self, lab_ranked, qid):  # :57-77
        n = len(lab_ranked)
        size = self.k if n > self.k else n
        changes = [[0.0] * n for _ in range(n)]
        for i in range(size):
            for j in range(size, n):
                c = self._binary(lab_ranked[j]) - self._binary(lab_ranked[i])
                changes[i][j] = changes[j][i] = float(F32(c) / F32(size))  # ((float) c) / size: a float division, widened on the store
        return changes


class RR:  # metric/ReciprocalRankScorer.java
    def __init__(self, k=0):  # :21-23
        self.k = k

    def score(self, lab_ranked, qid):  # :26-35
        n = len(lab_ranked)
        size = self.k if n > self.k else n
        first_rank = -1
        i = 0
        while i < size and first_rank == -1:
            if lab_ranked[i] > 0.0:
                first_rank = i + 1
            i += 1
        return 0.0 if first_rank == -1 else float(F32(1.0) / F32(first_rank))  # 1.0f / firstRank

    def swap_change(self, lab_ranked, qid):  # :48-107
        n = len(lab_ranked)
        first_rank = -1
        second_rank = -1
        size = self.k if n > self.k else n
        for i in range(size):
            if lab_ranked[i] > 0.0:  # relevant
                if first_rank == -1:
                    first_rank = i
                elif second_rank == -1:
                    second_rank = i
        changes = [[0.0] * n for _ in range(n)]
        rr = 0.0
        if first_rank != -1:
            rr = 1.0 / (first_rank + 1)
            for j in range(first_rank + 1, size):
                if int(lab_ranked[j]) == 0:  # non-relevant: ((int) label) == 0
                    if second_rank == -1 or j < second_rank:
                        changes[first_rank][j] = changes[j][first_rank] = 1.0 / (j + 1) - rr
                    else:
                        changes[first_rank][j] = changes[j][first_rank] = 1.0 / (second_rank + 1) - rr
            for j in range(size, n):
                if int(lab_ranked[j]) == 0:
                    if second_rank == -1:
                        changes[first_rank][j] = changes[j][first_rank] = -rr
                    else:
                        changes[first_rank][j] = changes[j][first_rank] = 1.0 / (second_rank + 1) - rr
        else:
            first_rank = size
        for i in range(first_rank):
            for j in range(first_rank, n):
                if lab_ranked[j] > 0:
                    changes[i][j] = changes[j][i] = 1.0 / (i + 1) - rr
        return changes
