"""The small file the chunking tests share: nine lists of 0 to 40 documents with 6-column rows (features 1 - 5), one of
them empty and two of them under one id with different labels, and a 6-tree model over those features.  Under SMALL_LIMIT a call takes 23
such rows, so the file goes in the five chunks written out in CHUNKS: one that ends in the empty list, the list of 40 alone over the
limit, one whose sum meets the limit's 23 rows exactly, and the second list of the shared id in a later chunk than the first."""
import numpy as np

import tree_models as TM
from ranklib_amd.learning import DataPoint, RankList

SIZES = [5, 12, 0, 40, 3, 20, 7, 9, 16]
IDS = ["a", "b", None, "c", "d", "b", "e", "f", "g"]
SMALL_LIMIT = 20 * 7 * 4                                    # 560 bytes: 23 rows of 6 f32 columns (552 bytes), not 24
CHUNKS = [(0, 3), (3, 4), (4, 6), (6, 8), (8, 9)]           # 5 + 12 + 0 | 40 | 3 + 20 | 7 + 9 | 16
CHUNK_ROWS = [17, 40, 23, 16, 16]


def lists(seed=9):
    rng = np.random.default_rng(seed)
    out = []
    for n, qid in zip(SIZES, IDS):
        pts = []
        for _ in range(n):
            fv = rng.choice(TM.GRID, 6).astype(np.float32)
            fv[0] = np.nan
            pts.append(DataPoint.from_parsed(float(rng.integers(0, 5)), qid, "", fv))
        out.append(RankList(pts))
    return out


def model_text():
    rng = np.random.default_rng(19)
    g = TM.Gen(rng, features=range(1, 6))
    trees = [TM.random_tree(g, int(rng.integers(2, 9))) for _ in range(6)]
    return TM.model_text(trees, np.full(6, 0.1, np.float32))
