"""A plain NumPy statement of rl_model_predict_leaves -- TEST INFRASTRUCTURE ONLY.  Trees are tree_models' dicts, nodes in
pre-order; a tree's leaves are numbered in that order, left first."""
import numpy as np


def numbers(tree):
    """int64 [nodes]: the number of every leaf among the tree's leaves in pre-order; -1 at inner nodes"""
    leaf = tree["feature"] == -1
    return np.where(leaf, np.cumsum(leaf) - 1, -1)


def counts(trees):
    return np.array([int((t["feature"] == -1).sum()) for t in trees], np.int32)


def leaves(trees, rows):
    """uint16 [rows][trees]: `value <= threshold` goes left (NaN on either side: right), a column the row does not have reads 0"""
    rows = np.asarray(rows, np.float32)
    n, width = rows.shape
    ar = np.arange(n)
    out = np.zeros((n, len(trees)), np.uint16)
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(trees):
            nd = np.zeros(n, np.int64)
            while (t["feature"][nd] != -1).any():
                f = t["feature"][nd].astype(np.int64)
                v = np.where(f < width, rows[ar, np.clip(f, 0, width - 1)], np.float32(0))
                nd = np.where(f == -1, nd, np.where(v <= t["threshold"][nd], t["left"][nd], t["right"][nd]))
            out[:, k] = numbers(t)[nd]
    return out
