"""The packed format of k_model_eval_tiled, read back independently -- TEST INFRASTRUCTURE ONLY.

tools/eval_pack_host_check.cpp prints what rl_eval_pack_host.h's eval_pack makes of a model file.  `parse` decodes that output,
`check_structure` holds it against the trees it was made from (tests/tree_models.py) rule by rule, and `replay` walks it as the kernel
does -- the staged tile with -infinity in column 0, the walkers' chains in lockstep through their phases, the leaf value from a word's low
half, Ensemble.eval's accumulation in tree order -- in numpy, vectorised over the documents.  Nothing here calls the library.
"""
import numpy as np

import tree_models as TM

NONE = 255


def parse(text):
    """the program's output as a dict: shape constants, ok / why, maxcol, nodes [trees][maxn] uint64, perm and meta [tiles][..] uint8"""
    pk = {}
    for ln in text.splitlines():
        key, _, rest = ln.partition(" ")
        if key == "shape":
            names = ("trees", "maxn", "docs", "parts", "per", "phases", "ph1", "ph2", "phlast")
            pk.update(zip(names, (int(x) for x in rest.split())))
        elif key in ("ok", "refused"):
            pk["ok"], pk["why"] = key == "ok", rest
        elif key == "maxcol":
            pk["maxcol"] = int(rest)
        elif key == "nodes":
            pk["nodes"] = np.array([int(x, 16) for x in rest.split()], np.uint64)
        elif key in ("perm", "meta"):
            pk[key] = np.array([int(x, 16) for x in rest.split()], np.uint8)
    tile, md = pk["parts"] * pk["per"], pk["parts"] * (1 + pk["phases"])
    pk["tile"], pk["tiles"] = tile, (pk["trees"] + tile - 1) // tile
    if pk["ok"]:
        pk["nodes"] = pk["nodes"].reshape(pk["trees"], pk["maxn"])
        pk["perm"] = pk["perm"].reshape(pk["tiles"], tile)
        pk["meta"] = pk["meta"].reshape(pk["tiles"], md)
    return pk


def _fields(word):
    word = int(word)
    return word & 0xffffffff, (word >> 32) & 0xffff, word >> 48          # value bits, column byte offset, left child byte offset


def _same_float_bits(bits, f):
    want = int(np.array([f], np.float32).view(np.uint32)[0])
    return bits == want or (np.isnan(f) and np.isnan(np.array([bits], np.uint32).view(np.float32)[0]))


def check_nodes(pk, trees):
    """every tree against its packed words, walked side by side from the root: a split carries its threshold and its column's offset and
    its children lie next to each other inside the tree; a leaf carries its output, column offset 0 and points at itself; every word of
    the tree is reached once and the padding is zero"""
    for t, words in zip(trees, pk["nodes"]):
        n = len(t["feature"])
        seen = np.zeros(pk["maxn"], bool)
        todo = [(0, 0)]                                   # (packed index, node of the tree)
        while todo:
            h, j = todo.pop()
            assert 0 <= h < n and not seen[h], (h, j)
            seen[h] = True
            bits, col, left = _fields(words[h])
            if t["feature"][j] == -1:
                assert col == 0 and left == 8 * h and _same_float_bits(bits, t["output"][j]), (h, j)
            else:
                assert col == int(t["feature"][j]) * pk["docs"] * 4 and _same_float_bits(bits, t["threshold"][j]), (h, j)
                assert left % 8 == 0 and left // 8 + 1 < n, (h, j)
                todo += [(left // 8, int(t["left"][j])), (left // 8 + 1, int(t["right"][j]))]     # adjacent: right = left + 1
        assert seen[:n].all() and not words[n:].any()


def check_tiles(pk, trees, phased):
    """perm, the walkers' steps and their phase ends, tile by tile"""
    tile, per, parts, phases = pk["tile"], pk["per"], pk["parts"], pk["phases"]
    next_ch = (pk["ph1"] if phases >= 2 else pk["phlast"], pk["ph2"] if phases >= 3 else pk["phlast"], pk["phlast"])
    steps_of = [max(TM.depth_of(t), 1) for t in trees]   # (a single leaf still takes one step: its output is stored)
    for k in range(pk["tiles"]):
        t0, tt = k * tile, min(tile, len(trees) - k * tile)
        perm, meta = pk["perm"][k], pk["meta"][k]
        real = perm[perm != NONE]
        assert sorted(real.tolist()) == list(range(tt)), k
        assert tt == tile or k == pk["tiles"] - 1                        # 255 only in the last, partial tile
        for p in range(parts):
            mine = perm[p * per:(p + 1) * per]
            mine = mine[mine != NONE]
            assert (perm[p * per:p * per + len(mine)] != NONE).all()     # a walker's trees come first, then the empty chains
            d = [steps_of[t0 + int(li)] for li in mine]
            assert d == sorted(d, reverse=True), (k, p, d)               # deepest first
            assert meta[p] == (max(d) if d else 0), (k, p)
            ends = meta[parts + p * phases:parts + (p + 1) * phases]
            want = [meta[p]] * phases if not phased else [d[next_ch[ph]] if next_ch[ph] < len(d) else 0 for ph in range(phases)]
            assert ends.tolist() == [int(x) for x in want], (k, p, ends, want)


def check_structure(pk, trees, phased):
    assert pk["trees"] == len(trees) and pk["maxn"] == max(len(t["feature"]) for t in trees)
    assert pk["maxcol"] == max([int(t["feature"].max()) for t in trees] + [0])
    check_nodes(pk, trees)
    check_tiles(pk, trees, phased)


def replay(pk, weights, rows):
    """k_model_eval_tiled's walk over the packed words.  The staged tile sX[column][doc] has -infinity in column 0 and 0 in the columns
    the rows lack.  Per tile of trees and walker: chain u starts at the root of tree perm[p * per + u] (tree 0 of the tile where there
    is none; its result is dropped), all `per` chains step to the first phase end, then ph1, ph2 and phlast of them to theirs, the last
    to the walker's steps.  A step: x = sX[column of the word]; next word = left child, or the one behind it unless x <= value.  The leaf
    output is the low half of the word a chain ends on.  Then s = f32(f64(s) + f64(out) * f64(w)), in the ensemble's order."""
    rows = np.asarray(rows, np.float32)
    n, width = rows.shape
    cols = max(width, pk["maxcol"] + 1)
    sX = np.zeros((cols, n), np.float32)
    sX[:width] = rows.T
    sX[0] = -np.inf
    docs, tile, per, parts, phases = pk["docs"], pk["tile"], pk["per"], pk["parts"], pk["phases"]
    chains = [per] + [pk["ph1"], pk["ph2"]][:phases - 1] + [pk["phlast"]]          # the chains still walking in each of the phases + 1 loops
    ar = np.arange(n)
    outs = np.zeros((pk["trees"], n), np.float32)
    with np.errstate(all="ignore"):
        for k in range(pk["tiles"]):
            t0, tt = k * tile, min(tile, pk["trees"] - k * tile)
            perm, meta = pk["perm"][k], pk["meta"][k]
            for p in range(parts):
                depth = int(meta[p])
                if depth == 0:
                    continue
                li = [int(x) for x in perm[p * per:(p + 1) * per]]
                base = [pk["nodes"][t0 + (x if x < tt else 0)] for x in li]
                v = [np.full(n, b[0], np.uint64) for b in base]
                until = [int(x) for x in meta[parts + p * phases:parts + (p + 1) * phases]] + [depth]
                step = 0
                for nch, end in zip(chains, until):
                    while step < end:
                        x = [sX[((v[u] >> np.uint64(32)) & np.uint64(0xffff)).astype(np.int64) // (docs * 4), ar] for u in range(nch)]
                        for u in range(nch):
                            thr = (v[u] & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32)
                            off = (v[u] >> np.uint64(48)).astype(np.int64) + np.where(x[u] <= thr, 0, 8)
                            assert (off // 8 < pk["maxn"]).all()
                            v[u] = base[u][off // 8]
                        step += 1
                for u in range(per):
                    if li[u] < tt:
                        outs[t0 + li[u]] = (v[u] & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32)
        s = np.zeros(n, np.float32)
        for t in range(pk["trees"]):
            s = (s.astype(np.float64) + outs[t].astype(np.float64) * np.float64(np.float32(weights[t]))).astype(np.float32)
    return s
