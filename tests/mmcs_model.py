"""Model of the mixed-height matrix commitments (hades252_mmcs_*), straight from the definition in include/hades252.h: the
row digests of tests/matrix_model.py (row_digests: the C oracle's sponge), the oracle's Merkle level, and nothing else.  The
convention is unpinned, like the sponge and the tree it is made of: parity is pinned to this repository's oracle only."""
import numpy as np

import matrix_model as M
import oracle_lib
from gpu_common import CAP, TAG
import hades_spec as S

INJECT = S.to_mont(31)                  # the injection's domain tag in the tests (the tree's tags are gpu_common.TAG)
BAD = 0xBAD0                            # a tampered scalar is replaced by the in-memory word BAD + k


def depth_of(n, arity):
    """n = arity^d -> d."""
    d = 0
    while n > 1:
        assert n % arity == 0, (n, arity)
        n //= arity
        d += 1
    return d


def by_height(groups):
    """The groups (row-major matrices [h_g, c_g, 4]) tallest first; the heights are distinct."""
    out = sorted((np.ascontiguousarray(g, dtype=np.uint64) for g in groups), key=lambda g: -g.shape[0])
    assert len({g.shape[0] for g in out}) == len(out)
    return out


def inject(oracle, nodes, leaves, inject_tag=INJECT, out_idx=1):
    """nodes[i] <- the parent of the pair (nodes[i], leaves[i]) at arity 2 under the injection tag."""
    pairs = np.stack([np.asarray(nodes).reshape(-1, 4), np.asarray(leaves).reshape(-1, 4)], axis=1)
    return oracle.merkle_level(pairs.reshape(-1), 2, inject_tag, out_idx).reshape(-1, 4)


def commit(oracle, groups, arity, cap=CAP, pad_mode=1, tag=None, inject_tag=INJECT, out_idx=1):
    """(tree [nodes, 4]: node_D, node_{D-1}, ..., the root -- final values, after injection; root [4])."""
    tag = TAG[arity] if tag is None else tag
    groups = by_height(groups)
    at = {depth_of(g.shape[0], arity): M.row_digests(oracle, g, cap, pad_mode) for g in groups}
    D = depth_of(groups[0].shape[0], arity)
    assert D >= 1
    levels = [at[D]]
    for l in range(D - 1, -1, -1):
        node = oracle.merkle_level(levels[-1].reshape(-1), arity, tag, out_idx).reshape(-1, 4)
        if l in at:
            node = inject(oracle, node, at[l], inject_tag, out_idx)
        levels.append(node)
    tree = np.concatenate(levels)
    return tree, tree[-1].copy()


def tree_nodes(max_rows, arity):
    return sum(arity ** l for l in range(depth_of(max_rows, arity) + 1))


def open_paths(tree, max_rows, arity, indices):
    """paths [q, D, arity - 1, 4]: level by level the arity - 1 siblings of the path node in child order, the node's own
    position skipped; an index >= max_rows gives zeros."""
    D = depth_of(max_rows, arity)
    tree = np.asarray(tree).reshape(-1, 4)
    paths = np.zeros((len(indices), D, arity - 1, 4), dtype=np.uint64)
    for t, node in enumerate(int(i) for i in indices):
        if node >= max_rows:
            continue
        off, n = 0, max_rows
        for l in range(D):
            first, pos = node - node % arity, node % arity
            paths[t, l] = [tree[off + first + s] for s in range(arity) if s != pos]
            off, n, node = off + n, n // arity, node // arity
    return paths


def open_rows(groups, index):
    """The opened rows of index `index` < h_0, tallest group first: row index / (h_0 / h_g) of every group."""
    groups = by_height(groups)
    h0 = groups[0].shape[0]
    return [g[index // (h0 // g.shape[0])].copy() for g in groups]


def flat_rows(rows):
    """The opened rows of one query as hades252_mmcs_verify takes them: concatenated, [sum of cols, 4]."""
    return np.concatenate([np.asarray(r).reshape(-1, 4) for r in rows])


def verify(oracle, rows, heights, index, path, arity, cap=CAP, pad_mode=1, tag=None, inject_tag=INJECT, out_idx=1):
    """The root recomputed from one opening: rows[g] [c_g, 4], tallest first; the index is not range-checked."""
    tag = TAG[arity] if tag is None else tag
    path = np.asarray(path).reshape(-1, arity - 1, 4)
    depths = [depth_of(h, arity) for h in heights]
    assert depths == sorted(set(depths), reverse=True) and depths[0] == path.shape[0] >= 1
    leaf = [M.row_digests(oracle, np.asarray(r).reshape(1, -1, 4), cap, pad_mode)[0] for r in rows]
    node, index = leaf[0], int(index)
    for l in range(depths[0] - 1, -1, -1):
        pos, sib = index % arity, list(path[depths[0] - 1 - l])
        node = oracle.merkle_level(np.concatenate(sib[:pos] + [node] + sib[pos:]), arity, tag, out_idx)
        index //= arity
        if l in depths[1:]:
            node = inject(oracle, node, leaf[depths.index(l)], inject_tag, out_idx)[0]
    return np.asarray(node).reshape(4)


def permutations(cols, depth, pad_mode):
    """What one query costs: the groups' sponge blocks, the levels and the injections."""
    return sum(max(1, (c + pad_mode + 3) // 4) for c in cols) + depth + len(cols) - 1


def tampers(rows, index, path, max_rows):
    """Every tampered opening of the tests, as (label, rows, index, path): one word of each group's row, one sibling, the
    index."""
    out = []
    for g in range(len(rows)):
        bad = [r.copy() for r in rows]
        bad[g][bad[g].shape[0] // 2] = np.array([BAD + g, 0, 0, 0], dtype=np.uint64)
        out.append(("row %d" % g, bad, index, path))
    bad = np.array(path, dtype=np.uint64, copy=True)
    bad[bad.shape[0] // 2, 0] = np.array([BAD + 99, 0, 0, 0], dtype=np.uint64)
    out.append(("sibling", rows, index, bad))
    out.append(("index", rows, (index + 1) % max_rows, path))
    return out


# ---- the golden file -------------------------------------------------------------------------------------------------
# (arity, heights, columns, pad_mode, opened index, first generator-B element)
GOLDEN_CASES = [(2, (8, 4, 1), (5, 3, 2), 1, 5, 19000), (4, (16, 4), (4, 1), 0, 11, 19100), (3, (9, 1), (1, 6), 1, 8, 19200)]


def golden_groups(oracle, heights, cols, first):
    """The fixture's matrices, row-major, from generator B: group after group."""
    out = []
    for h, c in zip(heights, cols):
        out.append(oracle.gen_b(first, h * c).reshape(h, c, 4))
        first += h * c
    return out


def _hex(a):
    return ["%064x" % oracle_lib.int_of(r) for r in np.asarray(a).reshape(-1, 4)]


unhex = M.unhex


def golden(oracle=None):
    """The three fixture shapes with tree, root, one opening and its tampered roots, from this repository's own oracle."""
    oracle = oracle or oracle_lib.load()
    cases = []
    for arity, heights, cols, pad_mode, index, first in GOLDEN_CASES:
        groups = golden_groups(oracle, heights, cols, first)
        tree, root = commit(oracle, groups, arity, pad_mode=pad_mode)
        rows, path = open_rows(groups, index), open_paths(tree, heights[0], arity, [index])[0]
        assert verify(oracle, rows, heights, index, path, arity, pad_mode=pad_mode).tobytes() == root.tobytes()
        bad = [{"what": what, "root": _hex(verify(oracle, r, heights, i, p, arity, pad_mode=pad_mode))[0]}
               for what, r, i, p in tampers(rows, index, path, heights[0])]
        cases.append({"arity": arity, "heights": list(heights), "cols": list(cols), "pad_mode": pad_mode,
                      "capacity_mont": "%064x" % CAP, "tag_mont": "%064x" % TAG[arity], "inject_tag_mont": "%064x" % INJECT,
                      "out_idx": 1, "matrices_row_major": [_hex(g) for g in groups], "tree": _hex(tree), "root": _hex(root)[0],
                      "opening": {"index": index, "rows": [_hex(r) for r in rows], "path": _hex(path)}, "tampered": bad})
    return {"layout": "scalars as 64 hex digits of the in-memory word (Montgomery limbs, little-endian limbs joined)",
            "cases": cases}
