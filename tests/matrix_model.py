"""Model of the column-major matrix commitments (hades252_matrix_*): nothing but a transpose, the C oracle's sponge and
Merkle tree (tests/oracle_lib.py) and the assembly of openings.  The convention is unpinned, like the sponge and the tree it
is made of: parity is pinned to this repository's oracle only."""
import numpy as np

import oracle_lib
from gpu_common import CAP, TAG

SENTINEL = 0xABCDEF0123456789


def planes_of(matrix, plane_stride=None, gap=SENTINEL):
    """Row-major [n_rows, n_cols, 4] -> column-major planes [n_cols, plane_stride, 4]; rows n_rows .. plane_stride - 1 of
    every plane (the gap between two columns) hold `gap` in every limb."""
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    n_rows, n_cols = m.shape[0], m.shape[1]
    stride = n_rows if plane_stride is None else plane_stride
    planes = np.full((n_cols, stride, 4), gap, dtype=np.uint64)
    planes[:, :n_rows] = m.transpose(1, 0, 2)
    return planes


def matrix_of(planes, n_rows):
    """Column-major planes -> the row-major matrix [n_rows, n_cols, 4]."""
    return np.ascontiguousarray(np.asarray(planes)[:, :n_rows].transpose(1, 0, 2))


def row_digests(oracle, matrix, cap=CAP, pad_mode=1):
    """leaf[r] = the oracle's sponge of row r, uint64 [n_rows, 4]."""
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    return oracle.sponge(m.reshape(-1), m.shape[1], cap, pad_mode).reshape(m.shape[0], 4)


def commit(oracle, matrix, arity, cap=CAP, pad_mode=1, tag=None, out_idx=1, pad=None):
    """(digests [n_rows, 4], tree [nodes, 4] in the layout of hades252_merkle_build_dev, root [4])."""
    digests = row_digests(oracle, matrix, cap, pad_mode)
    levels = oracle.merkle_tree(digests.reshape(-1), arity, TAG[arity] if tag is None else tag, out_idx, pad)
    tree = np.concatenate(levels).reshape(-1, 4)
    return digests, tree, tree[-1].copy()


def depth_of(n_rows, arity):
    d = 0
    while n_rows > 1:
        n_rows = -(-n_rows // arity)
        d += 1
    return d


def open_rows(matrix, digests, tree, arity, indices, pad=None):
    """(rows [q, n_cols, 4], paths [q, depth, arity - 1, 4]): row r and, level by level, the arity - 1 siblings of its path
    node in child order with the node's own position skipped; a sibling position past the end of level l is pad[l] (None:
    zero); an index >= n_rows gives zeros."""
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    n_rows, n_cols = m.shape[0], m.shape[1]
    depth = depth_of(n_rows, arity)
    levels, cur, off = [np.asarray(digests).reshape(-1, 4)], n_rows, 0
    tree = np.asarray(tree).reshape(-1, 4)
    for _ in range(depth - 1):
        cur = -(-cur // arity)
        levels.append(tree[off:off + cur])
        off += cur
    rows = np.zeros((len(indices), n_cols, 4), dtype=np.uint64)
    paths = np.zeros((len(indices), depth, arity - 1, 4), dtype=np.uint64)
    for t, r in enumerate(int(i) for i in indices):
        if r >= n_rows:
            continue
        rows[t] = m[r]
        node = r
        for l in range(depth):
            first, pos = node - node % arity, node % arity
            sibs = [first + s for s in range(arity) if s != pos]
            for s, j in enumerate(sibs):
                if j < levels[l].shape[0]:
                    paths[t, l, s] = levels[l][j]
                elif pad is not None:
                    paths[t, l, s] = np.asarray(pad).reshape(-1, 4)[l]
            node //= arity
    return rows, paths


def verify(oracle, row, index, path, arity, cap=CAP, pad_mode=1, tag=None, out_idx=1):
    """The root recomputed from one opened row, by the oracle alone."""
    row = np.ascontiguousarray(row, dtype=np.uint64)
    leaf = oracle.sponge(row.reshape(-1), row.shape[0], cap, pad_mode)
    return oracle.merkle_verify_path(leaf, int(index), path, arity, TAG[arity] if tag is None else tag, out_idx)


# ---- the golden file -------------------------------------------------------------------------------------------------
# (n_rows, n_cols, pad_mode, arity, opened row, first generator-B element)
GOLDEN_CASES = [(2, 1, 1, 2, 1, 12000), (5, 5, 0, 2, 3, 12100), (9, 6, 1, 3, 8, 12200)]


def _hex(a):
    return ["%064x" % oracle_lib.int_of(r) for r in np.asarray(a).reshape(-1, 4)]


def unhex(hexes):
    assert not isinstance(hexes, str), "a list of scalars, not one string"
    return np.array([oracle_lib.limbs_of(int(h, 16)) for h in hexes], dtype=np.uint64).reshape(-1, 4)


def golden(oracle=None):
    """Three small matrices with digests, tree, root and one opening each, from this repository's own oracle."""
    oracle = oracle or oracle_lib.load()
    cases = []
    for n_rows, n_cols, pad_mode, arity, opened, first in GOLDEN_CASES:
        m = oracle.gen_b(first, n_rows * n_cols).reshape(n_rows, n_cols, 4)
        digests, tree, root = commit(oracle, m, arity, pad_mode=pad_mode)
        rows, paths = open_rows(m, digests, tree, arity, [opened])
        cases.append({"n_rows": n_rows, "n_cols": n_cols, "pad_mode": pad_mode, "arity": arity,
                      "capacity_mont": "%064x" % CAP, "tag_mont": "%064x" % TAG[arity], "out_idx": 1,
                      "matrix_row_major": _hex(m), "digests": _hex(digests), "tree": _hex(tree), "root": _hex(root)[0],
                      "opening": {"index": opened, "row": _hex(rows[0]), "path": _hex(paths[0])}})
    return {"layout": "scalars as 64 hex digits of the in-memory word (Montgomery limbs, little-endian limbs joined)",
            "cases": cases}
