"""CPU tier: the model of the matrix commitments (tests/matrix_model.py) and its golden file.  The golden file is what
tools/gen_matrix_kat.py writes today, and every opening the model assembles verifies against the committed root with the
oracle's own path verification."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import matrix_model as M  # noqa: E402
from gpu_common import CAP, TAG  # noqa: E402


def test_golden_file_is_current(oracle):
    import gen_matrix_kat
    with open(gen_matrix_kat.OUT) as f:
        committed = f.read()
    assert committed == json.dumps(M.golden(oracle), indent=1) + "\n", "stale: python tools/gen_matrix_kat.py"
    assert len(committed) < 32 * 1024
    cases = json.loads(committed)["cases"]
    assert [(c["n_rows"], c["n_cols"], c["pad_mode"], c["arity"]) for c in cases] == [g[:4] for g in M.GOLDEN_CASES]


def test_planes_round_trip_and_gap():
    m = np.arange(5 * 3 * 4, dtype=np.uint64).reshape(5, 3, 4)
    planes = M.planes_of(m, 9)
    assert planes.shape == (3, 9, 4) and (planes[:, 5:] == M.SENTINEL).all()
    assert (planes[2, 4] == m[4, 2]).all() and M.matrix_of(planes, 5).tobytes() == m.tobytes()
    assert M.planes_of(m).shape == (3, 5, 4)


@pytest.mark.parametrize("n_rows,n_cols,arity,padded", [(2, 1, 2, False), (5, 5, 2, True), (9, 6, 3, False), (10, 3, 4, True),
                                                        (17, 4, 3, True)])
def test_openings_verify_with_the_oracle(oracle, n_rows, n_cols, arity, padded):
    m = oracle.gen_b(13000 + n_rows, n_rows * n_cols).reshape(n_rows, n_cols, 4)
    depth = M.depth_of(n_rows, arity)
    pad = oracle.merkle_empty_digests(arity, depth, 5, TAG[arity]) if padded else None
    digests, tree, root = M.commit(oracle, m, arity, pad_mode=n_cols % 2, pad=pad)
    assert digests.shape == (n_rows, 4) and depth == len(oracle.merkle_tree(digests.reshape(-1), arity, TAG[arity], 1, pad))
    idx = list(range(n_rows)) + [n_rows, n_rows + 5]
    rows, paths = M.open_rows(m, digests, tree, arity, idx, pad)
    assert paths.shape == (len(idx), depth, arity - 1, 4)
    for t in range(n_rows):
        assert rows[t].tobytes() == m[t].tobytes()
        assert M.verify(oracle, rows[t], t, paths[t], arity, pad_mode=n_cols % 2).tobytes() == root.tobytes(), t
    assert not rows[n_rows:].any() and not paths[n_rows:].any()          # an index >= n_rows: zeros
    # a changed scalar, a changed sibling and a wrong index each give another root
    bad = rows[1].copy()
    bad[0, 0] ^= np.uint64(1)
    assert M.verify(oracle, bad, 1, paths[1], arity, pad_mode=n_cols % 2).tobytes() != root.tobytes()
    badp = paths[1].copy()
    badp[depth - 1, 0, 1] ^= np.uint64(1)
    assert M.verify(oracle, rows[1], 1, badp, arity, pad_mode=n_cols % 2).tobytes() != root.tobytes()
    assert M.verify(oracle, rows[1], 0, paths[1], arity, pad_mode=n_cols % 2).tobytes() != root.tobytes()
    assert CAP != 0
