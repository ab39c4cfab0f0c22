"""GPU tier, row f12 (beyond SURVEY section 8): commitments to a matrix stored column by column (hades252_matrix_row_digests /
_commit / _open / _verify) against the model (tests/matrix_model.py: a transpose over the C oracle's sponge and Merkle tree)
and the library's own row-major calls.  Exact, byte for byte, everywhere; at most 2^14 + 3 rows per case."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matrix_model as M  # noqa: E402
from gpu_common import CAP, EDGE_VALUES, TAG  # noqa: E402
from oracle_lib import limbs_of  # noqa: E402

pytestmark = pytest.mark.gpu

N_BIG = (1 << 14) + 3
SENTINEL = M.SENTINEL
GUARD = 3                                  # sentinel digests on each side of an output


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "matrix_kat.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def pool(oracle):
    """1000 x 9 generator-B scalars, row-major, and the oracle's row digests of its leading columns per (n_cols, pad_mode);
    never written."""
    m = oracle.gen_b(16000, 1000 * 9).reshape(1000, 9, 4)
    m.setflags(write=False)
    digests = {}

    def leaves(n_cols, pad_mode):
        if (n_cols, pad_mode) not in digests:
            d = M.row_digests(oracle, np.ascontiguousarray(m[:, :n_cols]), CAP, pad_mode)
            d.setflags(write=False)
            digests[(n_cols, pad_mode)] = d
        return digests[(n_cols, pad_mode)]

    return m, leaves


def _p(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


def _cap():
    return (ctypes.c_uint64 * 4)(*limbs_of(CAP))


def _tag(arity):
    return (ctypes.c_uint64 * 4)(*limbs_of(TAG[arity]))


def _guarded(n):
    """An output of n digests between GUARD sentinel digests: (whole array, pointer to the interior)."""
    big = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
    return big, _p(big, GUARD * 32)


def _intact(big, n):
    assert (big[:GUARD] == SENTINEL).all() and (big[GUARD + n:] == SENTINEL).all(), "a digest outside the output was written"
    return big[GUARD:GUARD + n]


def _row_digests(hades_lib, planes, n_rows, pad_mode):
    big, ptr = _guarded(n_rows)
    assert hades_lib.hades252_matrix_row_digests(_p(planes), n_rows, planes.shape[0], planes.shape[1], _cap(), pad_mode, ptr) == 0
    return _intact(big, n_rows)


# ---- 1. known answers --------------------------------------------------------------------------------------------------
def test_kats_one_call_each(hades_lib, H, golden):
    for c in golden:
        m = M.unhex(c["matrix_row_major"]).reshape(c["n_rows"], c["n_cols"], 4)
        cap, tag, arity, pad_mode = int(c["capacity_mont"], 16), int(c["tag_mont"], 16), c["arity"], c["pad_mode"]
        planes = M.planes_of(m)
        assert H.matrix_row_digests_host(planes, cap, pad_mode).tobytes() == M.unhex(c["digests"]).tobytes()
        digests, tree, root = H.matrix_commit_host(planes, cap, arity, tag, pad_mode, c["out_idx"])
        assert digests.tobytes() == M.unhex(c["digests"]).tobytes() and tree.tobytes() == M.unhex(c["tree"]).tobytes()
        assert root.tobytes() == M.unhex([c["root"]]).tobytes()
        rows, paths = H.matrix_open_host(planes, digests, tree, arity, [c["opening"]["index"]])
        assert rows.tobytes() == M.unhex(c["opening"]["row"]).tobytes()
        assert paths.tobytes() == M.unhex(c["opening"]["path"]).tobytes()
        roots = H.matrix_verify_host(rows, [c["opening"]["index"]], paths, arity, cap, tag, pad_mode, c["out_idx"])
        assert roots.tobytes() == M.unhex([c["root"]]).tobytes()


# ---- 2. shapes and neighbours ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_shapes_and_neighbours(hades_lib, pool, n_rows):
    """Wave and block edges in the rows; block edges in the columns, and where the pad scalar opens a new block; a gap of
    seven sentinel scalars between the planes."""
    m, leaves = pool
    for n_cols in (1, 3, 4, 5, 8, 9):
        sub = np.ascontiguousarray(m[:n_rows, :n_cols])
        for pad_mode in (0, 1):
            want = leaves(n_cols, pad_mode)[:n_rows]
            for stride in (n_rows, n_rows + 7):
                got = _row_digests(hades_lib, M.planes_of(sub, stride), n_rows, pad_mode)
                assert got.tobytes() == want.tobytes(), (n_cols, pad_mode, stride)


# ---- 3. edge values ----------------------------------------------------------------------------------------------------
def test_edge_values_in_every_column_position(hades_lib, oracle, pool):
    """gpu_common.EDGE_VALUES (as in-memory words) in the rows at lanes 0, 63, 64, 255, 256 and in the last row, every value in
    every column position mod 4 over the four matrices; generator-B fill elsewhere."""
    n_rows, n_cols = 259, 9
    special = [0, 63, 64, 255, 256, n_rows - 1]
    seen = set()
    for shift in range(4):
        m = pool[0][:n_rows].copy()
        for i, r in enumerate(special):
            for c in range(n_cols):
                # row i of matrix `shift` holds nine consecutive catalogue entries from entry i + 6 * shift on: the 24 starts
                # cover every residue mod 14, so every entry meets every column (hence every position mod 4)
                v = (i + len(special) * shift + c) % len(EDGE_VALUES)
                m[r, c] = np.array(limbs_of(EDGE_VALUES[v]), dtype=np.uint64)
                seen.add((v, c % 4))
        pad_mode = shift % 2
        got = _row_digests(hades_lib, M.planes_of(m, n_rows + shift), n_rows, pad_mode)
        want = M.row_digests(oracle, m, CAP, pad_mode)
        bad = [r for r in special if got[r].tobytes() != want[r].tobytes()]
        assert not bad, bad
        assert got.tobytes() == want.tobytes()
    assert len(seen) == 4 * len(EDGE_VALUES)


# ---- 4. commit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arity", [2, 3, 4])
def test_commit(hades_lib, oracle, pool, arity):
    m, leaves = pool
    n_cols = 5
    for n_rows in (2, 5, 257, 1000):
        depth = M.depth_of(n_rows, arity)
        planes = M.planes_of(np.ascontiguousarray(m[:n_rows, :n_cols]), n_rows + 1)
        for pad in (None, oracle.merkle_empty_digests(arity, depth, 11, TAG[arity])):
            want_d = leaves(n_cols, 1)[:n_rows]
            want_t = np.concatenate(oracle.merkle_tree(want_d.reshape(-1), arity, TAG[arity], 1, pad)).reshape(-1, 4)
            nodes = want_t.shape[0]
            assert nodes * 32 == hades_lib.hades252_merkle_tree_bytes(n_rows, arity)

            def commit(with_digests, with_tree):
                d_big, d_ptr = _guarded(n_rows)
                t_big, t_ptr = _guarded(nodes)
                root = np.full(4 + 2, SENTINEL, dtype=np.uint64)
                rc = hades_lib.hades252_matrix_commit(_p(planes), n_rows, n_cols, planes.shape[1], _cap(), 1, arity, _tag(arity), 1,
                                                      None if pad is None else _p(pad), d_ptr if with_digests else None,
                                                      t_ptr if with_tree else None, _p(root, 8))
                assert rc == 0 and root[0] == SENTINEL and root[5] == SENTINEL
                d, t = _intact(d_big, n_rows), _intact(t_big, nodes)
                assert with_digests or (d == SENTINEL).all()
                assert with_tree or (t == SENTINEL).all()
                return d, t, root[1:5]

            d, t, root = commit(True, True)
            assert d.tobytes() == want_d.tobytes() and t.tobytes() == want_t.tobytes(), (n_rows, pad is None)
            assert root.tobytes() == want_t[-1].tobytes()
            d, t, r2 = commit(False, True)
            assert t.tobytes() == want_t.tobytes() and r2.tobytes() == root.tobytes()
            d, t, r3 = commit(True, False)
            assert d.tobytes() == want_d.tobytes() and r3.tobytes() == root.tobytes()
            assert commit(False, False)[2].tobytes() == root.tobytes()


def test_a_failing_copy_fails_the_commit_leaves_the_root_alone_and_loses_no_pipe(hades_lib, H, oracle, pool):
    """hades252_fault_inject returns an error INSTEAD of making the call: no GPU work is disturbed.  "memcpy:1" is the 2-D
    copy of the first tile (no padding table travels in front of it)."""
    n_rows, n_cols = 300, 5
    sub = np.ascontiguousarray(pool[0][:n_rows, :n_cols])
    planes = M.planes_of(sub)

    def commit(root):
        return hades_lib.hades252_matrix_commit(_p(planes), n_rows, n_cols, planes.shape[1], _cap(), 1, 2, _tag(2), 1, None, None,
                                                None, _p(root))

    H.trim()                                                              # the pool holds this call's pipe and nothing else
    first = np.zeros(4, dtype=np.uint64)
    assert commit(first) == 0
    held = H.pool_bytes()
    assert held > 0
    root = np.full(4, SENTINEL, dtype=np.uint64)
    H.fault_inject("memcpy:1")
    try:
        assert commit(root) == -2                                         # HADES252_ERR_HIP
    finally:
        H.fault_inject(None)
    assert (root == SENTINEL).all()
    assert commit(root) == 0
    assert root.tobytes() == first.tobytes() == M.commit(oracle, sub, 2)[2].tobytes()
    assert H.pool_bytes() == held


# ---- 5. several chunks -------------------------------------------------------------------------------------------------
_CHUNK_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from hades252_amd import build, strategy as H
build.build(verbose=False)
assert os.environ["HADES252_TEST_MATRIX_CHUNK_ROWS"] == "256"
src, dst, cap, tag = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
planes = np.fromfile(src, dtype=np.uint64).reshape(5, 1003, 4)
d, t, r = H.matrix_commit_host(planes, cap, 3, tag, 1, n_rows=1000)
d0 = H.matrix_row_digests_host(planes, cap, 0, n_rows=1000)
np.concatenate([d.reshape(-1), t.reshape(-1), r, d0.reshape(-1)]).tofile(dst)
print("CHUNKED", d.shape[0], t.shape[0])
"""


def test_four_chunks_give_the_single_chunk_bytes(hades_lib, H, pool, tmp_path):
    """HADES252_TEST_MATRIX_CHUNK_ROWS = 256 (read once by the library, hence a child process): 1000 rows are four chunks,
    the last one ragged (232 rows), and each of the two chunk buffers is used twice."""
    m, leaves = pool
    planes = M.planes_of(np.ascontiguousarray(m[:, :5]), 1003)
    d, t, r = H.matrix_commit_host(planes, CAP, 3, TAG[3], 1, n_rows=1000)
    d0 = H.matrix_row_digests_host(planes, CAP, 0, n_rows=1000)
    assert d.tobytes() == leaves(5, 1).tobytes() and d0.tobytes() == leaves(5, 0).tobytes()
    single = np.concatenate([d.reshape(-1), t.reshape(-1), r, d0.reshape(-1)])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    planes.tofile(src)
    env = dict(os.environ, HADES252_TEST_MATRIX_CHUNK_ROWS="256")
    run = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, str(src), str(dst), str(CAP), str(TAG[3])], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "CHUNKED 1000 %d" % t.shape[0] in run.stdout, run.stdout[-1500:] + run.stderr[-3000:]
    assert np.fromfile(dst, dtype=np.uint64).tobytes() == single.tobytes()


# ---- 6. open and verify ------------------------------------------------------------------------------------------------
def test_open_and_verify(hades_lib, H, oracle, pool):
    m, _ = pool
    arity, n_cols = 4, 6
    sub = np.ascontiguousarray(m[:, :n_cols])
    planes = M.planes_of(sub, 1000 + 7)
    digests, tree, root = H.matrix_commit_host(planes, CAP, arity, TAG[arity], n_rows=1000)
    idx = [0, 999, 500, 500, 3]
    rows, paths = H.matrix_open_host(planes, digests, tree, arity, idx, n_rows=1000)
    assert rows.tobytes() == sub[idx].tobytes()
    want_rows, want_paths = M.open_rows(sub, digests, tree, arity, idx)
    assert paths.tobytes() == want_paths.tobytes()
    roots = H.matrix_verify_host(rows, idx, paths, arity, CAP, TAG[arity])
    assert roots.tobytes() == np.tile(root, len(idx)).tobytes()
    assert M.verify(oracle, rows[1], 999, paths[1], arity).tobytes() == root.tobytes()
    # a changed row scalar, a changed path digest and a wrong index each give a different root -- and only there
    bad_rows, bad_paths, bad_idx = rows.copy(), paths.copy(), list(idx)
    bad_rows[1, n_cols - 1, 0] ^= np.uint64(1)
    assert bad_rows[1, n_cols - 1, 0] != rows[1, n_cols - 1, 0]
    bad_paths[2, paths.shape[1] - 1, 1, 3] ^= np.uint64(1 << 20)
    bad_idx[4] = 2
    for r, i, p, where in ((bad_rows, idx, paths, 1), (rows, idx, bad_paths, 2), (rows, bad_idx, paths, 4)):
        got = H.matrix_verify_host(r, i, p, arity, CAP, TAG[arity])
        for t in range(len(idx)):
            assert (got[t].tobytes() == root.tobytes()) == (t != where), (where, t)
    # through the C entry point with guarded outputs
    big, ptr = _guarded(len(idx))
    ii = np.array(idx, dtype=np.uint64)
    assert hades_lib.hades252_matrix_verify(_p(rows), n_cols, _p(ii), _p(paths), len(idx), paths.shape[1], arity, _cap(), 1,
                                            _tag(arity), 1, ptr) == 0
    assert _intact(big, len(idx)).tobytes() == roots.tobytes()


# ---- 7. against the library's own calls --------------------------------------------------------------------------------
def test_big_matrix_against_the_row_major_calls(hades_lib, H, oracle):
    n_cols, arity = 7, 2
    m = oracle.gen_b(17000, N_BIG * n_cols).reshape(N_BIG, n_cols, 4)
    planes = M.planes_of(m)
    digests, tree, root = H.matrix_commit_host(planes, CAP, arity, TAG[arity])
    assert digests.tobytes() == H.sponge_hash_host(m.reshape(-1), N_BIG, n_cols, CAP, 1).tobytes()
    assert digests[:100].tobytes() == M.row_digests(oracle, m[:100], CAP, 1).tobytes()
    assert root.tobytes() == H.merkle_root_host(digests.reshape(-1), arity, TAG[arity]).tobytes()
    assert tree[-1].tobytes() == root.tobytes() and tree.shape[0] * 32 == hades_lib.hades252_merkle_tree_bytes(N_BIG, arity)
    assert H.matrix_row_digests_host(planes, CAP, 0).tobytes() == H.sponge_hash_host(m.reshape(-1), N_BIG, n_cols, CAP, 0).tobytes()
