"""GPU tier, row f13 (beyond SURVEY section 8): streaming commitments to a matrix stored column by column (hades252_matstream_open /
_absorb / _cols / _digests / _commit / _close) against the one-shot calls of f12 on the concatenated matrix, the model
(tests/matrix_stream_model.py: the C oracle's permutation and additions; tests/matrix_model.py: its sponge and tree) and the
library's own row-major calls.  Exact, byte for byte, everywhere; at most 2^14 + 3 rows per case; outputs sit between
sentinel digests."""
import contextlib
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
import matrix_stream_model as MS  # noqa: E402
from gpu_common import CAP, EDGE_VALUES, TAG  # noqa: E402
from oracle_lib import P, limbs_of  # noqa: E402

pytestmark = pytest.mark.gpu

N_BIG = (1 << 14) + 3
SENTINEL = M.SENTINEL
GUARD = 3                                  # sentinel digests on each side of an output
INVALID, ERR_HIP = -1, -2


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


def _limbs(v):
    return (ctypes.c_uint64 * 4)(*limbs_of(v))


def _guarded(n):
    """An output of n digests between GUARD sentinel digests: (whole array, pointer to the interior)."""
    big = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
    return big, _p(big, GUARD * 32)


def _intact(big, n):
    assert (big[:GUARD] == SENTINEL).all() and (big[GUARD + n:] == SENTINEL).all(), "a digest outside the output was written"
    return big[GUARD:GUARD + n]


@contextlib.contextmanager
def _stream(lib, n_rows, cap=CAP):
    h = ctypes.c_void_p()
    assert lib.hades252_matstream_open(ctypes.byref(h), n_rows, _limbs(cap)) == 0 and h.value
    try:
        yield h
    finally:
        assert lib.hades252_matstream_close(h) == 0


def _absorb(lib, h, matrix, groups, strides=None):
    """The columns of row-major `matrix` in `groups`, group i from planes of stride strides[i % len] (a gap of sentinel scalars
    between the planes where the stride exceeds the row count)."""
    n_rows = matrix.shape[0]
    for i, part in enumerate(MS.split(matrix, groups)):
        stride = n_rows if strides is None else strides[i % len(strides)]
        planes = M.planes_of(part, stride)
        assert lib.hades252_matstream_absorb(h, _p(planes), part.shape[1], stride) == 0, (groups, i)


def _cols(lib, h):
    n = ctypes.c_uint64(1 << 63)
    assert lib.hades252_matstream_cols(h, ctypes.byref(n)) == 0
    return n.value


def _digests(lib, h, n_rows, pad_mode):
    big, ptr = _guarded(n_rows)
    assert lib.hades252_matstream_digests(h, pad_mode, ptr) == 0
    return _intact(big, n_rows)


def _one_shot_digests(lib, matrix, pad_mode):
    planes, n_rows = M.planes_of(matrix), matrix.shape[0]
    big, ptr = _guarded(n_rows)
    assert lib.hades252_matrix_row_digests(_p(planes), n_rows, planes.shape[0], planes.shape[1], _limbs(CAP), pad_mode, ptr) == 0
    return _intact(big, n_rows)


# ---- 1. known answers --------------------------------------------------------------------------------------------------
def test_kats_column_by_column_and_in_one_call(H, golden):
    for c in golden:
        m = M.unhex(c["matrix_row_major"]).reshape(c["n_rows"], c["n_cols"], 4)
        cap, tag, arity, pad_mode = int(c["capacity_mont"], 16), int(c["tag_mont"], 16), c["arity"], c["pad_mode"]
        planes = M.planes_of(m)
        for groups in ([1] * c["n_cols"], [c["n_cols"]]):
            with H.MatrixStream(c["n_rows"], cap) as ms:
                j = 0
                for g in groups:
                    assert ms.absorb(np.ascontiguousarray(planes[j:j + g])) is ms
                    j += g
                assert ms.cols == c["n_cols"]
                assert ms.digests(pad_mode).tobytes() == M.unhex(c["digests"]).tobytes()
                digests, tree, root = ms.commit(arity, tag, pad_mode, c["out_idx"])
                assert digests.tobytes() == M.unhex(c["digests"]).tobytes() and tree.tobytes() == M.unhex(c["tree"]).tobytes()
                assert root.tobytes() == M.unhex([c["root"]]).tobytes()
                d2, t2, r2 = ms.commit(arity, tag, pad_mode, c["out_idx"], want_digests=False, want_tree=False)
                assert d2 is None and t2 is None and r2.tobytes() == root.tobytes()


# ---- 2. every split ----------------------------------------------------------------------------------------------------
def test_every_split_of_six_columns(hades_lib, oracle, pool):
    n_rows, total = 65, 6
    m = np.ascontiguousarray(pool[0][:n_rows, :total])
    model = MS.Stream(oracle, n_rows).absorb(m)
    want = {}
    for pad_mode in (0, 1):
        want[pad_mode] = _one_shot_digests(hades_lib, m, pad_mode).copy()
        assert want[pad_mode].tobytes() == model.digests(pad_mode).tobytes() == pool[1](total, pad_mode)[:n_rows].tobytes()
    comps = MS.compositions(total)
    assert len(comps) == 32
    for groups in comps:
        with _stream(hades_lib, n_rows) as h:
            _absorb(hades_lib, h, m, groups)
            assert _cols(hades_lib, h) == total
            for pad_mode in (0, 1):
                assert _digests(hades_lib, h, n_rows, pad_mode).tobytes() == want[pad_mode].tobytes(), (groups, pad_mode)


# ---- 3. prefixes -------------------------------------------------------------------------------------------------------
def test_every_prefix_can_be_finished_and_absorbing_continues(hades_lib, oracle, pool):
    """The finish does not write the state: after every column both paddings are asked for, and the next column still lands
    on the state the previous ones left."""
    n_rows, total = 259, 9
    m = np.ascontiguousarray(pool[0][:n_rows, :total])
    model = MS.Stream(oracle, n_rows)
    with _stream(hades_lib, n_rows) as h:
        for j in range(total):
            col = np.ascontiguousarray(m[:, j:j + 1])
            _absorb(hades_lib, h, col, (1,))
            model.absorb(col)
            assert _cols(hades_lib, h) == j + 1
            for pad_mode in (0, 1, 1, 0):
                got = _digests(hades_lib, h, n_rows, pad_mode)
                assert got.tobytes() == model.digests(pad_mode).tobytes() == pool[1](j + 1, pad_mode)[:n_rows].tobytes(), (j, pad_mode)


# ---- 4. shapes and neighbours ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_shapes_and_neighbours(hades_lib, pool, n_rows):
    """Wave and block edges in the rows; block edges in the columns and in the groups (a group that ends inside a block, one
    that starts there), and where the pad scalar opens a new block; another plane stride for every group, with a gap of seven
    sentinel scalars between the planes."""
    m, leaves = pool
    for total in (1, 3, 4, 5, 8, 9):
        sub = np.ascontiguousarray(m[:n_rows, :total])
        for groups in ((total,), (1, total - 1), (3, total - 3)):
            if min(groups) < 1:
                continue
            for strides in ((n_rows, n_rows + 7), (n_rows + 7, n_rows)):
                with _stream(hades_lib, n_rows) as h:
                    _absorb(hades_lib, h, sub, groups, strides)
                    for pad_mode in (0, 1):
                        got = _digests(hades_lib, h, n_rows, pad_mode)
                        assert got.tobytes() == leaves(total, pad_mode)[:n_rows].tobytes(), (total, groups, strides, pad_mode)


# ---- 5. edge values ----------------------------------------------------------------------------------------------------
def test_edge_values_in_every_column_position_head_body_and_tail(hades_lib, oracle, pool):
    """gpu_common.EDGE_VALUES (as in-memory words) in the rows at lanes 0, 63, 64, 255, 256 and in the last row, every value in
    every column position mod 4 over the four matrices; generator-B fill elsewhere.  Every matrix goes through four splits,
    which put the columns of every position mod 4 into a body (whole blocks), those of positions 1 .. 3 into a head (a group
    that completes an open block) and those of positions 0 .. 2 into a tail (a group's last, partial block) -- a head never
    holds position 0 and a tail never position 3."""
    n_rows, n_cols = 259, 9
    special = [0, 63, 64, 255, 256, n_rows - 1]
    # columns by role -- (9,): body 0-7, tail 8; (1, 8): tail 0, head 1-3, body 4-7, tail 8; (2, 7): tail 0-1, head 2-3, body 4-7,
    # tail 8; (3, 2, 4): tail 0-2, head 3, tail 4, head 5-7, tail 8
    splits = [(9,), (1, 8), (2, 7), (3, 2, 4)]
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
        want = M.row_digests(oracle, m, CAP, pad_mode)
        for groups in splits:
            with _stream(hades_lib, n_rows) as h:
                _absorb(hades_lib, h, m, groups, (n_rows + shift,))
                got = _digests(hades_lib, h, n_rows, pad_mode)
            bad = [r for r in special if got[r].tobytes() != want[r].tobytes()]
            assert not bad, (groups, bad)
            assert got.tobytes() == want.tobytes(), groups
    assert len(seen) == 4 * len(EDGE_VALUES)


# ---- 6. commit ---------------------------------------------------------------------------------------------------------
def _commit(lib, h, n_rows, nodes, arity, pad, with_digests, with_tree, pad_mode=1):
    d_big, d_ptr = _guarded(n_rows)
    t_big, t_ptr = _guarded(nodes)
    root = np.full(4 + 2, SENTINEL, dtype=np.uint64)
    rc = lib.hades252_matstream_commit(h, pad_mode, arity, _limbs(TAG[arity]), 1, None if pad is None else _p(pad),
                                       d_ptr if with_digests else None, t_ptr if with_tree else None, _p(root, 8))
    assert rc == 0 and root[0] == SENTINEL and root[5] == SENTINEL
    d, t = _intact(d_big, n_rows), _intact(t_big, nodes)
    assert with_digests or (d == SENTINEL).all()
    assert with_tree or (t == SENTINEL).all()
    return d, t, root[1:5]


@pytest.mark.parametrize("arity", [2, 3, 4])
def test_commit_equals_the_one_shot_commit(hades_lib, H, oracle, pool, arity):
    m, leaves = pool
    n_cols = 5
    for n_rows in (2, 257, 1000):
        depth = M.depth_of(n_rows, arity)
        sub = np.ascontiguousarray(m[:n_rows, :n_cols])
        with _stream(hades_lib, n_rows) as h:
            _absorb(hades_lib, h, sub, (2, 3), (n_rows + 1, n_rows))
            for pad in (None, oracle.merkle_empty_digests(arity, depth, 11, TAG[arity])):
                want_d, want_t, want_r = H.matrix_commit_host(M.planes_of(sub), CAP, arity, TAG[arity], 1, 1, pad)
                assert want_d.tobytes() == leaves(n_cols, 1)[:n_rows].tobytes()
                nodes = want_t.shape[0]
                d, t, root = _commit(hades_lib, h, n_rows, nodes, arity, pad, True, True)
                assert d.tobytes() == want_d.tobytes() and t.tobytes() == want_t.tobytes(), (n_rows, pad is None)
                assert root.tobytes() == want_r.tobytes() == want_t[-1].tobytes()
                d, t, r2 = _commit(hades_lib, h, n_rows, nodes, arity, pad, False, True)
                assert t.tobytes() == want_t.tobytes() and r2.tobytes() == root.tobytes()
                d, t, r3 = _commit(hades_lib, h, n_rows, nodes, arity, pad, True, False)
                assert d.tobytes() == want_d.tobytes() and r3.tobytes() == root.tobytes()
                assert _commit(hades_lib, h, n_rows, nodes, arity, pad, False, False)[2].tobytes() == root.tobytes()
            assert _cols(hades_lib, h) == n_cols


def test_one_row_has_digests_and_no_tree(hades_lib, pool):
    m, leaves = pool
    sub = np.ascontiguousarray(m[:1, :5])
    with _stream(hades_lib, 1) as h:
        _absorb(hades_lib, h, np.ascontiguousarray(sub[:, :3]), (3,))
        root = np.full(4, SENTINEL, dtype=np.uint64)
        for arity in (2, 3, 4):
            assert hades_lib.hades252_matstream_commit(h, 1, arity, _limbs(TAG[arity]), 1, None, None, None, _p(root)) == INVALID
        assert (root == SENTINEL).all()
        assert _digests(hades_lib, h, 1, 1).tobytes() == leaves(3, 1)[:1].tobytes()
        _absorb(hades_lib, h, np.ascontiguousarray(sub[:, 3:]), (2,))          # still usable
        assert _cols(hades_lib, h) == 5 and _digests(hades_lib, h, 1, 0).tobytes() == leaves(5, 0)[:1].tobytes()


def test_argument_rules_on_an_open_stream(hades_lib):
    import test_matrix_stream_abi
    test_matrix_stream_abi.rules_that_need_an_open_stream(hades_lib)


# ---- 7. tiling ---------------------------------------------------------------------------------------------------------
_TILE_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from hades252_amd import build, strategy as H
build.build(verbose=False)
assert os.environ["HADES252_TEST_MATRIX_CHUNK_ROWS"] == "256" and int(os.environ["HADES252_TEST_MATRIX_CHUNK_COLS"]) >= 1
src, dst, cap, tag = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
planes = np.fromfile(src, dtype=np.uint64).reshape(9, 1003, 4)
out = []
with H.MatrixStream(1000, cap) as ms:
    ms.absorb(np.ascontiguousarray(planes[:2]))
    out.append(ms.digests(1).reshape(-1))
    ms.absorb(np.ascontiguousarray(planes[2:]))
    d, t, r = ms.commit(3, tag, 1)
    out += [d.reshape(-1), t.reshape(-1), r, ms.digests(0).reshape(-1)]
    print("TILED", ms.cols, d.shape[0], t.shape[0])
np.concatenate(out).tofile(dst)
"""


@pytest.mark.parametrize("tile_cols", [1, 3, 4])
def test_tiles_give_the_untiled_bytes(hades_lib, H, pool, tmp_path, tile_cols):
    """HADES252_TEST_MATRIX_CHUNK_ROWS = 256 and HADES252_TEST_MATRIX_CHUNK_COLS (read once by the library, hence a child
    process): 1000 rows are four row chunks, the last one ragged (232 rows); 9 columns absorbed as (2, 7) are tiles of one
    column (adds only, or an add and a permutation), of three (partial blocks at both ends of a tile) and of four (the first
    tile of the second call is shortened to the two columns of the open block; then a whole block; then a tail)."""
    m, leaves = pool
    planes = M.planes_of(np.ascontiguousarray(m[:, :9]), 1003)
    out = []
    with H.MatrixStream(1000, CAP) as ms:
        ms.absorb(np.ascontiguousarray(planes[:2]))
        out.append(ms.digests(1).reshape(-1))
        ms.absorb(np.ascontiguousarray(planes[2:]))
        d, t, r = ms.commit(3, TAG[3], 1)
        out += [d.reshape(-1), t.reshape(-1), r, ms.digests(0).reshape(-1)]
    assert out[0].tobytes() == leaves(2, 1).tobytes() and d.tobytes() == leaves(9, 1).tobytes()
    assert out[4].tobytes() == leaves(9, 0).tobytes()
    untiled = np.concatenate(out)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    planes.tofile(src)
    env = dict(os.environ, HADES252_TEST_MATRIX_CHUNK_ROWS="256", HADES252_TEST_MATRIX_CHUNK_COLS=str(tile_cols))
    run = subprocess.run([sys.executable, "-c", _TILE_CHILD, str(src), str(dst), str(CAP), str(TAG[3])], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "TILED 9 1000 %d" % t.shape[0] in run.stdout, run.stdout[-1500:] + run.stderr[-3000:]
    assert np.fromfile(dst, dtype=np.uint64).tobytes() == untiled.tobytes()


# ---- 8. interleaving ---------------------------------------------------------------------------------------------------
def test_two_streams_a_one_shot_commit_and_a_trim_do_not_disturb_each_other(hades_lib, H, oracle, pool):
    m, leaves = pool
    cap_b = (CAP + 12345) % P
    a = np.ascontiguousarray(m[:257, :7])
    b = np.ascontiguousarray(m[300:300 + 65, 1:9])
    want_b = {pad: M.row_digests(oracle, b, cap_b, pad) for pad in (0, 1)}
    one_shot = np.ascontiguousarray(m[:100, :5])
    with _stream(hades_lib, 257) as ha, _stream(hades_lib, 65, cap_b) as hb:
        _absorb(hades_lib, ha, a[:, :3], (3,))
        _absorb(hades_lib, hb, b[:, :5], (5,))
        d, t, r = H.matrix_commit_host(M.planes_of(one_shot), CAP, 2, TAG[2])
        assert d.tobytes() == leaves(5, 1)[:100].tobytes()
        _absorb(hades_lib, ha, a[:, 3:4], (1,))
        assert _digests(hades_lib, hb, 65, 1).tobytes() == M.row_digests(oracle, np.ascontiguousarray(b[:, :5]), cap_b, 1).tobytes()
        H.trim()                                                          # the pool is emptied; what the streams hold stays
        assert H.pool_bytes() == 0
        _absorb(hades_lib, hb, b[:, 5:], (1, 2))
        _absorb(hades_lib, ha, a[:, 4:], (3,))
        assert _cols(hades_lib, ha) == 7 and _cols(hades_lib, hb) == 8
        for pad in (0, 1):
            assert _digests(hades_lib, ha, 257, pad).tobytes() == leaves(7, pad)[:257].tobytes()
            assert _digests(hades_lib, hb, 65, pad).tobytes() == want_b[pad].tobytes()
        d2, t2, r2 = H.matrix_commit_host(M.planes_of(one_shot), CAP, 2, TAG[2])
        assert d2.tobytes() == d.tobytes() and t2.tobytes() == t.tobytes() and r2.tobytes() == r.tobytes()


# ---- 9. simulated host errors ------------------------------------------------------------------------------------------
def test_a_failing_copy_poisons_the_stream_and_a_failing_allocation_opens_none(hades_lib, H, pool):
    """hades252_fault_inject returns an error INSTEAD of making the call: no GPU work is disturbed."""
    m, leaves = pool
    n_rows = 257
    sub = np.ascontiguousarray(m[:n_rows, :5])
    planes = M.planes_of(sub)
    h = ctypes.c_void_p()
    assert hades_lib.hades252_matstream_open(ctypes.byref(h), n_rows, _limbs(CAP)) == 0
    try:
        assert hades_lib.hades252_matstream_absorb(h, _p(planes), 2, n_rows) == 0
        H.fault_inject("memcpy:1")
        try:
            assert hades_lib.hades252_matstream_absorb(h, _p(planes, 2 * n_rows * 32), 3, n_rows) == ERR_HIP
        finally:
            H.fault_inject(None)
        out = np.full((n_rows, 4), SENTINEL, dtype=np.uint64)
        root = np.full(4, SENTINEL, dtype=np.uint64)
        assert hades_lib.hades252_matstream_absorb(h, _p(planes, 2 * n_rows * 32), 3, n_rows) == ERR_HIP
        assert hades_lib.hades252_matstream_absorb(h, None, 0, 0) == ERR_HIP
        assert hades_lib.hades252_matstream_digests(h, 1, _p(out)) == ERR_HIP
        assert hades_lib.hades252_matstream_commit(h, 1, 2, _limbs(TAG[2]), 1, None, _p(out), None, _p(root)) == ERR_HIP
        assert (out == SENTINEL).all() and (root == SENTINEL).all()
        assert _cols(hades_lib, h) == 2                                   # the last good total
        # an argument error is still an argument error, and changes nothing
        assert hades_lib.hades252_matstream_digests(h, 2, _p(out)) == INVALID
    finally:
        assert hades_lib.hades252_matstream_close(h) == 0
    with _stream(hades_lib, n_rows) as fresh:
        _absorb(hades_lib, fresh, sub, (2, 3))
        assert _digests(hades_lib, fresh, n_rows, 1).tobytes() == leaves(5, 1)[:n_rows].tobytes()
    h.value = 0x10000
    H.fault_inject("malloc:1")
    try:
        assert hades_lib.hades252_matstream_open(ctypes.byref(h), n_rows, _limbs(CAP)) == ERR_HIP and h.value is None
    finally:
        H.fault_inject(None)
    with _stream(hades_lib, n_rows) as again:
        _absorb(hades_lib, again, sub, (5,))
        assert _digests(hades_lib, again, n_rows, 0).tobytes() == leaves(5, 0)[:n_rows].tobytes()


# ---- 10. against the library's own calls -------------------------------------------------------------------------------
def test_big_matrix_against_the_row_major_calls(hades_lib, H, oracle):
    n_cols, arity = 13, 4
    m = oracle.gen_b(18000, N_BIG * n_cols).reshape(N_BIG, n_cols, 4)
    planes = M.planes_of(m)
    with H.MatrixStream(N_BIG, CAP) as ms:
        ms.absorb(np.ascontiguousarray(planes[:5])).absorb(np.ascontiguousarray(planes[5:]))
        assert ms.cols == n_cols
        digests, tree, root = ms.commit(arity, TAG[arity])
        d0 = ms.digests(0)
    assert digests.tobytes() == H.sponge_hash_host(m.reshape(-1), N_BIG, n_cols, CAP, 1).tobytes()
    assert digests[:100].tobytes() == M.row_digests(oracle, m[:100], CAP, 1).tobytes()
    assert root.tobytes() == H.merkle_root_host(digests.reshape(-1), arity, TAG[arity]).tobytes()
    assert tree[-1].tobytes() == root.tobytes() and tree.shape[0] * 32 == hades_lib.hades252_merkle_tree_bytes(N_BIG, arity)
    assert d0.tobytes() == H.sponge_hash_host(m.reshape(-1), N_BIG, n_cols, CAP, 0).tobytes()
