"""GPU tier, row f15 (beyond SURVEY section 8): device-resident mixed-height commitments (hades252_dmmcs_absorb / _tree / _open /
_verify) against the fixtures of f14, the host path of f14 on the same matrices (hades252_mmcs_absorb / _open / _verify) and
the model (tests/mmcs_model.py).  Exact, byte for byte, everywhere; device outputs sit between sentinel digests.  Every
hades252_dmmcs_* call here goes on one stream, and that stream is synchronised before a host-form call on the same handle:
the header's ordering rule."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matrix_model as M  # noqa: E402
import mmcs_model as MM  # noqa: E402
from gpu_common import CAP, TAG, to_dev, to_host  # noqa: E402
from test_gpu_f14_mmcs import _absorb, _case, _commit, _handle, _limbs, _p, _verify  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = M.SENTINEL
GUARD = 3                                  # sentinel digests on each side of an output
INVALID = -1
INJECT = MM.INJECT
ARITY, HEIGHTS, COLS = 2, tuple(1 << k for k in range(10, -1, -1)), tuple(range(1, 12))   # 2^10 .. 2^0 rows, 1 .. 11 columns


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "mmcs_kat.json")) as f:
        return json.load(f)["cases"]


def _planes_dev(torch, m, stride=None):
    """Row-major [n_rows, g, 4] -> (device planes int64 [g, stride, 4] with sentinels in the gap, n_rows)."""
    return to_dev(torch, M.planes_of(m, stride)).view(m.shape[1], -1, 4), m.shape[0]


def _tables(parts):
    return (np.array([t.data_ptr() for t, _ in parts], dtype=np.uint64), np.array([n for _, n in parts], dtype=np.uint64),
            np.array([t.shape[0] for t, _ in parts], dtype=np.uint64), np.array([t.shape[1] for t, _ in parts], dtype=np.uint64))


def _dabsorb(lib, h, parts, stream=None):
    """hades252_dmmcs_absorb of parts [(device planes, n_rows), ...] in one call."""
    pl, rows, cols, strides = _tables(parts)
    return lib.hades252_dmmcs_absorb(h, _p(pl), _p(rows), _p(cols), _p(strides), len(parts), stream)


def _guarded_dev(torch, n, words):
    """A device output of n items of `words` scalars between GUARD sentinel items: (whole tensor, pointer to the interior)."""
    big = torch.full((n + 2 * GUARD, words, 4), -1, dtype=torch.int64, device="cuda")
    return big, big.data_ptr() + GUARD * words * 32


def _intact_dev(big, n):
    a = to_host(big).reshape(big.shape)
    assert (a[:GUARD] == np.uint64((1 << 64) - 1)).all() and (a[GUARD + n:] == np.uint64((1 << 64) - 1)).all(), "written outside the output"
    return a[GUARD:GUARD + n]


def _dopen(lib, torch, h, parts, idx, depth, arity):
    """hades252_dmmcs_open -> (rows [q, sum of cols, 4], paths [q, depth, arity - 1, 4]) on the host, guards checked."""
    pl, rows, cols, strides = _tables(parts)
    d_idx = to_dev(torch, np.array(idx, dtype=np.uint64))
    total = int(cols.sum())
    r_big, r_ptr = _guarded_dev(torch, len(idx), total)
    p_big, p_ptr = _guarded_dev(torch, len(idx), depth * (arity - 1))
    assert lib.hades252_dmmcs_open(h, _p(pl), _p(rows), _p(cols), _p(strides), len(parts), d_idx.data_ptr(), len(idx), r_ptr, p_ptr, None) == 0
    torch.cuda.synchronize()
    return _intact_dev(r_big, len(idx)), _intact_dev(p_big, len(idx)).reshape(len(idx), depth, arity - 1, 4)


def _dverify(lib, torch, rows, heights, cols, idx, paths, arity, pad_mode, out_idx=1):
    q = len(idx)
    d_rows, d_paths, d_idx = to_dev(torch, rows), to_dev(torch, paths), to_dev(torch, np.array(idx, dtype=np.uint64))
    hs, cs = np.array(heights, dtype=np.uint64), np.array(cols, dtype=np.uint64)
    big, ptr = _guarded_dev(torch, q, 1)
    rc = lib.hades252_dmmcs_verify(d_rows.data_ptr(), _p(hs), _p(cs), len(heights), d_idx.data_ptr(), d_paths.data_ptr(), q, arity,
                                   _limbs(CAP), pad_mode, _limbs(TAG[arity]), _limbs(INJECT), out_idx, ptr, None)
    assert rc == 0
    torch.cuda.synchronize()
    return _intact_dev(big, q).reshape(q, 4)


@pytest.fixture(scope="module")
def tall(hades_lib, oracle):
    """The shape of the equality tests: eleven groups of 2^10 .. 2^0 rows with 1 .. 11 columns, committed once through the
    HOST path (one hades252_mmcs_absorb per group) -- the tree every device variant must reproduce -- and once by the model."""
    groups = [oracle.gen_b(50000 + 20000 * i, n * c).reshape(n, c, 4) for i, (n, c) in enumerate(zip(HEIGHTS, COLS))]
    with _handle(hades_lib) as h:
        for g in groups:
            _absorb(hades_lib, h, g)
        tree, root = _commit(hades_lib, h, HEIGHTS[0], ARITY, 1)
    want = MM.commit(oracle, groups, ARITY)
    assert tree.tobytes() == want[0].tobytes() and root.tobytes() == want[1].tobytes()
    return groups, tree.copy(), root.copy()


# ---- 1. known answers --------------------------------------------------------------------------------------------------
def test_fixtures_from_device_tensors_and_the_device_tree(hades_lib, H, torch_cuda, oracle, golden):
    torch = torch_cuda
    for c, case in zip(golden, MM.GOLDEN_CASES):
        arity, heights, cols, pad_mode, _, groups = _case(oracle, case)
        want_tree, want_root = MM.unhex(c["tree"]), MM.unhex([c["root"]])
        with H.Mmcs(CAP) as mc:
            with pytest.raises(Exception):
                mc.tree_dev()                                                    # no commit yet
            assert mc.absorb_dev([_planes_dev(torch, g)[0] for g in groups]) is mc
            assert mc.heights == list(heights) and [mc.cols(n) for n in heights] == list(cols)   # the totals moved at enqueue time
            torch.cuda.synchronize()
            tree, root = mc.commit(arity, TAG[arity], INJECT, pad_mode, c["out_idx"])
            assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()
            d_tree, d_arity = mc.tree_dev()
            assert d_arity == arity and tuple(d_tree.shape) == want_tree.shape
            assert to_host(d_tree).tobytes() == want_tree.tobytes()
            raw, n_bytes, a = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
            assert hades_lib.hades252_dmmcs_tree(mc._h, ctypes.byref(raw), ctypes.byref(n_bytes), ctypes.byref(a)) == 0
            assert n_bytes.value == want_tree.nbytes == hades_lib.hades252_mmcs_tree_bytes(heights[0], arity) and a.value == arity


# ---- 2. equality with the host path ------------------------------------------------------------------------------------
def test_eleven_parts_in_one_call_give_the_host_paths_tree(hades_lib, torch_cuda, tall):
    groups, want_tree, want_root = tall
    with _handle(hades_lib) as h:
        assert _dabsorb(hades_lib, h, [_planes_dev(torch_cuda, g) for g in groups]) == 0
        torch_cuda.cuda.synchronize()
        tree, root = _commit(hades_lib, h, HEIGHTS[0], ARITY, 1)
    assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()


def test_two_calls_meet_every_open_block_position(hades_lib, torch_cuda, tall):
    """Group i (i + 1 columns) gets i % 4 columns in the first call (none: the part is skipped) and the rest in the second,
    which so starts at every position 0 .. 3 of an open block, in one launch."""
    groups, want_tree, want_root = tall
    first = [_planes_dev(torch_cuda, g[:, :i % 4]) if i % 4 else (torch_cuda.zeros((0, g.shape[0], 4), dtype=torch_cuda.int64, device="cuda"),
                                                                 g.shape[0]) for i, g in enumerate(groups)]
    second = [_planes_dev(torch_cuda, g[:, i % 4:]) for i, g in enumerate(groups)]
    assert {i % 4 for i in range(len(groups))} == {0, 1, 2, 3}
    with _handle(hades_lib) as h:
        assert _dabsorb(hades_lib, h, first) == 0 and _dabsorb(hades_lib, h, list(reversed(second))) == 0
        torch_cuda.cuda.synchronize()
        tree, root = _commit(hades_lib, h, HEIGHTS[0], ARITY, 1)
    assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()


def test_host_and_device_feed_one_handle(hades_lib, torch_cuda, tall):
    groups, want_tree, want_root = tall
    with _handle(hades_lib) as h:
        _absorb(hades_lib, h, groups[0])                                         # the tallest group from the host: synchronous
        _absorb(hades_lib, h, groups[3][:, :2])
        assert _dabsorb(hades_lib, h, [_planes_dev(torch_cuda, g) for g in groups[1:3]] + [_planes_dev(torch_cuda, groups[3][:, 2:])] +
                        [_planes_dev(torch_cuda, g) for g in groups[4:-1]]) == 0
        torch_cuda.cuda.synchronize()                                            # before the next host-form call
        _absorb(hades_lib, h, groups[-1])
        tree, root = _commit(hades_lib, h, HEIGHTS[0], ARITY, 1)
    assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()


def test_strides_above_the_height_leave_the_gaps_unread_and_the_planes_unwritten(hades_lib, torch_cuda, tall):
    groups, want_tree, want_root = tall
    parts = [_planes_dev(torch_cuda, g, g.shape[0] + 1 + 2 * i) for i, g in enumerate(groups)]
    before = [to_host(t).copy() for t, _ in parts]
    with _handle(hades_lib) as h:
        assert _dabsorb(hades_lib, h, parts) == 0
        torch_cuda.cuda.synchronize()
        tree, root = _commit(hades_lib, h, HEIGHTS[0], ARITY, 1)
        idx = [0, 1, HEIGHTS[0] - 1, 513]
        rows, _ = _dopen(hades_lib, torch_cuda, h, parts, idx, 10, ARITY)
    assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()
    assert all(to_host(t).tobytes() == b.tobytes() for (t, _), b in zip(parts, before))            # the absorb never writes to planes
    assert rows.tobytes() == np.stack([MM.flat_rows(MM.open_rows(groups, i)) for i in idx]).tobytes()   # no sentinel in a row


# ---- 3. a refused call changes nothing ---------------------------------------------------------------------------------
def test_a_refused_call_between_two_good_ones_leaves_the_root_what_it_would_have_been(hades_lib, torch_cuda, tall):
    groups, want_tree, want_root = tall
    parts = [_planes_dev(torch_cuda, g) for g in groups]
    n = ctypes.c_uint64()
    with _handle(hades_lib) as h:
        assert _dabsorb(hades_lib, h, parts[:4]) == 0
        assert _dabsorb(hades_lib, h, [parts[4], parts[5], (parts[6][0], parts[4][1])]) == INVALID   # a height twice
        for g in groups[4:7]:
            assert hades_lib.hades252_mmcs_cols(h, g.shape[0], ctypes.byref(n)) == 0 and n.value == 0   # nothing created, nothing moved
        assert _dabsorb(hades_lib, h, parts[4:]) == 0
        torch_cuda.cuda.synchronize()
        tree, root = _commit(hades_lib, h, HEIGHTS[0], ARITY, 1)
    assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()


# ---- 4. openings -------------------------------------------------------------------------------------------------------
def test_open_equals_the_model_and_the_host_opening(hades_lib, H, torch_cuda, tall):
    """Every leaf index of the 2^10 shape, repeated and unsorted ones, h_0 and 2^63 (zeros)."""
    groups, want_tree, _ = tall
    h0 = HEIGHTS[0]
    idx = list(range(h0)) + [7, 7, h0 - 1, 0, 7] + [h0, 1 << 63]
    good = len(idx) - 2
    want_rows = np.zeros((len(idx), sum(COLS), 4), dtype=np.uint64)
    want_rows[:good] = np.stack([MM.flat_rows(MM.open_rows(groups, i)) for i in idx[:good]])
    want_paths = MM.open_paths(want_tree, h0, ARITY, idx)
    assert not want_paths[good:].any()
    assert H.mmcs_open(want_tree, h0, ARITY, np.array(idx, dtype=np.uint64)).tobytes() == want_paths.tobytes()
    parts = [_planes_dev(torch_cuda, g) for g in groups]
    with _handle(hades_lib) as h:
        assert _dabsorb(hades_lib, h, parts) == 0
        torch_cuda.cuda.synchronize()
        _commit(hades_lib, h, h0, ARITY, 1)
        rows, paths = _dopen(hades_lib, torch_cuda, h, parts, idx, 10, ARITY)
        assert rows.tobytes() == want_rows.tobytes() and paths.tobytes() == want_paths.tobytes()
        # a subset of the groups (the tallest and two more), and no query at all
        sub = [parts[0], parts[3], parts[10]]
        rows, paths = _dopen(hades_lib, torch_cuda, h, sub, idx[:65], 10, ARITY)
        assert paths.tobytes() == want_paths[:65].tobytes()
        assert rows.tobytes() == np.concatenate([want_rows[:65, :1], want_rows[:65, 6:10], want_rows[:65, 55:66]], axis=1).tobytes()
        pl, rws, cols, strides = _tables(parts)
        assert hades_lib.hades252_dmmcs_open(h, _p(pl), _p(rws), _p(cols), _p(strides), len(parts), None, 0, None, None, None) == 0


# ---- 5. verification ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def openings(oracle):
    """The first fixture shape with its honest openings and every tamper of them, each verified ONCE by the model."""
    arity, heights, cols, pad_mode, _, groups = _case(oracle, MM.GOLDEN_CASES[0])
    tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    kinds = []                                                                   # (rows, index, path, the model's root, honest)
    for i in range(heights[0]):
        r, p = MM.open_rows(groups, i), MM.open_paths(tree, heights[0], arity, [i])[0]
        kinds.append((MM.flat_rows(r), i, p, MM.verify(oracle, r, heights, i, p, arity, pad_mode=pad_mode), True))
        for _, br, bi, bp in MM.tampers(r, i, p, heights[0]):
            kinds.append((MM.flat_rows(br), bi, np.asarray(bp).reshape(p.shape), MM.verify(oracle, br, heights, bi, bp, arity, pad_mode=pad_mode), False))
    assert all((k[3] == root).all() == k[4] for k in kinds)                      # honest: the root; every tamper: another one
    return arity, heights, cols, pad_mode, root, kinds


@pytest.mark.parametrize("n", [1, 257, 4097])
def test_device_verification_equals_the_host_verification_and_the_model(hades_lib, torch_cuda, openings, n):
    arity, heights, cols, pad_mode, root, kinds = openings
    pick = [kinds[(7 * t) % len(kinds)] for t in range(n)]
    rows, idx, paths = np.stack([k[0] for k in pick]), [k[1] for k in pick], np.stack([k[2] for k in pick])
    want = np.stack([k[3] for k in pick])
    got = _dverify(hades_lib, torch_cuda, rows, heights, cols, idx, paths, arity, pad_mode)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == _verify(hades_lib, rows, heights, cols, idx, paths, arity, pad_mode).tobytes()
    honest = np.array([k[4] for k in pick])
    assert (got[honest] == root).all() and not (got[~honest] == root).all(axis=1).any()
    assert n == 1 or (honest.any() and not honest.all())


# ---- 6. the whole pipeline on a stream of its own ------------------------------------------------------------------------
def test_absorb_commit_open_verify_on_a_non_default_stream(hades_lib, H, torch_cuda, tall):
    torch = torch_cuda
    groups, want_tree, want_root = tall
    rng = np.random.default_rng(15)
    idx = rng.integers(0, HEIGHTS[0], size=300, dtype=np.uint64)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    parts = [_planes_dev(torch, g)[0] for g in groups]
    d_idx = to_dev(torch, idx)
    torch.cuda.synchronize()
    with H.Mmcs(CAP) as mc, torch.cuda.stream(s):
        assert torch.cuda.current_stream() == s and s != torch.cuda.default_stream()
        mc.absorb_dev(parts[:5]).absorb_dev(parts[5:])
        s.synchronize()                                                          # before the host-form commit
        tree, root = mc.commit(ARITY, TAG[ARITY], INJECT)
        rows_t, paths_t = mc.open_dev(parts, d_idx)
        roots_t = H.mmcs_verify_dev(rows_t, HEIGHTS, COLS, d_idx, paths_t, ARITY, CAP, TAG[ARITY], INJECT)
        assert torch.cuda.default_stream().query()                               # nothing went to the default stream
        s.synchronize()
        assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()
        assert to_host(roots_t).tobytes() == np.tile(want_root, (idx.size, 1)).tobytes()
        assert to_host(paths_t).tobytes() == MM.open_paths(want_tree, HEIGHTS[0], ARITY, idx.tolist()).tobytes()
        assert to_host(rows_t).tobytes() == np.stack([MM.flat_rows(MM.open_rows(groups, int(i))) for i in idx]).tobytes()


# ---- 7. argument rules ---------------------------------------------------------------------------------------------------
def test_argument_rules_on_a_live_handle(hades_lib):
    import test_dmmcs_abi
    test_dmmcs_abi.rules_that_need_a_handle(hades_lib)


def test_python_wrappers_refuse_wrong_shapes_before_the_library(H, torch_cuda, monkeypatch):
    import test_dmmcs_abi
    test_dmmcs_abi.wrappers_refuse_wrong_shapes(torch_cuda, H, monkeypatch)
