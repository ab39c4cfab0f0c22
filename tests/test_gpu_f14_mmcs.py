"""GPU tier, row f14 (beyond SURVEY section 8): mixed-height matrix commitments (hades252_mmcs_new / _absorb / _cols / _commit /
_free / _tree_bytes / _open / _verify) against the model (tests/mmcs_model.py: the C oracle's sponge and Merkle level), the
streaming commitment of f13 for one group, and the library's own device calls composed (sponge, path segments, a level at
arity 2 for every injection).  Exact, byte for byte, everywhere; outputs sit between sentinel digests."""
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
import mmcs_model as MM  # noqa: E402
from gpu_common import CAP, TAG, to_dev, to_host  # noqa: E402
from oracle_lib import P, limbs_of  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = M.SENTINEL
GUARD = 3                                  # sentinel digests on each side of an output
INVALID, ERR_HIP = -1, -2
INJECT = MM.INJECT


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "mmcs_kat.json")) as f:
        return json.load(f)["cases"]


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
def _handle(lib, cap=CAP):
    h = ctypes.c_void_p()
    assert lib.hades252_mmcs_new(ctypes.byref(h), _limbs(cap)) == 0 and h.value
    try:
        yield h
    finally:
        assert lib.hades252_mmcs_free(h) == 0


def _absorb(lib, h, part, stride=None):
    """Columns (row-major [n_rows, g, 4]) of the group of their height, from planes of stride `stride`."""
    n_rows = part.shape[0]
    planes = M.planes_of(part, n_rows if stride is None else stride)
    assert lib.hades252_mmcs_absorb(h, _p(planes), n_rows, part.shape[1], planes.shape[1]) == 0


def _cols(lib, h, n_rows):
    n = ctypes.c_uint64(1 << 63)
    assert lib.hades252_mmcs_cols(h, n_rows, ctypes.byref(n)) == 0
    return n.value


def _commit(lib, h, max_rows, arity, pad_mode, with_tree=True, out_idx=1):
    nodes = MM.tree_nodes(max_rows, arity)
    t_big, t_ptr = _guarded(nodes)
    root = np.full(4 + 2, SENTINEL, dtype=np.uint64)
    rc = lib.hades252_mmcs_commit(h, pad_mode, arity, _limbs(TAG[arity]), _limbs(INJECT), out_idx, t_ptr if with_tree else None,
                                  _p(root, 8))
    assert rc == 0 and root[0] == SENTINEL and root[5] == SENTINEL
    t = _intact(t_big, nodes)
    assert with_tree or (t == SENTINEL).all()
    return t, root[1:5]


def _verify(lib, rows, heights, cols, idx, paths, arity, pad_mode, out_idx=1):
    """rows [q, sum(cols), 4] -> roots [q, 4], written between sentinel digests."""
    q = len(idx)
    rows, paths = np.ascontiguousarray(rows, dtype=np.uint64), np.ascontiguousarray(paths, dtype=np.uint64)
    hs, cs, ix = np.array(heights, dtype=np.uint64), np.array(cols, dtype=np.uint64), np.array(idx, dtype=np.uint64)
    assert rows.shape == (q, sum(cols), 4) and paths.shape == (q, MM.depth_of(heights[0], arity), arity - 1, 4)
    big, ptr = _guarded(q)
    rc = lib.hades252_mmcs_verify(_p(rows), _p(hs), _p(cs), len(heights), _p(ix), _p(paths), q, arity, _limbs(CAP), pad_mode,
                                  _limbs(TAG[arity]), _limbs(INJECT), out_idx, ptr)
    assert rc == 0
    return _intact(big, q)


def _openings(groups, tree, arity, idx):
    """(rows [q, sum(cols), 4], paths) of the indices `idx` by the model's gathers."""
    h0 = max(g.shape[0] for g in groups)
    rows = np.stack([MM.flat_rows(MM.open_rows(groups, i)) for i in idx])
    return rows, MM.open_paths(tree, h0, arity, idx)


def _case(oracle, c):
    arity, heights, cols, pad_mode, index, first = c
    return arity, heights, cols, pad_mode, index, MM.golden_groups(oracle, heights, cols, first)


# ---- 1. known answers --------------------------------------------------------------------------------------------------
def test_fixtures_through_python_and_c_interleaved_and_in_every_split(hades_lib, H, oracle, golden):
    for c, case in zip(golden, MM.GOLDEN_CASES):
        arity, heights, cols, pad_mode, index, groups = _case(oracle, case)
        cap, tag, inj = int(c["capacity_mont"], 16), int(c["tag_mont"], 16), int(c["inject_tag_mont"], 16)
        want_tree, want_root = MM.unhex(c["tree"]), MM.unhex([c["root"]])
        assert (cap, tag, inj) == (CAP, TAG[arity], INJECT)
        with H.Mmcs(cap) as mc:                                                  # Python: one call per group, shortest first
            for g in reversed(groups):
                assert mc.absorb(M.planes_of(g)) is mc
            assert mc.heights == list(heights) and [mc.cols(h) for h in heights] == list(cols) and mc.cols(2) == 0
            tree, root = mc.commit(arity, tag, inj, pad_mode, c["out_idx"])
            assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()
            t2, r2 = mc.commit(arity, tag, inj, pad_mode, want_tree=False)
            assert t2 is None and r2.tobytes() == root.tobytes()
        with _handle(hades_lib) as h:                                            # C: a column at a time, round robin over the heights
            for j in range(max(cols)):
                for g in groups:
                    if j < g.shape[1]:
                        _absorb(hades_lib, h, g[:, j:j + 1], g.shape[0] + j)
            assert [_cols(hades_lib, h, n) for n in heights] == list(cols)
            tree, root = _commit(hades_lib, h, heights[0], arity, pad_mode)
            assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()
            assert _commit(hades_lib, h, heights[0], arity, pad_mode, with_tree=False)[1].tobytes() == want_root.tobytes()
        for split in MS.compositions(cols[0]):                                   # every split of the tallest group's columns
            with _handle(hades_lib) as h:
                parts = MS.split(groups[0], split)
                _absorb(hades_lib, h, parts[0])
                for g in groups[1:]:
                    _absorb(hades_lib, h, g)
                for part in parts[1:]:
                    _absorb(hades_lib, h, part)
                assert _commit(hades_lib, h, heights[0], arity, pad_mode)[0].tobytes() == want_tree.tobytes(), split


# ---- 2. one group is f13 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arity,n_rows", [(2, 512), (3, 243), (4, 256)])
def test_one_group_is_the_digests_and_the_tree_of_the_streaming_commitment(hades_lib, H, oracle, arity, n_rows):
    m = oracle.gen_b(23000, n_rows * 7).reshape(n_rows, 7, 4)
    for pad_mode in (0, 1):
        with H.MatrixStream(n_rows, CAP) as ms:
            digests, tree, root = ms.absorb(M.planes_of(m)).commit(arity, TAG[arity], pad_mode)
        with _handle(hades_lib) as h:
            _absorb(hades_lib, h, m[:, :3])
            _absorb(hades_lib, h, m[:, 3:], n_rows + 5)
            got_tree, got_root = _commit(hades_lib, h, n_rows, arity, pad_mode)
        assert got_tree.tobytes() == np.concatenate([digests, tree]).tobytes() and got_root.tobytes() == root.tobytes()
        assert got_tree.nbytes == hades_lib.hades252_mmcs_tree_bytes(n_rows, arity)


# ---- 3. prefixes -------------------------------------------------------------------------------------------------------
def test_commit_absorb_more_commit_again(hades_lib, oracle):
    arity, heights = 2, (64, 16, 2)
    a, b, c = (oracle.gen_b(23500 + 1000 * i, n * 6).reshape(n, 6, 4) for i, n in enumerate(heights))
    with _handle(hades_lib) as h:
        _absorb(hades_lib, h, a[:, :2])
        _absorb(hades_lib, h, c[:, :5])
        for pad_mode in (1, 0):
            tree, root = _commit(hades_lib, h, 64, arity, pad_mode)
            want = MM.commit(oracle, [a[:, :2], c[:, :5]], arity, pad_mode=pad_mode)
            assert tree.tobytes() == want[0].tobytes() and root.tobytes() == want[1].tobytes()
        _absorb(hades_lib, h, b[:, :4])                                          # a new height between the two, and more columns
        _absorb(hades_lib, h, a[:, 2:])
        _absorb(hades_lib, h, c[:, 5:])
        for pad_mode in (0, 1):
            tree, root = _commit(hades_lib, h, 64, arity, pad_mode)
            want = MM.commit(oracle, [a, b[:, :4], c], arity, pad_mode=pad_mode)
            assert tree.tobytes() == want[0].tobytes() and root.tobytes() == want[1].tobytes()
        assert [_cols(hades_lib, h, n) for n in heights] == [6, 4, 6]


# ---- 4. every level form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arity,heights,cols", [(2, (1 << 15, 1 << 13, 1 << 9), (6, 9, 3)), (4, (4 ** 7, 4 ** 5), (5, 2))])
def test_injections_at_a_per_lane_a_five_waves_and_a_per_wave_level(hades_lib, H, oracle, arity, heights, cols):
    """The row digests and the injections run one item per lane; the levels they follow take the form their size asks for
    (gpu_common.level_form): 2^13 parents five waves per parent, 2^9 and 4^5 one parent per wave, and the levels around them
    one parent per row and, fused above the shortest group, the tree build's own.  The tree is the model's byte for byte."""
    from gpu_common import level_form
    forms = {level_form(n * arity, arity).split("<")[0] for n in heights[1:]}
    assert forms == ({"k_merkle_coop", "k_merkle_lanes"} if arity == 2 else {"k_merkle_lanes"})
    groups = [oracle.gen_b(24000 + 100000 * i, n * k).reshape(n, k, 4) for i, (n, k) in enumerate(zip(heights, cols))]
    want_tree, want_root = MM.commit(oracle, groups, arity)
    with H.Mmcs(CAP) as mc:
        for g in groups:
            mc.absorb(M.planes_of(g))
        tree, root = mc.commit(arity, TAG[arity], INJECT)
    assert tree.shape == want_tree.shape
    off = 0
    for l, n in enumerate(heights[0] // arity ** k for k in range(MM.depth_of(heights[0], arity) + 1)):
        assert tree[off:off + n].tobytes() == want_tree[off:off + n].tobytes(), "level %d from the leaves" % l
        off += n
    assert root.tobytes() == want_root.tobytes() == tree[-1].tobytes()
    # a few openings of the big tree verify to its root
    idx = [0, 1, heights[0] // 2 + 3, heights[0] - 1]
    rows, paths = _openings(groups, tree, arity, idx)
    assert H.mmcs_open(tree, heights[0], arity, idx).tobytes() == paths.tobytes()
    got = _verify(hades_lib, rows, heights, cols, idx, paths, arity, 1)
    assert got.tobytes() == np.tile(root, (len(idx), 1)).tobytes()


# ---- 5. tiling ---------------------------------------------------------------------------------------------------------
_TILE_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from hades252_amd import build, strategy as H
build.build(verbose=False)
assert os.environ["HADES252_TEST_MATRIX_CHUNK_ROWS"] == "256" and int(os.environ["HADES252_TEST_MATRIX_CHUNK_COLS"]) >= 1
src, dst, cap, tag, inj = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
flat = np.fromfile(src, dtype=np.uint64)
tall, short = flat[:9 * 1027 * 4].reshape(9, 1027, 4), flat[9 * 1027 * 4:].reshape(5, 256, 4)
with H.Mmcs(cap) as mc:
    mc.absorb(np.ascontiguousarray(tall[:2]), 1024).absorb(short).absorb(np.ascontiguousarray(tall[2:]), 1024)
    tree, root = mc.commit(4, tag, inj, 1)
    print("TILED", mc.cols(1024), mc.cols(256), tree.shape[0])
np.concatenate([tree.reshape(-1), root]).tofile(dst)
"""


@pytest.mark.parametrize("tile_cols", [1, 3, 4])
def test_tiles_give_the_untiled_bytes(hades_lib, H, oracle, tmp_path, tile_cols):
    """HADES252_TEST_MATRIX_CHUNK_ROWS = 256 and HADES252_TEST_MATRIX_CHUNK_COLS (read once by the library, hence a child
    process): the 1024 rows of the tall group are four row tiles, its 9 columns absorbed as (2, 7) are tiles of one, three and
    four columns; the short group is one row tile."""
    tall = M.planes_of(oracle.gen_b(25000, 1024 * 9).reshape(1024, 9, 4), 1027)
    short = M.planes_of(oracle.gen_b(26000, 256 * 5).reshape(256, 5, 4))
    with H.Mmcs(CAP) as mc:
        mc.absorb(np.ascontiguousarray(tall[:2]), 1024).absorb(short).absorb(np.ascontiguousarray(tall[2:]), 1024)
        tree, root = mc.commit(4, TAG[4], INJECT, 1)
    want = MM.commit(oracle, [M.matrix_of(tall, 1024), M.matrix_of(short, 256)], 4)
    assert tree.tobytes() == want[0].tobytes() and root.tobytes() == want[1].tobytes()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([tall.reshape(-1), short.reshape(-1)]).tofile(src)
    env = dict(os.environ, HADES252_TEST_MATRIX_CHUNK_ROWS="256", HADES252_TEST_MATRIX_CHUNK_COLS=str(tile_cols))
    run = subprocess.run([sys.executable, "-c", _TILE_CHILD, str(src), str(dst), str(CAP), str(TAG[4]), str(INJECT)], cwd=ROOT,
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "TILED 9 5 %d" % tree.shape[0] in run.stdout, run.stdout[-1500:] + run.stderr[-3000:]
    assert np.fromfile(dst, dtype=np.uint64).tobytes() == np.concatenate([tree.reshape(-1), root]).tobytes()


# ---- 6. openings -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arity", [2, 3, 4])
def test_open_equals_the_device_opening_of_the_uploaded_tree(hades_lib, H, torch_cuda, oracle, arity):
    h0 = arity ** 4
    groups = [oracle.gen_b(27000 + 5000 * i, n * 3).reshape(n, 3, 4) for i, n in enumerate((h0, arity ** 2, 1))]
    tree, _ = MM.commit(oracle, groups, arity)
    idx = np.array(list(range(h0)) + [h0, h0 + 1, (1 << 64) - 1, 0, h0 - 1, 3, 3], dtype=np.uint64)
    d_leaves, d_tree, d_idx = to_dev(torch_cuda, tree[:h0]), to_dev(torch_cuda, tree[h0:]), to_dev(torch_cuda, idx)
    d_paths = torch_cuda.full((idx.size * 4 * (arity - 1) * 4,), -1, dtype=torch_cuda.int64, device="cuda")
    assert hades_lib.hades252_merkle_open_dev(d_leaves.data_ptr(), d_tree.data_ptr(), h0, arity, d_idx.data_ptr(), idx.size,
                                              d_paths.data_ptr(), None) == 0     # (the C call: the wrapper refuses such indices)
    torch_cuda.cuda.synchronize()
    want = to_host(d_paths).reshape(idx.size, 4, arity - 1, 4)
    big = np.full((idx.size + 2 * GUARD, 4, arity - 1, 4), SENTINEL, dtype=np.uint64)
    assert hades_lib.hades252_mmcs_open(_p(tree), h0, arity, _p(idx), idx.size, _p(big, GUARD * 4 * (arity - 1) * 32)) == 0
    assert (big[:GUARD] == SENTINEL).all() and (big[GUARD + idx.size:] == SENTINEL).all()
    assert big[GUARD:GUARD + idx.size].tobytes() == want.tobytes() == MM.open_paths(tree, h0, arity, idx.tolist()).tobytes()
    assert not want[h0:h0 + 3].any()                                             # an index >= h_0: an all-zero path


# ---- 7. verification: known answers ------------------------------------------------------------------------------------
def test_every_index_of_the_fixtures_verifies_and_the_tampered_openings_give_the_models_roots(hades_lib, H, oracle, golden):
    for c, case in zip(golden, MM.GOLDEN_CASES):
        arity, heights, cols, pad_mode, index, groups = _case(oracle, case)
        tree, root = MM.unhex(c["tree"]), MM.unhex([c["root"]])[0]
        idx = list(range(heights[0]))
        rows, paths = _openings(groups, tree, arity, idx)
        got = _verify(hades_lib, rows, heights, cols, idx, paths, arity, pad_mode)
        assert got.tobytes() == np.tile(root, (len(idx), 1)).tobytes()
        assert H.mmcs_verify(rows, heights, cols, idx, paths, arity, CAP, TAG[arity], INJECT, pad_mode).tobytes() == got.tobytes()
        # the fixture's opening, and every tamper of it: the recorded roots, all in one call
        r0, p0 = [MM.unhex(r) for r in c["opening"]["rows"]], MM.unhex(c["opening"]["path"]).reshape(-1, arity - 1, 4)
        bad = MM.tampers(r0, index, p0, heights[0])
        assert [b[0] for b in bad] == [t["what"] for t in c["tampered"]]
        rows = np.stack([MM.flat_rows(r0)] + [MM.flat_rows(b[1]) for b in bad])
        idx = [index] + [b[2] for b in bad]
        paths = np.stack([p0] + [np.asarray(b[3]).reshape(p0.shape) for b in bad])
        got = _verify(hades_lib, rows, heights, cols, idx, paths, arity, pad_mode)
        want = MM.unhex([c["root"]] + [t["root"] for t in c["tampered"]])
        assert got.tobytes() == want.tobytes()
        assert len({g.tobytes() for g in got}) == len(bad) + 1                  # every tamper moves the root


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_query_counts_around_a_wave_and_a_block_with_guard_words_behind_the_roots(hades_lib, oracle, n):
    arity, heights, cols, pad_mode, _, groups = _case(oracle, MM.GOLDEN_CASES[0])
    tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    idx = [(5 * t + 1) % heights[0] for t in range(n)]
    rows, paths = _openings(groups, tree, arity, idx)
    want = np.tile(root, (n, 1))
    for t in range(0, n, 7):                                                     # every seventh opening claims a neighbouring index
        idx[t] = (idx[t] + 1) % heights[0]
        want[t] = MM.verify(oracle, MM.open_rows(groups, (5 * t + 1) % heights[0]), heights, idx[t], paths[t], arity, pad_mode=pad_mode)
    got = _verify(hades_lib, rows, heights, cols, idx, paths, arity, pad_mode)
    assert got.tobytes() == want.tobytes()


# ---- 8. column counts and edge values ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_mode", [0, 1])
def test_columns_per_group_under_both_paddings_with_zero_and_p_minus_one_in_every_block_position(hades_lib, oracle, pad_mode):
    """1, 3, 4, 5 and 8 columns in each of two groups: a partial block, a block the pad scalar closes, one it opens, a body
    and a tail, two whole blocks.  Row r of the tall group holds zero at column r % c and p - 1 at column (r + 1) % c, the
    rows of the short group the other way round: over the 16 rows every value meets every column, hence every position."""
    arity, heights = 2, (16, 4)
    edge = {0: np.zeros(4, dtype=np.uint64), 1: np.array(limbs_of(P - 1), dtype=np.uint64)}
    for c in (1, 3, 4, 5, 8):
        groups = [oracle.gen_b(28000 + 100 * c + 1000 * i, n * c).reshape(n, c, 4).copy() for i, n in enumerate(heights)]
        for i, g in enumerate(groups):
            for r in range(g.shape[0]):
                g[r, (r + i) % c] = edge[0]
                g[r, (r + 1 - i) % c] = edge[1 if c > 1 else r % 2]
        tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
        with _handle(hades_lib) as h:
            for g in groups:
                _absorb(hades_lib, h, g)
            got_tree, got_root = _commit(hades_lib, h, heights[0], arity, pad_mode)
        assert got_tree.tobytes() == tree.tobytes() and got_root.tobytes() == root.tobytes(), c
        idx = list(range(heights[0]))
        rows, paths = _openings(groups, tree, arity, idx)
        got = _verify(hades_lib, rows, heights, (c, c), idx, paths, arity, pad_mode)
        assert got.tobytes() == np.tile(root, (len(idx), 1)).tobytes(), c
        for out_idx in (0, 4):                                                   # another output word, on one opening
            want = MM.verify(oracle, MM.open_rows(groups, 5), heights, 5, paths[5], arity, pad_mode=pad_mode, out_idx=out_idx)
            got = _verify(hades_lib, rows[5:6], heights, (c, c), [5], paths[5:6], arity, pad_mode, out_idx)
            assert got[0].tobytes() == want.tobytes(), (c, out_idx)


# ---- 9. against the library's own device calls -------------------------------------------------------------------------
def test_4096_queries_against_the_composed_device_calls(hades_lib, H, torch_cuda, oracle):
    """The chain of one query as the existing entry points run it: a sponge per group, a path verification per tree segment
    (hades252_merkle_verify_dev on the segment's levels with the index shifted down), a level at arity 2 under the
    injection tag for every injection."""
    torch = torch_cuda
    arity, heights, cols, pad_mode, nq = 2, (1 << 10, 1 << 6, 1), (5, 3, 2), 1, 4096
    groups = [oracle.gen_b(29000 + 10000 * i, n * k).reshape(n, k, 4) for i, (n, k) in enumerate(zip(heights, cols))]
    with H.Mmcs(CAP) as mc:
        for g in groups:
            mc.absorb(M.planes_of(g))
        tree, root = mc.commit(arity, TAG[arity], INJECT, pad_mode)
    rng = np.random.default_rng(14)
    idx = rng.integers(0, heights[0], size=nq, dtype=np.uint64)
    rows = np.concatenate([g[(idx // np.uint64(heights[0] // g.shape[0])).astype(np.int64)] for g in groups], axis=1)
    paths = H.mmcs_open(tree, heights[0], arity, idx)
    bad = np.arange(0, nq, 5)                                                    # a fifth of the openings is tampered with
    rows[bad[0::3], rng.integers(0, sum(cols), size=bad[0::3].size)] = np.array([MM.BAD, 0, 0, 0], dtype=np.uint64)
    paths[bad[1::3], rng.integers(0, 10, size=bad[1::3].size), 0] = np.array([MM.BAD + 1, 0, 0, 0], dtype=np.uint64)
    idx[bad[2::3]] ^= np.uint64(1)
    got = H.mmcs_verify(rows, heights, cols, idx, paths, arity, CAP, TAG[arity], INJECT, pad_mode)
    # the composition
    depths = [MM.depth_of(n, arity) for n in heights]
    d_idx, d_paths = to_dev(torch, idx), to_dev(torch, paths).view(nq, depths[0], arity - 1, 4)
    node, at, col = None, depths[0], 0
    for g, (d, k) in enumerate(zip(depths, cols)):
        leaf = H.sponge_hash(to_dev(torch, np.ascontiguousarray(rows[:, col:col + k])).view(-1), k, CAP, pad_mode).view(nq, 4)
        col += k
        if g == 0:
            node = leaf
        else:
            seg = d_paths[:, depths[0] - at:depths[0] - d].contiguous()
            shifted = torch.from_numpy((idx >> np.uint64(depths[0] - at)).view(np.int64)).cuda()
            node = H.merkle_verify(node.contiguous(), shifted, seg, arity, TAG[arity]).view(nq, 4)
            node = H.merkle_level(torch.stack([node, leaf], dim=1).contiguous().view(-1), 2, INJECT).view(nq, 4)
            at = d
    assert at == 0                                                               # the last group sits at the root
    want = to_host(node).reshape(nq, 4)
    assert got.tobytes() == want.tobytes()
    honest = np.ones(nq, dtype=bool)
    honest[bad] = False
    assert (got[honest] == root).all() and not (got[~honest] == root).all(axis=1).any()


# ---- 10. chunks of queries -----------------------------------------------------------------------------------------------
_CHUNK_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from hades252_amd import build, strategy as H
build.build(verbose=False)
assert os.environ["HADES252_TEST_MMCS_CHUNK_QUERIES"] == sys.argv[3]
a = np.load(sys.argv[1])
roots = H.mmcs_verify(a["rows"], a["heights"], a["cols"], a["idx"], a["paths"], 2, int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), 1)
print("CHUNKED", roots.shape[0])
roots.tofile(sys.argv[2])
"""


@pytest.mark.parametrize("chunk", [1, 100, 256])
def test_forced_query_chunks_give_the_unchunked_bytes(hades_lib, H, oracle, tmp_path, chunk):
    """HADES252_TEST_MMCS_CHUNK_QUERIES (read once by the library, hence a child process): 257 queries in 257 chunks of one
    (both buffers reused over and over), in three chunks (the last ragged) and in two (the last a single query)."""
    arity, heights, cols, pad_mode, _, groups = _case(oracle, MM.GOLDEN_CASES[0])
    tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    idx = [(3 * t) % heights[0] for t in range(257)]
    rows, paths = _openings(groups, tree, arity, idx)
    rows[::4, 0] = np.array([MM.BAD, 0, 0, 0], dtype=np.uint64)                  # every fourth root differs
    want = H.mmcs_verify(rows, heights, cols, idx, paths, arity, CAP, TAG[arity], INJECT, pad_mode)
    assert (want[1] == root).all() and not (want[0] == root).all()
    src, dst = tmp_path / "in.npz", tmp_path / "out.bin"
    np.savez(src, rows=rows, heights=np.array(heights, dtype=np.uint64), cols=np.array(cols, dtype=np.uint64),
             idx=np.array(idx, dtype=np.uint64), paths=paths)
    env = dict(os.environ, HADES252_TEST_MMCS_CHUNK_QUERIES=str(chunk))
    run = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, str(src), str(dst), str(chunk), str(CAP), str(TAG[arity]), str(INJECT)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "CHUNKED 257" in run.stdout, run.stdout[-1500:] + run.stderr[-3000:]
    assert np.fromfile(dst, dtype=np.uint64).tobytes() == want.tobytes()


# ---- 11. argument rules and simulated host errors ----------------------------------------------------------------------
def test_argument_rules_on_a_live_handle(hades_lib):
    import test_mmcs_abi
    test_mmcs_abi.rules_that_need_a_handle(hades_lib)


def test_a_failing_copy_poisons_the_handle_and_loses_no_pipe(hades_lib, H, oracle):
    """hades252_fault_inject returns an error INSTEAD of making the call: no GPU work is disturbed."""
    arity, heights, cols, pad_mode, _, groups = _case(oracle, MM.GOLDEN_CASES[0])
    want_tree, want_root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    planes = [M.planes_of(g) for g in groups]
    root = np.full(4, SENTINEL, dtype=np.uint64)
    tree = np.full((MM.tree_nodes(heights[0], arity), 4), SENTINEL, dtype=np.uint64)

    def commit(h):
        return hades_lib.hades252_mmcs_commit(h, pad_mode, arity, _limbs(TAG[arity]), _limbs(INJECT), 1, _p(tree), _p(root))

    for where in ("absorb", "commit"):
        H.trim()
        h = ctypes.c_void_p()
        assert hades_lib.hades252_mmcs_new(ctypes.byref(h), _limbs(CAP)) == 0
        try:
            assert hades_lib.hades252_mmcs_absorb(h, _p(planes[0]), 8, 5, 8) == 0
            assert hades_lib.hades252_mmcs_absorb(h, _p(planes[1]), 4, 2, 4) == 0
            H.fault_inject("memcpy:1")
            try:
                if where == "absorb":
                    assert hades_lib.hades252_mmcs_absorb(h, _p(planes[1], 2 * 4 * 32), 4, 1, 4) == ERR_HIP
                else:
                    assert commit(h) == ERR_HIP
            finally:
                H.fault_inject(None)
            assert hades_lib.hades252_mmcs_absorb(h, _p(planes[2]), 1, 2, 1) == ERR_HIP
            assert hades_lib.hades252_mmcs_absorb(h, None, 8, 0, 0) == ERR_HIP
            assert commit(h) == ERR_HIP
            assert (root == SENTINEL).all() and (tree == SENTINEL).all()
            assert _cols(hades_lib, h, 8) == 5 and _cols(hades_lib, h, 4) == 2 and _cols(hades_lib, h, 1) == 0   # the last good totals
            assert hades_lib.hades252_mmcs_commit(h, 2, arity, _limbs(TAG[arity]), _limbs(INJECT), 1, None, _p(root)) == INVALID
        finally:
            assert hades_lib.hades252_mmcs_free(h) == 0
        with _handle(hades_lib) as fresh:                                        # the pool is whole: the next call gets a pipe
            for g in groups:
                _absorb(hades_lib, fresh, g)
            got_tree, got_root = _commit(hades_lib, fresh, heights[0], arity, pad_mode)
            assert got_tree.tobytes() == want_tree.tobytes() and got_root.tobytes() == want_root.tobytes()
    # verification has no handle: the call fails, the next one is whole
    idx = list(range(heights[0]))
    rows, paths = _openings(groups, want_tree, arity, idx)
    H.fault_inject("memcpy:2")
    try:
        with pytest.raises(Exception) as e:
            H.mmcs_verify(rows, heights, cols, idx, paths, arity, CAP, TAG[arity], INJECT, pad_mode)
        assert getattr(e.value, "code", None) == ERR_HIP
    finally:
        H.fault_inject(None)
    assert _verify(hades_lib, rows, heights, cols, idx, paths, arity, pad_mode).tobytes() == np.tile(want_root, (8, 1)).tobytes()
    H.fault_inject("malloc:1")
    try:
        with _handle(hades_lib) as mc:                                           # the group's allocation fails: poisoned, nothing kept
            assert hades_lib.hades252_mmcs_absorb(mc, _p(planes[0]), 8, 5, 8) == ERR_HIP
            H.fault_inject(None)
            assert _cols(hades_lib, mc, 8) == 0 and hades_lib.hades252_mmcs_absorb(mc, _p(planes[0]), 8, 5, 8) == ERR_HIP
    finally:
        H.fault_inject(None)


# ---- 12. interleaving --------------------------------------------------------------------------------------------------
def test_two_handles_a_stream_and_a_trim_do_not_disturb_each_other(hades_lib, H, oracle):
    cap_b = (CAP + 12345) % P
    a = [oracle.gen_b(30000 + 3000 * i, n * 4).reshape(n, 4, 4) for i, n in enumerate((81, 9))]         # arity 3
    b = [oracle.gen_b(31000 + 3000 * i, n * 3).reshape(n, 3, 4) for i, n in enumerate((64, 16, 4))]     # arity 4
    s = oracle.gen_b(32000, 100 * 5).reshape(100, 5, 4)
    want_a = MM.commit(oracle, a, 3)
    want_b = MM.commit(oracle, b, 4, cap=cap_b, pad_mode=0)
    with _handle(hades_lib) as ha, _handle(hades_lib, cap_b) as hb, H.MatrixStream(100, CAP) as ms:
        _absorb(hades_lib, ha, a[0][:, :1])
        _absorb(hades_lib, hb, b[2])
        ms.absorb(M.planes_of(s[:, :2]))
        _absorb(hades_lib, ha, a[1])
        _absorb(hades_lib, hb, b[0][:, :2])
        H.trim()                                                                 # the pool is emptied; what the handles hold stays
        assert H.pool_bytes() == 0
        _absorb(hades_lib, ha, a[0][:, 1:])
        ms.absorb(M.planes_of(s[:, 2:]))
        _absorb(hades_lib, hb, b[1])
        tree_a, root_a = _commit(hades_lib, ha, 81, 3, 1)
        H.trim()
        _absorb(hades_lib, hb, b[0][:, 2:])
        big, ptr = _guarded(MM.tree_nodes(64, 4))
        root_b = np.zeros(4, dtype=np.uint64)
        assert hades_lib.hades252_mmcs_commit(hb, 0, 4, _limbs(TAG[4]), _limbs(INJECT), 1, ptr, _p(root_b)) == 0
        assert ms.digests(1).tobytes() == M.row_digests(oracle, s, CAP, 1).tobytes()
        assert tree_a.tobytes() == want_a[0].tobytes() and root_a.tobytes() == want_a[1].tobytes()
        assert _intact(big, MM.tree_nodes(64, 4)).tobytes() == want_b[0].tobytes() and root_b.tobytes() == want_b[1].tobytes()
        assert _commit(hades_lib, ha, 81, 3, 1)[1].tobytes() == want_a[1].tobytes()                       # and again, after the trim
