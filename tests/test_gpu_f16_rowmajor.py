"""GPU tier, row f16 (beyond SURVEY section 8): row-major matrices for the mixed-height commitments (hades252_rmmcs_absorb_rows,
hades252_rmmcs_absorb_ex, hades252_rmmcs_open_ex) against the fixtures of f14, the column-major paths of f14 / f15 on the same
matrices and the model (tests/mmcs_model.py).  A handle fed row-major holds the states it would hold after the column-major
calls on the transposed matrix, so every tree, root, row and path here is compared byte for byte; device outputs sit between
sentinel digests.  Every device-form call goes on one stream, and that stream is synchronised before a host-form call on the
same handle: the header's ordering rule."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj  # noqa: E402
import matrix_model as M  # noqa: E402
import mmcs_model as MM  # noqa: E402
import rowmajor_model as RM  # noqa: E402
from gpu_common import CAP, TAG, to_dev, to_host  # noqa: E402
from rowmajor_model import LAYOUT_COLS as COLS_, LAYOUT_ROWS as ROWS_  # noqa: E402
from test_gpu_f14_mmcs import _absorb, _case, _commit, _handle, _limbs, _p  # noqa: E402
from test_gpu_f15_dmmcs import (ARITY, COLS, HEIGHTS, INJECT, INVALID, _dabsorb, _guarded_dev, _intact_dev, _planes_dev, _tables,  # noqa: E402
                                golden, tall)  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SENTINEL = M.SENTINEL
VGPRS_PER_SIMD = 512


def _mat_dev(torch, m, layout, stride=None):
    """Row-major [n_rows, g, 4] -> a part (device tensor, n_rows, g, stride, layout): the matrix in `layout` on the device,
    sentinels in the gap behind every row (LAYOUT_ROWS: stride scalars per row) or plane (LAYOUT_COLS: stride rows)."""
    n_rows, g = m.shape[0], m.shape[1]
    if layout == ROWS_:
        stride = g if stride is None else stride
        return to_dev(torch, RM.rows_of(m, stride)).view(n_rows, stride, 4), n_rows, g, stride, layout
    stride = n_rows if stride is None else stride
    return to_dev(torch, M.planes_of(m, stride)).view(g, stride, 4), n_rows, g, stride, layout


def _ex_tables(parts):
    return [np.array([p[0].data_ptr() for p in parts], dtype=np.uint64)] + \
           [np.array([p[k] for p in parts], dtype=np.uint64) for k in (1, 2, 3)] + [np.array([p[4] for p in parts], dtype=np.uint32)]


def _xabsorb(lib, h, parts, stream=None, layouts=True):
    """hades252_rmmcs_absorb_ex of parts (as _mat_dev makes them) in one call."""
    pl, rows, cols, strides, lay = _ex_tables(parts)
    return lib.hades252_rmmcs_absorb_ex(h, _p(pl), _p(rows), _p(cols), _p(strides), _p(lay) if layouts else None, len(parts), stream)


def _xopen(lib, torch, h, parts, idx, depth, arity):
    """hades252_rmmcs_open_ex -> (rows [q, sum of cols, 4], paths [q, depth, arity - 1, 4]) on the host, guards checked."""
    pl, rows, cols, strides, lay = _ex_tables(parts)
    d_idx = to_dev(torch, np.array(idx, dtype=np.uint64))
    total = int(cols.sum())
    r_big, r_ptr = _guarded_dev(torch, len(idx), total)
    p_big, p_ptr = _guarded_dev(torch, len(idx), depth * (arity - 1))
    assert lib.hades252_rmmcs_open_ex(h, _p(pl), _p(rows), _p(cols), _p(strides), _p(lay), len(parts), d_idx.data_ptr(), len(idx), r_ptr,
                                      p_ptr, None) == 0
    torch.cuda.synchronize()
    return _intact_dev(r_big, len(idx)), _intact_dev(p_big, len(idx)).reshape(len(idx), depth, arity - 1, 4)


def _rabsorb(lib, h, part, stride=None):
    """hades252_rmmcs_absorb_rows of columns (row-major [n_rows, g, 4]) from a host buffer of row stride `stride`."""
    rows = RM.rows_of(part, stride)
    assert lib.hades252_rmmcs_absorb_rows(h, _p(rows), part.shape[0], part.shape[1], rows.shape[1]) == 0


def _same(tree, root, want_tree, want_root):
    assert tree.tobytes() == want_tree.tobytes() and root.tobytes() == want_root.tobytes()


# ---- 1. known answers --------------------------------------------------------------------------------------------------
def test_fixtures_all_rows_through_the_device_form_and_the_host_form(hades_lib, H, torch_cuda, oracle, golden):
    torch = torch_cuda
    for c, case in zip(golden, MM.GOLDEN_CASES):
        arity, heights, cols, pad_mode, _, groups = _case(oracle, case)
        want_tree, want_root = MM.unhex(c["tree"]), MM.unhex([c["root"]])
        with H.Mmcs(CAP) as mc:                                                  # Python: device tensors [n_rows, g, 4]
            assert mc.absorb_dev([to_dev(torch, g).view(g.shape) for g in groups], [H._lib.LAYOUT_ROWS] * len(groups)) is mc
            assert mc.heights == list(heights) and [mc.cols(n) for n in heights] == list(cols)   # the totals moved at enqueue time
            torch.cuda.synchronize()
            _same(*mc.commit(arity, TAG[arity], INJECT, pad_mode, c["out_idx"]), want_tree, want_root)
        with _handle(hades_lib) as h:                                            # C: one call, all parts row-major
            assert _xabsorb(hades_lib, h, [_mat_dev(torch, g, ROWS_) for g in groups]) == 0
            torch.cuda.synchronize()
            _same(*_commit(hades_lib, h, heights[0], arity, pad_mode, out_idx=c["out_idx"]), want_tree, want_root)
        with H.Mmcs(CAP) as mc:                                                  # the host form, Python then C
            for g in reversed(groups):
                assert mc.absorb_rows(np.ascontiguousarray(g)) is mc
            assert mc.heights == list(heights) and [mc.cols(n) for n in heights] == list(cols)
            _same(*mc.commit(arity, TAG[arity], INJECT, pad_mode, c["out_idx"]), want_tree, want_root)
        with _handle(hades_lib) as h:
            for g in groups:
                _rabsorb(hades_lib, h, g)
            _same(*_commit(hades_lib, h, heights[0], arity, pad_mode, out_idx=c["out_idx"]), want_tree, want_root)


# ---- 2. equality with the host path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1])
def test_mixed_layouts_in_one_launch_give_the_host_paths_tree(hades_lib, torch_cuda, tall, parity):
    """Eleven parts in ONE call, the groups of one parity row-major and the others column-major."""
    groups, want_tree, want_root = tall
    parts = [_mat_dev(torch_cuda, g, ROWS_ if i % 2 == parity else COLS_) for i, g in enumerate(groups)]
    assert {p[4] for p in parts} == {ROWS_, COLS_}
    with _handle(hades_lib) as h:
        assert _xabsorb(hades_lib, h, parts) == 0
        torch_cuda.cuda.synchronize()
        _same(*_commit(hades_lib, h, HEIGHTS[0], ARITY, 1), want_tree, want_root)


def test_two_calls_meet_every_open_block_position_across_a_layout_switch(hades_lib, torch_cuda, tall):
    """Group i (i + 1 columns) gets i % 4 columns column-major in the first call (none: the part is skipped, and its layout
    is garbage) and the rest row-major in the second, parts reversed, which so starts at every position 0 .. 3 of an open
    block, in one launch."""
    torch = torch_cuda
    groups, want_tree, want_root = tall
    skipped = lambda g: (torch.zeros((0, g.shape[0], 4), dtype=torch.int64, device="cuda"), g.shape[0], 0, g.shape[0], 77)   # noqa: E731
    first = [_mat_dev(torch, g[:, :i % 4], COLS_) if i % 4 else skipped(g) for i, g in enumerate(groups)]
    second = [_mat_dev(torch, g[:, i % 4:], ROWS_) for i, g in enumerate(groups)]
    assert {i % 4 for i in range(len(groups))} == {0, 1, 2, 3}
    with _handle(hades_lib) as h:
        assert _xabsorb(hades_lib, h, first) == 0 and _xabsorb(hades_lib, h, list(reversed(second))) == 0
        torch.cuda.synchronize()
        _same(*_commit(hades_lib, h, HEIGHTS[0], ARITY, 1), want_tree, want_root)


def test_row_strides_above_the_width_leave_the_gaps_unread_and_the_matrices_unwritten(hades_lib, torch_cuda, tall):
    groups, want_tree, want_root = tall
    parts = [_mat_dev(torch_cuda, g, ROWS_, g.shape[1] + 1 + 2 * i) for i, g in enumerate(groups)]
    before = [to_host(p[0]).copy() for p in parts]
    assert all((b == SENTINEL).any() for b in before)
    with _handle(hades_lib) as h:
        assert _xabsorb(hades_lib, h, parts) == 0
        torch_cuda.cuda.synchronize()
        tree, root = _commit(hades_lib, h, HEIGHTS[0], ARITY, 1)
        idx = [0, 1, HEIGHTS[0] - 1, 513]
        rows, _ = _xopen(hades_lib, torch_cuda, h, parts, idx, 10, ARITY)
    _same(tree, root, want_tree, want_root)
    assert all(to_host(p[0]).tobytes() == b.tobytes() for p, b in zip(parts, before))               # the absorb never writes to them
    assert not (rows == SENTINEL).any()
    assert rows.tobytes() == np.stack([MM.flat_rows(MM.open_rows(groups, i)) for i in idx]).tobytes()


def test_null_layouts_are_the_column_major_call(hades_lib, torch_cuda, tall):
    """layouts = NULL through _ex against hades252_dmmcs_absorb on the same column-major parts: the same trees and roots
    (k_rm_absorb against k_dmmcs_absorb), strides above the height."""
    groups, want_tree, want_root = tall
    parts = [_mat_dev(torch_cuda, g, COLS_, g.shape[0] + 1 + i) for i, g in enumerate(groups)]
    got = []
    for ex in (True, False):
        with _handle(hades_lib) as h:
            if ex:
                assert _xabsorb(hades_lib, h, parts, layouts=False) == 0
            else:
                assert _dabsorb(hades_lib, h, [(p[0], p[1]) for p in parts]) == 0
            torch_cuda.cuda.synchronize()
            got.append(_commit(hades_lib, h, HEIGHTS[0], ARITY, 1))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    _same(*got[0], want_tree, want_root)


def test_host_and_device_in_both_layouts_feed_one_handle(hades_lib, torch_cuda, tall):
    torch = torch_cuda
    groups, want_tree, want_root = tall
    with _handle(hades_lib) as h:
        _rabsorb(hades_lib, h, groups[0], 3)                                     # the tallest group from host rows: synchronous
        _absorb(hades_lib, h, groups[3][:, :1])                                  # one group from all four sources
        _rabsorb(hades_lib, h, groups[3][:, 1:2], 2)
        assert _xabsorb(hades_lib, h, [_mat_dev(torch, groups[1], ROWS_), _mat_dev(torch, groups[2], COLS_),
                                       _mat_dev(torch, groups[3][:, 2:3], COLS_)] +
                        [_mat_dev(torch, g, ROWS_ if i % 2 else COLS_) for i, g in enumerate(groups[4:-1])]) == 0
        assert _xabsorb(hades_lib, h, [_mat_dev(torch, groups[3][:, 3:], ROWS_, 5)]) == 0
        torch.cuda.synchronize()                                                 # before the next host-form call
        _rabsorb(hades_lib, h, groups[-1])
        _same(*_commit(hades_lib, h, HEIGHTS[0], ARITY, 1), want_tree, want_root)


# ---- 3. a refused call changes nothing ---------------------------------------------------------------------------------
def test_a_refused_call_between_two_good_ones_leaves_the_root_what_it_would_have_been(hades_lib, torch_cuda, tall):
    groups, want_tree, want_root = tall
    parts = [_mat_dev(torch_cuda, g, ROWS_ if i % 2 else COLS_) for i, g in enumerate(groups)]
    n = ctypes.c_uint64()
    with _handle(hades_lib) as h:
        assert _xabsorb(hades_lib, h, parts[:4]) == 0
        for bad in ([parts[4], parts[5], parts[6][:4] + (2,)],                                       # a layout that is none
                    [parts[4], parts[5][:3] + (parts[5][2] - 1, ROWS_), parts[6]],                   # a row stride below the width
                    [parts[6], parts[5], (parts[4][0], parts[6][1]) + parts[4][2:]]):                # a height twice
            assert _xabsorb(hades_lib, h, bad) == INVALID
            for g in groups[4:7]:
                assert hades_lib.hades252_mmcs_cols(h, g.shape[0], ctypes.byref(n)) == 0 and n.value == 0   # nothing created or moved
        assert _xabsorb(hades_lib, h, parts[4:]) == 0
        torch_cuda.cuda.synchronize()
        _same(*_commit(hades_lib, h, HEIGHTS[0], ARITY, 1), want_tree, want_root)


# ---- 4. openings -------------------------------------------------------------------------------------------------------
def test_open_equals_the_model_and_the_column_major_opening(hades_lib, torch_cuda, tall):
    """Every leaf index of the 2^10 shape, repeated and unsorted ones, h_0 and 2^63 (zeros), the layouts alternating."""
    torch = torch_cuda
    groups, want_tree, _ = tall
    h0 = HEIGHTS[0]
    idx = list(range(h0)) + [7, 7, h0 - 1, 0, 7] + [h0, 1 << 63]
    good = len(idx) - 2
    want_rows = np.zeros((len(idx), sum(COLS), 4), dtype=np.uint64)
    want_rows[:good] = np.stack([MM.flat_rows(MM.open_rows(groups, i)) for i in idx[:good]])
    want_paths = MM.open_paths(want_tree, h0, ARITY, idx)
    assert not want_paths[good:].any()
    parts = [_mat_dev(torch, g, COLS_ if i % 2 else ROWS_, (g.shape[0] if i % 2 else g.shape[1]) + i % 3) for i, g in enumerate(groups)]
    twins = [_planes_dev(torch, g) for g in groups]
    with _handle(hades_lib) as h:
        assert _xabsorb(hades_lib, h, parts) == 0
        torch.cuda.synchronize()
        _commit(hades_lib, h, h0, ARITY, 1)
        rows, paths = _xopen(hades_lib, torch, h, parts, idx, 10, ARITY)
        assert rows.tobytes() == want_rows.tobytes() and paths.tobytes() == want_paths.tobytes()
        # hades252_dmmcs_open on the column-major twins writes the same bytes
        pl, rws, cols, strides = _tables(twins)
        d_idx = to_dev(torch, np.array(idx, dtype=np.uint64))
        r_big, r_ptr = _guarded_dev(torch, len(idx), sum(COLS))
        p_big, p_ptr = _guarded_dev(torch, len(idx), 10)
        assert hades_lib.hades252_dmmcs_open(h, _p(pl), _p(rws), _p(cols), _p(strides), len(twins), d_idx.data_ptr(), len(idx), r_ptr,
                                             p_ptr, None) == 0
        torch.cuda.synchronize()
        assert _intact_dev(r_big, len(idx)).tobytes() == rows.tobytes() and _intact_dev(p_big, len(idx)).tobytes() == paths.tobytes()
        # a subset of the groups (the tallest and two more), and no query at all
        rows, paths = _xopen(hades_lib, torch, h, [parts[0], parts[3], parts[10]], idx[:65], 10, ARITY)
        assert paths.tobytes() == want_paths[:65].tobytes()
        assert rows.tobytes() == np.concatenate([want_rows[:65, :1], want_rows[:65, 6:10], want_rows[:65, 55:66]], axis=1).tobytes()
        pl, rws, cols, strides, lay = _ex_tables(parts)
        assert hades_lib.hades252_rmmcs_open_ex(h, _p(pl), _p(rws), _p(cols), _p(strides), _p(lay), len(parts), None, 0, None, None, None) == 0


# ---- 5. the whole pipeline on a stream of its own ------------------------------------------------------------------------
def test_absorb_commit_open_verify_on_a_non_default_stream(hades_lib, H, torch_cuda, tall):
    """Rows from hades252_rmmcs_open_ex and its paths through hades252_dmmcs_verify: every root is the committed root.  The
    row-major parts are narrowed views of wider matrices."""
    torch = torch_cuda
    groups, want_tree, want_root = tall
    rng = np.random.default_rng(16)
    idx = rng.integers(0, HEIGHTS[0], size=300, dtype=np.uint64)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    L = H._lib
    layouts = [L.LAYOUT_ROWS if i % 2 == 0 else L.LAYOUT_COLS for i in range(len(groups))]
    parts = [to_dev(torch, RM.rows_of(g, g.shape[1] + 2)).view(g.shape[0], -1, 4)[:, :g.shape[1]] if l == L.LAYOUT_ROWS else
             _planes_dev(torch, g)[0] for g, l in zip(groups, layouts)]
    assert not parts[2].is_contiguous() and parts[2].stride() == (4 * 5, 4, 1)
    d_idx = to_dev(torch, idx)
    torch.cuda.synchronize()
    with H.Mmcs(CAP) as mc, torch.cuda.stream(s):
        assert torch.cuda.current_stream() == s and s != torch.cuda.default_stream()
        mc.absorb_dev(parts[:5], layouts[:5]).absorb_dev(parts[5:], layouts[5:])
        s.synchronize()                                                          # before the host-form commit
        tree, root = mc.commit(ARITY, TAG[ARITY], INJECT)
        rows_t, paths_t = mc.open_dev(parts, d_idx, layouts)
        roots_t = H.mmcs_verify_dev(rows_t, HEIGHTS, COLS, d_idx, paths_t, ARITY, CAP, TAG[ARITY], INJECT)
        assert torch.cuda.default_stream().query()                               # nothing went to the default stream
        s.synchronize()
        _same(tree, root, want_tree, want_root)
        assert to_host(roots_t).tobytes() == np.tile(want_root, (idx.size, 1)).tobytes()
        assert to_host(paths_t).tobytes() == MM.open_paths(want_tree, HEIGHTS[0], ARITY, idx.tolist()).tobytes()
        assert to_host(rows_t).tobytes() == np.stack([MM.flat_rows(MM.open_rows(groups, int(i))) for i in idx]).tobytes()


# ---- 6. the host form's tiles --------------------------------------------------------------------------------------------
_TILE_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from hades252_amd import build, strategy as H
build.build(verbose=False)
assert os.environ["HADES252_TEST_MATRIX_CHUNK_ROWS"] == "256" and int(os.environ["HADES252_TEST_MATRIX_CHUNK_COLS"]) >= 1
src, dst, cap, tag, inject = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
rows = np.fromfile(src, dtype=np.uint64).reshape(1024 + 64, 14, 4)
tall, short = np.ascontiguousarray(rows[:1024]), np.ascontiguousarray(rows[1024:])
with H.Mmcs(cap) as mc:
    mc.absorb_rows(tall[:, :5].copy(), 2)           # five scalars per row, two of them columns
    mc.absorb_rows(short, 6)
    mc.absorb_rows(tall[:, 2:].copy(), 9)           # the open block holds two columns; row stride 12
    tree, root = mc.commit(2, tag, inject)
    print("TILED", mc.cols(1024), mc.cols(64), tree.shape[0])
np.concatenate([tree.reshape(-1), root]).tofile(dst)
"""


@pytest.mark.parametrize("tile_cols", [1, 3, 4])
def test_host_tiles_give_the_column_major_tree(hades_lib, oracle, tmp_path, tile_cols):
    """HADES252_TEST_MATRIX_CHUNK_ROWS = 256 and HADES252_TEST_MATRIX_CHUNK_COLS, the tile hooks of the streams (read once by
    the library, hence a child process): 1024 rows are four row tiles; 11 columns absorbed as (2, 9) from rows 14 and 12
    scalars apart are column tiles of one column, of three (partial blocks at both ends of a tile) and of four (the first tile
    of the second call is shortened to the two columns the open block still takes; then whole blocks; then a tail): every tile
    a pitched copy.  The same tree as the column-major host call without tiles."""
    a, b = oracle.gen_b(91000, 1024 * 11).reshape(1024, 11, 4), oracle.gen_b(92000, 64 * 6).reshape(64, 6, 4)
    with _handle(hades_lib) as h:
        _absorb(hades_lib, h, a)
        _absorb(hades_lib, h, b)
        want_tree, want_root = _commit(hades_lib, h, 1024, 2, 1)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([RM.rows_of(a, 14), RM.rows_of(b, 14)]).tofile(src)
    env = dict(os.environ, HADES252_TEST_MATRIX_CHUNK_ROWS="256", HADES252_TEST_MATRIX_CHUNK_COLS=str(tile_cols))
    run = subprocess.run([sys.executable, "-c", _TILE_CHILD, str(src), str(dst), str(CAP), str(TAG[2]), str(INJECT)], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "TILED 11 6 %d" % want_tree.shape[0] in run.stdout, run.stdout[-1500:] + run.stderr[-3000:]
    assert np.fromfile(dst, dtype=np.uint64).tobytes() == np.concatenate([want_tree.reshape(-1), want_root]).tobytes()


# ---- 7. argument rules ---------------------------------------------------------------------------------------------------
def test_argument_rules_on_a_live_handle(hades_lib):
    import test_rowmajor_abi
    test_rowmajor_abi.rules_that_need_a_handle(hades_lib)


def test_python_wrappers_refuse_wrong_shapes_before_the_library(H, torch_cuda, monkeypatch):
    import test_rowmajor_abi
    test_rowmajor_abi.wrappers_refuse_wrong_shapes(torch_cuda, H, monkeypatch)


# ---- 8. resources --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["k_rm_absorb", "k_rm_rows"])
def test_kernels_have_no_scratch_and_fit_their_bounds(hades_lib, kernel):
    """By the code object's metadata only: one instance each (neither is templated), no scratch, no spill, registers within
    the budget of the launch bounds, and the LDS the shipped source declares: none."""
    co = codeobj.load()
    names = co.kernels(kernel)
    assert len(names) == 1, sorted(co.meta)
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "kernels_rowmajor.hpp")) as f:
        src = f.read()
    minw = int(re.search(r"__launch_bounds__\(kBlock, (\d+)\) %s\(" % kernel, src).group(1))
    budget = VGPRS_PER_SIMD // minw // 8 * 8             # __launch_bounds__(256, minw): minw waves per SIMD share 512 registers
    assert minw == 3 and budget == 168
    r = co.meta[names[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    # scalar registers parked in lanes of a vector register (no memory): the permutation's, so no more than the sibling has
    sibling = co.meta[co.kernels({"k_rm_absorb": "k_dmmcs_absorb", "k_rm_rows": "k_dmmcs_rows"}[kernel])[0]]
    assert r.get("sgpr_spill_count", 0) <= sibling.get("sgpr_spill_count", 0), (r, sibling)
    assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] + r["agpr_count"] <= budget, (r, budget)
    assert "__shared__" not in src and r["group_segment_fixed_size"] == 0
    print("%s: %d VGPRs, %d AGPRs, %d SGPRs, LDS %d" % (names[0], r["vgpr_count"], r["agpr_count"], r["sgpr_count"],
                                                      r["group_segment_fixed_size"]))
