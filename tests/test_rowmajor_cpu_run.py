"""CPU tier: the shipped kernels of hades252_amd/csrc/kernels_rowmajor.hpp (k_rm_absorb, k_rm_rows) run on the CPU under
ASan + UBSan, bit-exact against the models of the COLUMN-major paths (tests/matrix_stream_model.py: the row states through the
oracle's permutation; tests/mmcs_model.py: the opened rows) -- before any GPU sees them.  Absorbing a row-major matrix is
defined as absorbing the column-major matrix with the same entries, so there is no model of its own.

tests/hostsim_rowmajor/rowmajor_main.cpp is a stand-alone program (its own main) over the block emulator of
tests/hostsim/hip/hip_runtime.h and the tree's headers as tests/hostsim_lib.py copies them.  It is built with hostsim_lib's
compiler and its "asan" flags and run as an ordinary child process: nothing is preloaded, nothing is loaded into this
interpreter.  Every buffer is a heap block of exactly its size -- a row-major matrix ends with the last scalar of its last
row -- and the gap behind a row's width (a plane's height) is poisoned: a read past a row's width is an ASan report.  An
emulated block takes seconds, so the cases are few."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import matrix_model as M  # noqa: E402
import matrix_stream_model as MS  # noqa: E402
import mmcs_model as MM  # noqa: E402
import oracle_lib  # noqa: E402
import rowmajor_model as RM  # noqa: E402
from rowmajor_model import LAYOUT_COLS, LAYOUT_ROWS  # noqa: E402

HERE = os.path.join(ROOT, "tests", "hostsim_rowmajor")
MAIN = os.path.join(HERE, "rowmajor_main.cpp")
# (columns already in the open block, columns of the part): the head stays open (twice), the head closes, two body blocks
# and a tail of one (the prefetch), a head that closes, a body block and a tail
COMBOS = [(0, 1), (1, 1), (3, 1), (0, 9), (2, 7)]
GAP = 3                                   # scalars between a row's last column (a plane's last row) and the next one


@pytest.fixture(scope="module")
def exe():
    """The driver under ASan + UBSan; rebuilt when the driver, the stand-in, a copied header or the flags change."""
    return HS.build_driver(MAIN, "rowmajor_main", "asan")


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env=dict(os.environ, **HS.SAN_ENV))
    assert r.returncode == 0, "rowmajor_main exited %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])


def _laid(m, layout):
    """Matrix [n_rows, g, 4] in `layout` with GAP scalars of sentinel behind every row (plane): (bytes up to its last
    scalar, stride)."""
    n_rows, g = m.shape[0], m.shape[1]
    if layout == LAYOUT_ROWS:
        return RM.exact(RM.rows_of(m, g + GAP), n_rows, g, layout), g + GAP
    return RM.exact(M.planes_of(m, n_rows + GAP), n_rows, g, layout), n_rows + GAP


def test_driver_defines_no_device_routine_and_launches_with_the_call_sites_geometry():
    with open(MAIN) as f:
        main = HS._strip_comments(f.read())
    assert "__global__" not in main and "__device__" not in main and not re.search(r"\basm\b", main)
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", main) == ["k_rm_absorb", "k_rm_rows"]
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "abi_rowmajor.hpp")) as f:
        host = re.sub(r"\s+", " ", HS._strip_comments(f.read()))
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", host) == ["k_rm_absorb", "k_rm_rows"]
    main = re.sub(r"\s+", " ", main)
    for launch in ("hipLaunchKernelGGL(k_rm_absorb, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, "
                   "(uint32_t)n_live);",
                   "hipLaunchKernelGGL(k_rm_rows, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, table, "
                   "(uint32_t)n_parts, d_indices, n_queries, (uint64_t)h0, row_cols, (uint8_t *)d_rows);"):
        assert launch in host and launch in main, launch
    # the grid is the blocks of all parts laid end to end, counted the same way on both sides
    assert "table.first_block[i] = (uint32_t)n_blocks;" in host and "table.first_block[i] = (uint32_t)n_blocks;" in main
    assert "table.first_block[p] = (uint32_t)n_blocks;" in host and "table.first_block[p] = (uint32_t)n_blocks;" in main
    assert "n_blocks += blocks_for((size_t)n_rows[p]);" in host and "n_blocks += (unsigned)((n_rows + kBlock - 1) / kBlock);" in main
    assert "n_blocks += blocks_for(n_queries * (size_t)n_cols[p]);" in host
    assert "n_blocks += (unsigned)((n_queries * cols + kBlock - 1) / kBlock);" in main
    # the two steps of a layout, the same on both sides: (1, stride) column-major, (stride, 1) row-major
    assert "*row_step = 1; *col_step = stride;" in host and "*row_step = stride; *col_step = 1;" in host
    assert "m.row_step = 1; m.col_step = stride;" in main and "m.row_step = stride; m.col_step = 1;" in main
    assert "table.rows[i] = n_rows[p];" in host and "table.S[i] = n_rows[p];" in host                # a whole group per part
    assert "table.rows[i] = n_rows;" in main and "table.S[i] = n_rows;" in main
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "kernels_rowmajor.hpp")) as f:
        kernels = HS._strip_comments(f.read())
    assert "__shared__" not in kernels and "__syncthreads" not in kernels and not re.search(r"\basm\b", kernels)
    assert len(re.findall(r"__launch_bounds__\(kBlock, 3\)", kernels)) == 2 == len(re.findall(r"__global__", kernels))


def test_absorb_body_is_the_streams_body_but_for_the_address():
    """k_rm_absorb holds a copy of k_planes_absorb's body: once the stream's address of column x, planes + (x * stride +
    row) * 32, is written as at + x * step, the two are the same text from the state loads to the state stores."""
    def body(name, kernel):
        with open(os.path.join(ROOT, "hades252_amd", "csrc", name)) as f:
            text = f.read().split("%s(" % kernel)[1]
        text = text[text.index("    Fr st[5];"):]
        return re.sub(r"//[^\n]*", "", text[:text.index("\n}\n")]).replace("group", "part")
    stream = re.sub(r"planes \+ \((\(.*?\)) \* stride \+ row\) \* 32", r"at + \1 * step", body("kernels_matrix_stream.hpp", "k_planes_absorb"))
    assert "stride" not in stream and stream.count("at + ") == 4
    assert body("kernels_rowmajor.hpp", "k_rm_absorb") == stream


def _absorb_case(exe, tmp_path, oracle, shape, turn):
    """One launch over parts of the heights `shape` (shortest first, as the call site lays them); part i takes combo
    (turn + i) % 5 and the layout ROWS / COLS / ROWS on even turns, COLS / ROWS / COLS on odd ones.  Row 0 of every matrix
    is zero and its last row p - 1 (a matrix of one row: zero in the one-part shape, p - 1 else)."""
    args, want = [exe, "absorb", str(tmp_path / ("out%d" % turn)), str(len(shape))], []
    for i, n_rows in enumerate(shape):
        cur, g = COMBOS[(turn + i) % len(COMBOS)]
        layout = LAYOUT_ROWS if (turn + i) % 2 == 0 else LAYOUT_COLS
        m = oracle.gen_b(60000 + 1000 * turn + 100 * i + n_rows, n_rows * (cur + g)).reshape(n_rows, cur + g, 4).copy()
        m[0] = 0
        if n_rows > 1 or len(shape) > 1:
            m[n_rows - 1] = np.array(oracle_lib.limbs_of(oracle_lib.P - 1), dtype=np.uint64)
        model = MS.Stream(oracle, n_rows).absorb(m[:, :cur])
        before = model.state_planes().copy()
        want.append(model.absorb(m[:, cur:]).state_planes())
        data, stride = _laid(m[:, cur:], layout)
        state_f, mat_f = tmp_path / ("state%d_%d.bin" % (turn, i)), tmp_path / ("mat%d_%d.bin" % (turn, i))
        state_f.write_bytes(before.tobytes())
        mat_f.write_bytes(data)
        args += [str(state_f), str(mat_f), str(n_rows), str(g), str(stride), str(cur), str(layout)]
    _run(args)
    for i, w in enumerate(want):
        got = (tmp_path / ("out%d.state.%d" % (turn, i))).read_bytes()
        assert got == w.tobytes(), (shape, turn, i, COMBOS[(turn + i) % len(COMBOS)])


@pytest.mark.parametrize("turn", range(len(COMBOS)))
def test_one_part_of_one_row_equals_the_model(exe, tmp_path, oracle, turn):
    _absorb_case(exe, tmp_path, oracle, (1,), turn)


@pytest.mark.parametrize("turn", range(len(COMBOS)))
def test_three_parts_of_mixed_layouts_in_one_launch_equal_the_model(exe, tmp_path, oracle, turn):
    """1 / 65 / 257 rows: a lone lane, a ragged block, two blocks plus a ragged one -- five blocks, three parts, every part
    with another (cur, columns) and the layouts alternating; over the five turns every part meets every combination."""
    _absorb_case(exe, tmp_path, oracle, (1, 65, 257), turn)


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_rows_equal_the_model(exe, tmp_path, oracle, case, n):
    """n queries that walk over every leaf of a fixture shape (arities 2, 4 and 3), then index = h_0 and index = 2^63: the
    model's opened rows, and zeros for the two.  The layouts alternate over the groups, the tallest row-major."""
    arity, heights, cols, _, _, first = MM.GOLDEN_CASES[case]
    groups = MM.golden_groups(oracle, heights, cols, first)
    h0 = heights[0]
    idx = [(5 * t + 1) % h0 for t in range(n)] + [h0, 1 << 63]
    assert n < h0 or set(idx[:n]) == set(range(h0))
    want = np.zeros((len(idx), sum(cols), 4), dtype=np.uint64)
    for t, i in enumerate(idx[:n]):
        want[t] = MM.flat_rows(MM.open_rows(groups, i))
    (tmp_path / "idx.bin").write_bytes(np.array(idx, dtype=np.uint64).tobytes())
    out = tmp_path / "rows.bin"
    args = [exe, "rows", str(out), str(len(idx)), str(h0), str(tmp_path / "idx.bin"), str(len(groups))]
    for g, m in enumerate(groups):
        layout = LAYOUT_ROWS if g % 2 == 0 else LAYOUT_COLS
        data, stride = _laid(m, layout)
        f = tmp_path / ("mat%d.bin" % g)
        f.write_bytes(data)
        args += [str(f), str(m.shape[0]), str(m.shape[1]), str(stride), str(layout)]
    _run(args)
    assert out.read_bytes() == want.tobytes()
