"""CPU tier: the shipped kernel of hades252_amd/csrc/kernels_matrix.hpp (k_sponge_planes) runs on the CPU under ASan + UBSan,
bit-exact against the model (tests/matrix_model.py: the C oracle's sponge of the transposed matrix) -- before any GPU sees it.

tests/hostsim_matrix/matrix_main.cpp is a stand-alone program (its own main) over the block emulator of
tests/hostsim/hip/hip_runtime.h and the tree's headers as tests/hostsim_lib.py copies them (rewritten(): the allow-list of
semantically empty edits; check_copy() refuses anything else).  It is built with hostsim_lib's compiler and its "asan" flags
and run as an ordinary child process: nothing is preloaded, nothing is loaded into this interpreter.  The planes are a heap
block that ends with the last row of the last plane, the gaps between planes are poisoned, the digests are a heap block of
exactly n_rows * 32 bytes: a read past a plane's last row or a store past the last digest is an ASan report.  An emulated
block takes seconds, so the cases are few."""
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
import oracle_lib  # noqa: E402
from gpu_common import CAP  # noqa: E402

HERE = os.path.join(ROOT, "tests", "hostsim_matrix")
MAIN = os.path.join(HERE, "matrix_main.cpp")


@pytest.fixture(scope="module")
def exe():
    """The driver under ASan + UBSan; rebuilt when the driver, the stand-in, a copied header or the flags change."""
    return HS.build_driver(MAIN, "matrix_main")


def _exact_planes(matrix, stride):
    """The planes as one flat buffer that ends with the last row of the last plane."""
    n_rows, n_cols = matrix.shape[0], matrix.shape[1]
    return M.planes_of(matrix, stride).reshape(-1)[:((n_cols - 1) * stride + n_rows) * 4]


def _run(exe, tmp_path, matrix, stride, pad_mode, cap=CAP, check=True):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(_exact_planes(matrix, stride).tobytes())
    n_rows, n_cols = matrix.shape[0], matrix.shape[1]
    r = subprocess.run([exe, str(src), str(dst), str(n_rows), str(n_cols), str(stride), str(pad_mode)] +
                       [str(v) for v in oracle_lib.limbs_of(cap)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **HS.SAN_ENV))
    if not check:
        return r
    assert r.returncode == 0, "matrix_main exited %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    return np.frombuffer(dst.read_bytes(), dtype=np.uint64)


def test_driver_defines_no_device_routine_and_launches_with_the_call_sites_geometry():
    with open(MAIN) as f:
        main = HS._strip_comments(f.read())
    assert "__global__" not in main and "__device__" not in main and not re.search(r"\basm\b", main)
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", main) == ["k_sponge_planes"]
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "host_matrix.hpp")) as f:
        host = f.read()
    # the call site: one block of kBlock lanes per kBlock rows of the chunk, no LDS; the chunk's plane stride is K
    assert ("hipLaunchKernelGGL(k_sponge_planes, dim3(blocks_for(m)), dim3(kBlock), 0, pp.s_k, d, m, n_cols, K, d_dig + off * 32, "
            "cap, pad_mode);") in host
    assert "hipLaunchKernelGGL(k_sponge_planes, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0," in main
    assert "m, n_cols, stride, digests, cap, pad_mode);" in main


@pytest.mark.parametrize("n_rows,n_cols,stride,pad_mode", [(1, 1, 1, 1), (65, 5, 65, 0), (65, 5, 65, 1), (257, 4, 300, 1)])
def test_row_digests_equal_the_models(exe, tmp_path, oracle, n_rows, n_cols, stride, pad_mode):
    """One lane; a full wave and one lane of the next with a ragged last block of columns (5 = 4 + 1; the pad scalar joins
    it); two blocks with a gap between the planes, where the pad scalar opens a block of its own."""
    m = oracle.gen_b(15000 + n_rows, n_rows * n_cols).reshape(n_rows, n_cols, 4)
    if n_rows > 2:
        m[0], m[n_rows - 1, n_cols - 1] = 0, np.array(oracle_lib.limbs_of(oracle_lib.P - 1), dtype=np.uint64)
    got = _run(exe, tmp_path, m, stride, pad_mode)
    assert got.tobytes() == M.row_digests(oracle, m, CAP, pad_mode).tobytes()

