"""CPU tier: the shipped kernels of hades252_amd/csrc/kernels_matrix_stream.hpp (k_planes_init, k_planes_absorb,
k_planes_finish) run on the CPU under ASan + UBSan, bit-exact against the model (tests/matrix_stream_model.py: the oracle's
permutation and additions modulo p) -- before any GPU sees them.

tests/hostsim_matrix_stream/stream_main.cpp is a stand-alone program (its own main) over the block emulator of
tests/hostsim/hip/hip_runtime.h and the tree's headers as tests/hostsim_lib.py copies them (rewritten(): the allow-list of
semantically empty edits; check_copy() refuses anything else).  It is built with hostsim_lib's compiler and its "asan" flags
and run as an ordinary child process: nothing is preloaded, nothing is loaded into this interpreter.  The state planes and
the digests are heap blocks of exactly their size, the planes of a group end with the last row of the last plane and the gaps
between planes are poisoned: an access past a plane's last row, a state word of a row past the last or a store past the last
digest is an ASan report.  An emulated block takes seconds, so the cases are few."""
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
import oracle_lib  # noqa: E402
from gpu_common import CAP  # noqa: E402

HERE = os.path.join(ROOT, "tests", "hostsim_matrix_stream")
MAIN = os.path.join(HERE, "stream_main.cpp")


@pytest.fixture(scope="module")
def exe():
    """The driver under ASan + UBSan; rebuilt when the driver, the stand-in, a copied header or the flags change."""
    return HS.build_driver(MAIN, "stream_main")


def _exact_planes(group, stride):
    """The planes of a group [n_rows, g, 4] as one flat buffer that ends with the last row of the last plane."""
    n_rows, g = group.shape[0], group.shape[1]
    return M.planes_of(group, stride).reshape(-1)[:((g - 1) * stride + n_rows) * 4]


def _run(exe, tmp_path, groups, strides, pad_mode, cap=CAP):
    """-> (state planes [5, n_rows, 4] after every group, digests [n_rows, 4], state planes after the finish)."""
    n_rows = groups[0].shape[0]
    args = [exe, str(tmp_path / "out"), str(n_rows), str(pad_mode)] + [str(v) for v in oracle_lib.limbs_of(cap)]
    for i, (g, stride) in enumerate(zip(groups, strides)):
        src = tmp_path / ("in%d.bin" % i)
        src.write_bytes(_exact_planes(g, stride).tobytes())
        args += [str(src), str(g.shape[1]), str(stride)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env=dict(os.environ, **HS.SAN_ENV))
    assert r.returncode == 0, "stream_main exited %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])

    def read(name, shape):
        a = np.frombuffer((tmp_path / ("out." + name)).read_bytes(), dtype=np.uint64)
        return a.reshape(shape)

    states = [read("state.%d" % i, (5, n_rows, 4)) for i in range(len(groups))]
    return states, read("digests", (n_rows, 4)), read("state.end", (5, n_rows, 4))


def test_driver_defines_no_device_routine_and_launches_with_the_call_sites_geometry():
    with open(MAIN) as f:
        main = HS._strip_comments(f.read())
    assert "__global__" not in main and "__device__" not in main and not re.search(r"\basm\b", main)
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", main) == ["k_planes_init", "k_planes_absorb", "k_planes_finish"]
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "host_matrix_stream.hpp")) as f:
        host = f.read()
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", host) == ["k_planes_absorb", "k_planes_finish", "k_planes_init"]
    # the call sites: one block of kBlock lanes per kBlock rows, no LDS; a tile's plane stride is K, the state's is S
    assert ("hipLaunchKernelGGL(k_planes_absorb, dim3(blocks_for(m)), dim3(kBlock), 0, pp.s_k, ms->d_state + off * 32, S, m, d, gw, "
            "K, (int)cur);") in host
    assert ("hipLaunchKernelGGL(k_planes_finish, dim3(blocks_for(S)), dim3(kBlock), 0, pp.s_k, ms->d_state, S, S, ms->d_dig, "
            "(int)(ms->n_cols % 4), pad_mode);") in host
    assert ("hipLaunchKernelGGL(k_planes_init, dim3(blocks_for(n_rows)), dim3(kBlock), 0, call.pipe.s_k, ms->d_state, n_rows, "
            "n_rows,") in host
    main = re.sub(r"\s+", " ", main)
    assert ("hipLaunchKernelGGL(k_planes_absorb, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, "
            "state, S, m, d, gw, K, (int)cur);") in main
    assert ("hipLaunchKernelGGL(k_planes_finish, dim3((unsigned)((S + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, "
            "state, S, S, digests, (int)(total % 4), pad_mode);") in main
    assert ("hipLaunchKernelGGL(k_planes_init, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, "
            "(hipStream_t) nullptr, state, n_rows, n_rows, cap);") in main


@pytest.mark.parametrize("n_rows,groups,strides,pad_mode", [
    (1, (1,), (1,), 1),                          # one lane, one column
    (65, (2, 3), (65, 65), 0),                   # a full wave and one lane: a head (2 + 2 closes the block), no body, a tail
    (65, (2, 3), (65, 65), 1),                   # ... and the pad scalar joins the open block
    (257, (3, 5, 4), (300, 257, 260), 1),        # two blocks of lanes: a head that closes a block, a body, a tail; gaps between
])                                               # the planes; the pad scalar opens a block of its own (12 columns)
def test_states_and_digests_equal_the_models(exe, tmp_path, oracle, n_rows, groups, strides, pad_mode):
    total = sum(groups)
    m = oracle.gen_b(17000 + n_rows, n_rows * total).reshape(n_rows, total, 4).copy()
    if n_rows > 2:
        m[0], m[n_rows - 1, total - 1] = 0, np.array(oracle_lib.limbs_of(oracle_lib.P - 1), dtype=np.uint64)
    parts = MS.split(m, groups)
    states, digests, end = _run(exe, tmp_path, parts, strides, pad_mode)
    model = MS.Stream(oracle, n_rows)
    for i, part in enumerate(parts):
        model.absorb(part)
        assert states[i].tobytes() == model.state_planes().tobytes(), "state after group %d" % i
    assert digests.tobytes() == model.digests(pad_mode).tobytes() == M.row_digests(oracle, m, CAP, pad_mode).tobytes()
    assert end.tobytes() == states[-1].tobytes()                       # the finish does not write the state
