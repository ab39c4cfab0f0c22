"""CPU tier: the shipped kernels of hades252_amd/csrc/kernels_inverse.hpp run on the CPU under ASan + UBSan, bit-exact
against the big-integer model (tests/perm_inverse_model.py) -- before any GPU sees them.

tests/hostsim_inverse/inverse_main.cpp is a stand-alone program (its own main) over the block emulator of
tests/hostsim/hip/hip_runtime.h and the tree's headers as tests/hostsim_lib.py copies them (rewritten(): the allow-list of
semantically empty edits; check_copy() refuses anything else).  It is built with hostsim_lib's compiler and its "asan" flags
and run as an ordinary child process on heap buffers of exactly the data's size: nothing is preloaded, nothing is loaded
into this interpreter.  An emulated block takes seconds, so the cases are few."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import perm_inverse_model as M  # noqa: E402

HERE = os.path.join(ROOT, "tests", "hostsim_inverse")
MAIN = os.path.join(HERE, "inverse_main.cpp")
S, P = M.S, M.P


@pytest.fixture(scope="module")
def exe():
    """The driver under ASan + UBSan; rebuilt when the driver, the stand-in, a copied header or the flags change."""
    return HS.build_driver(MAIN, "inverse_main")


def _run(exe, tmp_path, what, data, n, *rounds):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.ascontiguousarray(data, dtype=np.uint64).tobytes())
    r = subprocess.run([exe, what, str(src), str(dst), str(n)] + [str(v) for v in rounds], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **HS.SAN_ENV))
    assert r.returncode == 0, "inverse_main exited %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    return np.frombuffer(dst.read_bytes(), dtype=np.uint64)


def _states(n, seed):
    """n states of canonical integers, the first few of them edge values."""
    rng = np.random.default_rng(seed)
    vals = [[int.from_bytes(rng.bytes(32), "little") % P for _ in range(5)] for _ in range(n)]
    for k, v in enumerate((0, 1, P - 1)):
        if k < n:
            vals[k] = [v] * 5
    return vals


def test_driver_defines_no_device_routine_and_launches_with_the_call_sites_geometry():
    with open(MAIN) as f:
        main = HS._strip_comments(f.read())
    assert "__global__" not in main and "__device__" not in main and "asm" not in main
    assert set(re.findall(r"hipLaunchKernelGGL\((\w+)", main)) == {"k_perm_inverse", "k_fifth_root"}
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "host_inverse.hpp")) as f:
        host = f.read()
    # the call sites: one block of kBlock lanes per kBlock records; the state kernel asks for lds_for(5) =
    # kWavesPerBlock * lds_wave_bytes(5) bytes (launch.hpp), the scalar kernel for none
    assert "hipLaunchKernelGGL(k_fifth_root, dim3(blocks_for(m)), dim3(kBlock), 0, pp.s_k, d, m);" in host
    assert "hipLaunchKernelGGL(k_perm_inverse, dim3(blocks_for(m)), dim3(kBlock), lds_for(5), pp.s_k, d, m, round_hi, round_lo);" in host
    assert "hipLaunchKernelGGL(k_fifth_root, grid, block, 0," in main
    assert "hipLaunchKernelGGL(k_perm_inverse, grid, block, (size_t)kWavesPerBlock * lds_wave_bytes(5)," in main
    assert "dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);" in main


def test_whole_inverse_of_one_state(exe, tmp_path):
    x = [3, P - 2, 1 << 200, 0, 5]
    y = S.perm(x)
    got = _run(exe, tmp_path, "rounds", M.states_of([y]), 1, 67, 0)
    assert got.tobytes() == M.states_of([x]).tobytes()
    assert M.perm_inverse(y) == x


@pytest.mark.parametrize("hi,lo", [(67, 64), (5, 3)])
def test_round_ranges_over_two_blocks_worth_of_waves(exe, tmp_path, hi, lo):
    """n = 65: a full wave and one lane of the next; the ranges cross a full/partial switch each."""
    n = 65
    ins = _states(n, 1000 * hi + lo)
    want = [M.inverse_rounds(st, hi, lo) for st in ins]
    got = _run(exe, tmp_path, "rounds", M.states_of(ins), n, hi, lo)
    assert got.tobytes() == M.states_of(want).tobytes()
    # the model agrees with the forward rounds of round_inverse on one of them
    import round_inverse as RI
    st = want[7]
    for r in range(lo, hi):
        st = RI.round_fwd(st, r)
    assert st == ins[7]


def test_fifth_roots_of_the_edge_values(exe, tmp_path):
    vals = [0, 1, P - 1]
    got = _run(exe, tmp_path, "root", M.scalars_of(vals), 3)
    assert got.tobytes() == M.scalars_of([M.fifth_root(v) for v in vals]).tobytes()
    assert [pow(v, 5, P) for v in M.values_of(got)] == vals
