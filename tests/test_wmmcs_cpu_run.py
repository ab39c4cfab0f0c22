"""CPU tier: the shipped kernel of hades252_amd/csrc/kernels_wmmcs.hpp (k_mmcs_inputs) run on the CPU under ASan + UBSan,
bit-exact against the model (tests/mmcs_witness_model.py: the chain of every opening through the oracle's permutation) --
before any GPU sees it.

tests/hostsim_wmmcs/wmmcs_main.cpp is a stand-alone program (its own main) over the block emulator of
tests/hostsim/hip/hip_runtime.h and the tree's headers as tests/hostsim_lib.py copies them (rewritten(): the allow-list of
semantically empty edits; check_copy() refuses anything else).  It is built with hostsim_lib's compiler and its "asan" flags
and run as an ordinary child process: nothing is preloaded, nothing is loaded into this interpreter.  Every buffer is a heap
block of exactly its size: a word past the inputs, the rows, the paths or the roots is an ASan report.  An emulated block
takes seconds, so the cases are few."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import mmcs_model as MM  # noqa: E402
import mmcs_witness_model as WM  # noqa: E402
import oracle_lib  # noqa: E402
from gpu_common import CAP, TAG  # noqa: E402

HERE = os.path.join(ROOT, "tests", "hostsim_wmmcs")
MAIN = os.path.join(HERE, "wmmcs_main.cpp")


@pytest.fixture(scope="module")
def exe():
    """The driver under ASan + UBSan; rebuilt when the driver, the stand-in, a copied header or the flags change."""
    return HS.build_driver(MAIN, "wmmcs_main")


def _limbs(v):
    return [str(x) for x in oracle_lib.limbs_of(v)]


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env=dict(os.environ, **HS.SAN_ENV))
    assert r.returncode == 0, "wmmcs_main exited %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])


def _one_line(text):
    return re.sub(r"\s+", " ", re.sub(r"\s*\\\n\s*", " ", HS._strip_comments(text)))


def test_driver_defines_no_device_routine_and_launches_with_the_call_sites_geometry():
    with open(MAIN) as f:
        main = HS._strip_comments(f.read())
    assert "__global__" not in main and "__device__" not in main and not re.search(r"\basm\b", main)
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", main) == ["k_mmcs_inputs"]
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "abi_wmmcs.hpp")) as f:
        host = _one_line(f.read())
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", host) == ["k_mmcs_inputs"]
    # the call site: one block of kBlock lanes per kBlock queries, no LDS; the driver spells blocks_for out
    launch = ("hipLaunchKernelGGL(k_mmcs_inputs<A>, dim3(%s), dim3(kBlock), 0, s, (const uint8_t *)d_rows, d_idx, "
              "(const uint8_t *)d_paths, n_queries, table, (uint32_t)n_groups, row_cols, depth, n_perms, pad_mode, cap, tag, inject_tag, "
              "out_idx, (uint8_t *)d_inputs, (uint8_t *)d_roots)")
    assert launch % "blocks_for(n_queries)" in host
    assert launch % "(unsigned)((n_queries + kBlock - 1) / kBlock)" in _one_line(main)
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "launch.hpp")) as f:
        assert "blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }" in f.read()
    for pick in ("case 2: HADES_LAUNCH_MMCS_INPUTS(2); break;", "case 3: HADES_LAUNCH_MMCS_INPUTS(3); break;",
                 "default: HADES_LAUNCH_MMCS_INPUTS(4); break;"):
        assert pick in host and pick in _one_line(main), pick
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "kernels_wmmcs.hpp")) as f:
        kernels = HS._strip_comments(f.read())
    assert len(re.findall(r"\bfast_perm<5>\(", kernels)) == 1 and "fast_perm<1>" not in kernels
    assert len(re.findall(r"__global__ void __launch_bounds__\(kBlock, 3\) k_mmcs_inputs\(", kernels)) == 1 == kernels.count("__global__")
    assert "__shared__" not in kernels and "__syncthreads" not in kernels and not re.search(r"\basm\b", kernels)
    assert "#pragma unroll 1\n    for (size_t t = 0; t < n_perms; t++) {" in kernels


def _case(exe, tmp_path, oracle, case, n, want_roots=True):
    """n openings of a fixture shape whose indices walk over every leaf (and so every position of every level); query 0
    opens an all-zero tallest row and the last query rows of p - 1."""
    arity, heights, cols, pad_mode, _, first = MM.GOLDEN_CASES[case]
    groups = [g.copy() for g in MM.golden_groups(oracle, heights, cols, first)]
    groups[0][0] = 0
    groups[-1][-1] = np.array(oracle_lib.limbs_of(oracle_lib.P - 1), dtype=np.uint64)
    tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    depth = MM.depth_of(heights[0], arity)
    idx = [(5 * t) % heights[0] for t in range(n - 1)] + [heights[0] - 1]             # (5 is prime to 8, 16 and 9)
    assert n < heights[0] or set(idx) == set(range(heights[0]))
    paths = MM.open_paths(tree, heights[0], arity, idx)
    rows = [MM.open_rows(groups, i) for i in idx]
    want, outs = WM.batch(oracle, rows, heights, idx, paths, arity, pad_mode=pad_mode)
    n_perms = MM.permutations(cols, depth, pad_mode)
    assert want.shape == (n_perms, n, 5, 4) and all(outs[-1, q, 1].tobytes() == root.tobytes() for q in range(n))
    depths = [MM.depth_of(h, arity) for h in heights]
    climb = [a - b for a, b in zip(depths, depths[1:] + [0])]
    files = {"rows": np.stack([MM.flat_rows(r) for r in rows]), "idx": np.array(idx, dtype=np.uint64), "paths": paths}
    for name, a in files.items():
        (tmp_path / (name + ".bin")).write_bytes(np.ascontiguousarray(a, dtype=np.uint64).tobytes())
    out = tmp_path / "inputs.bin"
    args = [exe, str(out), str(n), str(arity), str(pad_mode), "1", str(n_perms)]
    args += _limbs(CAP) + _limbs(TAG[arity]) + _limbs(MM.INJECT) + [str(tmp_path / (k + ".bin")) for k in ("rows", "idx", "paths")]
    args += ["1" if want_roots else "0", str(len(cols))] + [str(v) for pair in zip(cols, climb) for v in pair]
    _run(args)
    assert out.read_bytes() == want.tobytes()
    roots = tmp_path / "inputs.bin.roots"
    if want_roots:
        assert roots.read_bytes() == np.tile(root, n).tobytes()
    else:
        assert not roots.exists()


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_inputs_and_roots_equal_the_model(exe, tmp_path, oracle, case, n):
    """A lone lane, a ragged block, two blocks plus a ragged one, over the three fixture shapes (arities 2, 4 and 3; 9, 5 and
    6 permutations per opening: at most 2313 emulated permutations a case)."""
    _case(exe, tmp_path, oracle, case, n)


def test_without_roots_nothing_but_the_inputs_is_written(exe, tmp_path, oracle):
    _case(exe, tmp_path, oracle, 0, 1, want_roots=False)
