"""CPU tier: the shipped kernels of hades252_amd/csrc/kernels_mmcs.hpp (k_mmcs_inject, k_mmcs_verify) run on the CPU under
ASan + UBSan, bit-exact against the model (tests/mmcs_model.py: the oracle's sponge and Merkle level) -- before any GPU sees
them.

tests/hostsim_mmcs/mmcs_main.cpp is a stand-alone program (its own main) over the block emulator of
tests/hostsim/hip/hip_runtime.h and the tree's headers as tests/hostsim_lib.py copies them (rewritten(): the allow-list of
semantically empty edits; check_copy() refuses anything else).  It is built with hostsim_lib's compiler and its "asan" flags
and run as an ordinary child process: nothing is preloaded, nothing is loaded into this interpreter.  Every buffer is a heap
block of exactly its size and a poisoned gap lies between the rows and the paths: a row word past the last row, a sibling
outside the paths, a store past the last node or root is an ASan report.  An emulated block takes seconds, so the cases are
few."""
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
import oracle_lib  # noqa: E402
from gpu_common import CAP, TAG  # noqa: E402

HERE = os.path.join(ROOT, "tests", "hostsim_mmcs")
MAIN = os.path.join(HERE, "mmcs_main.cpp")


@pytest.fixture(scope="module")
def exe():
    """The driver under ASan + UBSan; rebuilt when the driver, the stand-in, a copied header or the flags change."""
    return HS.build_driver(MAIN, "mmcs_main")


def _limbs(v):
    return [str(x) for x in oracle_lib.limbs_of(v)]


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env=dict(os.environ, **HS.SAN_ENV))
    assert r.returncode == 0, "mmcs_main exited %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])


def test_driver_defines_no_device_routine_and_launches_with_the_call_sites_geometry():
    with open(MAIN) as f:
        main = HS._strip_comments(f.read())
    assert "__global__" not in main and "__device__" not in main and not re.search(r"\basm\b", main)
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", main) == ["k_mmcs_inject", "k_mmcs_verify"]
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "host_mmcs.hpp")) as f:
        host = re.sub(r"\s*\\\n\s*", " ", f.read())
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", host) == ["k_planes_finish", "k_mmcs_inject", "k_mmcs_verify"]
    # the call sites: one block of kBlock lanes per kBlock items, no LDS
    assert ("hipLaunchKernelGGL(k_mmcs_inject, dim3(blocks_for(n)), dim3(kBlock), 0, pp.s_k, parents, "
            "h->groups[order[next]]->d_dig, n, inject_tag, out_idx);") in host
    assert ("hipLaunchKernelGGL(k_mmcs_verify<A>, dim3(blocks_for(m)), dim3(kBlock), 0, s, d_rows, d_idx, d_paths, m, table, n_groups, "
            "row_cols, depth, n_perms, pad_mode, cap, tag, inject_tag, out_idx, d_roots)") in host
    assert ("hipLaunchKernelGGL(k_planes_finish, dim3(blocks_for(S)), dim3(kBlock), 0, pp.s_k, ms->d_state, S, S, dig, "
            "(int)(ms->n_cols % 4), pad_mode);") in host
    main = re.sub(r"\s+", " ", main.replace("\\\n", " "))
    assert ("hipLaunchKernelGGL(k_mmcs_inject, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t) nullptr, "
            "nodes, leaf, n, inject_tag, out_idx);") in main
    assert ("hipLaunchKernelGGL(k_mmcs_verify<A>, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_rows, d_idx, "
            "d_paths, m, table, n_groups, row_cols, depth, n_perms, pad_mode, cap, tag, inject_tag, out_idx, d_roots)") in main
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "kernels_mmcs.hpp")) as f:
        kernels = HS._strip_comments(f.read())
    assert len(re.findall(r"\bfast_perm<5>\(", kernels)) == 1 and len(re.findall(r"\bfast_perm<1>\(", kernels)) == 1
    assert "__shared__" not in kernels and "__syncthreads" not in kernels and not re.search(r"\basm\b", kernels)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_inject_equals_the_model(exe, tmp_path, oracle, n):
    nodes, leaves = oracle.gen_b(21000 + n, n).reshape(n, 4).copy(), oracle.gen_b(22000 + n, n).reshape(n, 4).copy()
    if n > 2:
        nodes[0], leaves[n - 1] = 0, np.array(oracle_lib.limbs_of(oracle_lib.P - 1), dtype=np.uint64)
    (tmp_path / "nodes.bin").write_bytes(nodes.tobytes())
    (tmp_path / "leaves.bin").write_bytes(leaves.tobytes())
    for out_idx in ((1,) if n > 1 else (0, 1, 4)):
        out = tmp_path / ("out%d.bin" % out_idx)
        _run([exe, "inject", str(out), str(n), str(out_idx)] + _limbs(MM.INJECT) + [str(tmp_path / "nodes.bin"), str(tmp_path / "leaves.bin")])
        got = np.frombuffer(out.read_bytes(), dtype=np.uint64).reshape(n, 4)
        assert got.tobytes() == MM.inject(oracle, nodes, leaves, MM.INJECT, out_idx).tobytes(), out_idx


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_verify_equals_the_model(exe, tmp_path, oracle, case, n):
    """n queries over a fixture shape: the indices walk over every leaf (and so every position of every level), query 0 opens
    an all-zero tallest row and the last query rows of p - 1; every third query is tampered with (a row word, a sibling or the
    index in turn), so that the roots differ from query to query."""
    arity, heights, cols, pad_mode, _, first = MM.GOLDEN_CASES[case]
    groups = [g.copy() for g in MM.golden_groups(oracle, heights, cols, first)]
    groups[0][0] = 0
    groups[-1][-1] = np.array(oracle_lib.limbs_of(oracle_lib.P - 1), dtype=np.uint64)
    tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    depth = MM.depth_of(heights[0], arity)
    idx = [(3 * t) % heights[0] for t in range(n - 1)] + [heights[0] - 1]
    paths = MM.open_paths(tree, heights[0], arity, idx)
    rows, want, honest = [], [], 0
    for t, i in enumerate(idx):
        r, p = MM.open_rows(groups, i), paths[t]
        if t % 3 == 1:
            bad = MM.tampers(r, i, p, heights[0])
            _, r, i, p = bad[(t // 3) % len(bad)]
            idx[t], paths[t] = i, p
        w = MM.verify(oracle, r, heights, i, p, arity, pad_mode=pad_mode)
        honest += w.tobytes() == root.tobytes()
        rows.append(MM.flat_rows(r))
        want.append(w)
    assert honest == n - len(range(1, n, 3))
    depths = [MM.depth_of(h, arity) for h in heights]
    climb = [a - b for a, b in zip(depths, depths[1:] + [0])]
    files = {"rows": np.stack(rows), "idx": np.array(idx, dtype=np.uint64), "paths": paths}
    for name, a in files.items():
        (tmp_path / (name + ".bin")).write_bytes(np.ascontiguousarray(a, dtype=np.uint64).tobytes())
    out = tmp_path / "roots.bin"
    args = [exe, "verify", str(out), str(n), str(arity), str(pad_mode), "1", str(MM.permutations(cols, depth, pad_mode))]
    args += _limbs(CAP) + _limbs(TAG[arity]) + _limbs(MM.INJECT) + [str(tmp_path / (k + ".bin")) for k in ("rows", "idx", "paths")]
    args += [str(len(cols))] + [str(v) for pair in zip(cols, climb) for v in pair]
    _run(args)
    got = np.frombuffer(out.read_bytes(), dtype=np.uint64).reshape(n, 4)
    assert got.tobytes() == np.stack(want).tobytes()
