"""CPU tier: the boundary of the matrix commitments (hades252_matrix_row_digests / _commit / _open / _verify) without a GPU --
the symbols are declared, bound and exported, host pointers only; every argument rule answers before the device is touched;
hades252_matrix_open, which is plain host code, really runs here against the golden matrices and the oracle's trees; the
Python wrappers refuse bad arguments before they call the library; the C++ wrappers compile and link; the code object of
k_sponge_planes has no scratch, no spilled VGPR, no LDS and fits its launch bounds; and the new sources leave the keys of the
committed counter records alone."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import abi_common
import codeobj
import matrix_model as M
from abi_common import INVALID, MIS, PTR, limbs4
from gpu_common import TAG

NAMES = ["hades252_matrix_row_digests", "hades252_matrix_commit", "hades252_matrix_open", "hades252_matrix_verify"]
SENTINEL = M.SENTINEL
VGPRS_PER_SIMD = 512                     # per lane; allocated in blocks of 8
ODD = PTR + 4                            # not 8-byte aligned (abi_common.MIS is 8-byte aligned: fine for host pointers)
MAX_COLS = 4096


def _p(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(abi_common.ROOT, "tests", "golden", "matrix_kat.json")) as f:
        return json.load(f)["cases"]


def test_symbols_are_declared_bound_and_exported_host_pointers_only(hades_lib):
    abi_common.assert_declared_bound_exported(NAMES)
    m = re.search(r"^#define HADES252_MATRIX_MAX_COLS (\d+)", abi_common.header(), flags=re.M)
    from hades252_amd import _lib
    assert m is not None and int(m.group(1)) == _lib.MATRIX_MAX_COLS == MAX_COLS
    text = re.sub(r"/\*.*?\*/", "", abi_common.header(), flags=re.S)
    assert not re.search(r"hades252_matrix\w*_dev\b", text)
    assert sorted(re.findall(r"\bhades252_matrix_\w+", text)) == sorted(NAMES)


def test_header_says_what_the_calls_are_and_are_not():
    block = abi_common.header_block("column-major matrix commitments", "#define HADES252_MATRIX_MAX_COLS",
                                    ("CONVENTION UNPINNED", "(c * plane_stride + r) * 4", "hades252_sponge_hash",
                                     "hades252_merkle_build_pad_dev", "hades252_merkle_open_pad_dev", "no device-pointer form",
                                     "no canonical-bytes form", "no witness form", "one row per lane", "latency form",
                                     "8-byte aligned", "plane_stride < n_rows", "touches no device", "all-zero row and path",
                                     "Page-locked", "do not overlap", "HADES252_ERR_NO_DEVICE", "overflows size_t",
                                     "even with NULL pointers"))
    assert "(f12)" in block


def test_argument_rules_answer_before_the_device(hades_lib):
    digests_of, commit, open_, verify = (getattr(hades_lib, n) for n in NAMES)
    cap, tag = limbs4(), limbs4(5, 6, 7, 8)
    # no-op successes, even with NULL (and misaligned, and otherwise invalid) arguments
    assert digests_of(None, 0, 0, 0, None, 7, None) == 0 and digests_of(ODD, 0, 1, 0, cap, 1, ODD) == 0
    assert open_(None, 0, 0, 0, None, None, 9, None, None, 0, None, None) == 0
    assert verify(None, 0, None, None, 0, 0, 9, None, 7, None, 9, None) == 0

    def rd(planes=PTR, n_rows=4, n_cols=3, stride=4, cap_=cap, pad_mode=1, out=PTR):
        return digests_of(planes, n_rows, n_cols, stride, cap_, pad_mode, out)

    def cm(planes=PTR, n_rows=4, n_cols=3, stride=4, cap_=cap, pad_mode=1, arity=2, tag_=tag, out_idx=1, pad=None, dig=PTR,
           tree=PTR, root=PTR):
        return commit(planes, n_rows, n_cols, stride, cap_, pad_mode, arity, tag_, out_idx, pad, dig, tree, root)

    def op(planes=PTR, n_rows=4, n_cols=3, stride=4, dig=PTR, tree=PTR, arity=2, pad=None, idx=PTR, nq=2, rows=PTR, paths=PTR):
        return open_(planes, n_rows, n_cols, stride, dig, tree, arity, pad, idx, nq, rows, paths)

    def vf(rows=PTR, n_cols=3, idx=PTR, paths=PTR, nq=2, depth=2, arity=2, cap_=cap, pad_mode=1, tag_=tag, out_idx=1, roots=PTR):
        return verify(rows, n_cols, idx, paths, nq, depth, arity, cap_, pad_mode, tag_, out_idx, roots)

    # a NULL pointer that is needed
    assert rd(planes=None) == INVALID and rd(cap_=None) == INVALID and rd(out=None) == INVALID
    assert cm(planes=None) == INVALID and cm(cap_=None) == INVALID and cm(tag_=None) == INVALID and cm(root=None) == INVALID
    for k in ("planes", "dig", "tree", "idx", "rows", "paths"):
        assert op(**{k: None}) == INVALID, k
    for k in ("rows", "idx", "paths", "cap_", "tag_", "roots"):
        assert vf(**{k: None}) == INVALID, k
    # a pointer that is not 8-byte aligned (never dereferenced)
    for off in (1, 2, 4, 7):
        bad = PTR + off
        assert rd(planes=bad) == INVALID and rd(out=bad) == INVALID
        for k in ("planes", "pad", "dig", "tree", "root"):
            assert cm(**{k: bad}) == INVALID, k
        for k in ("planes", "dig", "tree", "pad", "idx", "rows", "paths"):
            assert op(**{k: bad}) == INVALID, k
        for k in ("rows", "idx", "paths", "roots"):
            assert vf(**{k: bad}) == INVALID, k
    # n_cols outside 1 .. HADES252_MATRIX_MAX_COLS
    for n_cols in (0, MAX_COLS + 1, 1 << 40):
        assert rd(n_cols=n_cols) == INVALID and cm(n_cols=n_cols) == INVALID and op(n_cols=n_cols) == INVALID
        assert vf(n_cols=n_cols) == INVALID
    # plane_stride < n_rows
    assert rd(stride=3) == INVALID and cm(stride=3) == INVALID and op(stride=0) == INVALID
    # pad_mode, arity, out_idx
    for pad_mode in (-1, 2, 7):
        assert rd(pad_mode=pad_mode) == INVALID and cm(pad_mode=pad_mode) == INVALID and vf(pad_mode=pad_mode) == INVALID
    for arity in (-2, 0, 1, 5):
        assert cm(arity=arity) == INVALID and op(arity=arity) == INVALID and vf(arity=arity) == INVALID
    for out_idx in (-1, 5, 99):
        assert cm(out_idx=out_idx) == INVALID and vf(out_idx=out_idx) == INVALID
    # n_rows < 2 where a tree is needed; a depth that is not positive (or beyond the 64 levels a 2^64 tree has)
    for n_rows in (0, 1):
        assert cm(n_rows=n_rows, stride=4) == INVALID and op(n_rows=n_rows) == INVALID
    for depth in (0, -1, -(1 << 31), 65):
        assert vf(depth=depth) == INVALID
    # byte counts that do not fit size_t, and counts beyond 2^30
    assert rd(n_rows=4, n_cols=MAX_COLS, stride=(1 << 64) // 32 // MAX_COLS + 1) == INVALID
    assert cm(n_rows=4, n_cols=MAX_COLS, stride=(1 << 64) // 32 // MAX_COLS + 1) == INVALID
    assert rd(n_rows=(1 << 30) + 1, stride=(1 << 30) + 1) == INVALID and cm(n_rows=(1 << 30) + 1, stride=(1 << 30) + 1) == INVALID
    assert op(nq=(1 << 64) // 32 // 3 + 1) == INVALID and op(n_cols=1, nq=(1 << 64) // 32 // 2 + 1) == INVALID
    assert vf(nq=(1 << 30) + 1) == INVALID and vf(nq=(1 << 64) - 1) == INVALID
    assert MIS % 8 == 0


def _golden_arrays(c):
    m = M.unhex(c["matrix_row_major"]).reshape(c["n_rows"], c["n_cols"], 4)
    return m, M.unhex(c["digests"]), M.unhex(c["tree"])


def _open(hades_lib, planes, n_rows, digests, tree, arity, pad, idx):
    """hades252_matrix_open into buffers with a sentinel row before and after each output."""
    n_cols, stride = planes.shape[0], planes.shape[1]
    depth = M.depth_of(n_rows, arity)
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    q = idx.size
    rows = np.full((q + 2, n_cols, 4), SENTINEL, dtype=np.uint64)
    paths = np.full((q + 2, depth, arity - 1, 4), SENTINEL, dtype=np.uint64)
    rc = hades_lib.hades252_matrix_open(_p(planes), n_rows, n_cols, stride, _p(digests), _p(tree), arity,
                                        None if pad is None else _p(pad), _p(idx), q, _p(rows, rows[0].nbytes),
                                        _p(paths, paths[0].nbytes))
    assert rc == 0
    for a in (rows, paths):
        assert (a[0] == SENTINEL).all() and (a[-1] == SENTINEL).all(), "written outside the output"
    return rows[1:-1], paths[1:-1]


def test_open_runs_here_and_gives_the_golden_openings(hades_lib, golden):
    for c in golden:
        m, digests, tree = _golden_arrays(c)
        n_rows, arity = c["n_rows"], c["arity"]
        rows, paths = _open(hades_lib, M.planes_of(m), n_rows, digests, tree, arity, None, [c["opening"]["index"]])
        assert rows.tobytes() == M.unhex(c["opening"]["row"]).tobytes()
        assert paths.tobytes() == M.unhex(c["opening"]["path"]).tobytes()
        # every row, duplicates, unsorted, and indices past the end -- with a gap between the planes
        idx = list(range(n_rows - 1, -1, -1)) + [0, 0, n_rows, n_rows - 1, (1 << 64) - 1, n_rows + 1]
        rows, paths = _open(hades_lib, M.planes_of(m, n_rows + 3), n_rows, digests, tree, arity, None, idx)
        want_rows, want_paths = M.open_rows(m, digests, tree, arity, [min(i, n_rows) for i in idx])
        assert rows.tobytes() == want_rows.tobytes() and paths.tobytes() == want_paths.tobytes()
        for t, i in enumerate(idx):
            assert rows[t].any() == (i < n_rows)                           # an index >= n_rows: zeros
            assert i < n_rows or not paths[t].any()
        assert not (rows == SENTINEL).any()                                # the gap between two planes is never read


@pytest.mark.parametrize("n_rows,n_cols,arity", [(7, 2, 2), (10, 3, 3), (22, 1, 4), (65, 2, 4)])
def test_open_on_the_oracles_padded_trees(hades_lib, oracle, n_rows, n_cols, arity):
    """Ragged levels with the empty-subtree table: a sibling past the end of level l is pad[l]; every opening verifies."""
    m = oracle.gen_b(14000 + n_rows, n_rows * n_cols).reshape(n_rows, n_cols, 4)
    depth = M.depth_of(n_rows, arity)
    pad = oracle.merkle_empty_digests(arity, depth, 9, TAG[arity])
    digests, tree, root = M.commit(oracle, m, arity, pad=pad)
    idx = list(range(n_rows))
    rows, paths = _open(hades_lib, M.planes_of(m, n_rows + 1), n_rows, digests, tree, arity, pad, idx)
    want_rows, want_paths = M.open_rows(m, digests, tree, arity, idx, pad)
    assert rows.tobytes() == want_rows.tobytes() == m.tobytes() and paths.tobytes() == want_paths.tobytes()
    for t in (0, n_rows // 2, n_rows - 1):
        assert M.verify(oracle, rows[t], t, paths[t], arity).tobytes() == root.tobytes()


def test_python_wrappers_refuse_bad_arguments_before_the_library(monkeypatch):
    from hades252_amd import _lib, strategy as H

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    good = np.zeros((3, 8, 4), dtype=np.uint64)
    calls = (lambda a: H.matrix_row_digests_host(a, 1), lambda a: H.matrix_commit_host(a, 1, 2, 3),
             lambda a: H.matrix_open_host(a, np.zeros((8, 4), dtype=np.uint64), np.zeros((7, 4), dtype=np.uint64), 2, [0]))
    for f in calls:
        for planes in (np.zeros((3, 8, 4), dtype=np.int64), [[[0] * 4] * 8] * 3, np.zeros((3, 8, 2, 4), dtype=np.uint64)[:, :, 0]):
            with pytest.raises(TypeError):
                f(planes)
        for planes in (np.zeros((3, 32), dtype=np.uint64), np.zeros((3, 8, 5), dtype=np.uint64), np.zeros((0, 8, 4), dtype=np.uint64),
                       np.zeros((_lib.MATRIX_MAX_COLS + 1, 2, 4), dtype=np.uint64)):
            with pytest.raises(ValueError):
                f(planes)
    with pytest.raises(ValueError):
        H.matrix_row_digests_host(good, 1, n_rows=9)                      # more rows than the planes hold
    with pytest.raises(ValueError):
        H.matrix_row_digests_host(good, 1, pad_mode=2)
    for kw in ({"arity": 5}, {"arity": 1}, {"n_rows": 1}, {"pad_mode": 3}, {"out_idx": 5}, {"pad": np.zeros((2, 4), dtype=np.uint64)}):
        args = dict(arity=2)
        args.update(kw)
        with pytest.raises(ValueError):
            H.matrix_commit_host(good, 1, args.pop("arity"), 3, **args)
    with pytest.raises(ValueError):                                       # a tree of the wrong size
        H.matrix_open_host(good, np.zeros((8, 4), dtype=np.uint64), np.zeros((6, 4), dtype=np.uint64), 2, [0])
    rows, paths = np.zeros((2, 3, 4), dtype=np.uint64), np.zeros((2, 3, 1, 4), dtype=np.uint64)
    for r, i, p, a in ((rows, [0, 1], paths, 3), (rows, [0], paths, 2), (rows[:, 0], [0, 1], paths, 2),
                       (rows, [0, 1], np.zeros((2, 0, 1, 4), dtype=np.uint64), 2), (rows, [0, 1], paths, 1)):
        with pytest.raises(ValueError):
            H.matrix_verify_host(np.ascontiguousarray(r), i, p, a, 1, 3)


def test_python_open_and_no_op_cases(hades_lib, golden):
    from hades252_amd import strategy as H
    out = H.matrix_row_digests_host(np.zeros((3, 0, 4), dtype=np.uint64), 1)
    assert out.shape == (0, 4) and out.dtype == np.uint64
    assert H.matrix_row_digests_host(np.zeros((3, 8, 4), dtype=np.uint64), 1, n_rows=0).shape == (0, 4)
    c = golden[2]
    m, digests, tree = _golden_arrays(c)
    rows, paths = H.matrix_open_host(M.planes_of(m, 12), digests, tree, c["arity"], [c["opening"]["index"], 99], n_rows=c["n_rows"])
    assert rows.shape == (2, c["n_cols"], 4) and paths.shape == (2, M.depth_of(c["n_rows"], c["arity"]), c["arity"] - 1, 4)
    assert rows[0].tobytes() == M.unhex(c["opening"]["row"]).tobytes()
    assert paths[0].tobytes() == M.unhex(c["opening"]["path"]).tobytes() and not rows[1].any() and not paths[1].any()
    r0, p0 = H.matrix_open_host(M.planes_of(m), digests, tree, c["arity"], [])
    assert r0.shape[0] == 0 and p0.shape[0] == 0
    assert H.matrix_verify_host(r0, [], p0, c["arity"], 1, 3).shape == (0, 4)


def test_cpp_wrappers_compile_and_link(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "matrix", r'''
#include "hades252.hpp"
#include <cstdint>
#include <cstdio>
#include <vector>
int main() {
    using dusk_hades::BlsScalar;
    std::vector<BlsScalar> planes(2 * 4), digests(4), tree(3), rows(2), paths(2);
    BlsScalar cap{}, tag{};
    std::uint64_t idx[1] = {7};
    try {
        dusk_hades::matrix_row_digests(planes.data(), 0, 2, 4, cap, true, digests.data());            // no-ops: no device
        dusk_hades::matrix_verify(rows.data(), 2, idx, paths.data(), 0, 2, 2, cap, true, tag, 1, digests.data());
        dusk_hades::matrix_open(planes.data(), 4, 2, 4, digests.data(), tree.data(), 2, nullptr, idx, 1, rows.data(), paths.data());
        bool zero = true;                                                                             // index 7 >= 4 rows
        for (const BlsScalar &s : rows)
            for (int k = 0; k < 4; k++) zero = zero && s.limbs[k] == 0;
        std::printf(zero ? "open ok\n" : "open wrote something\n");
        dusk_hades::matrix_commit(planes.data(), 1, 2, 4, cap, true, 2, tag);                         // one row: no tree
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused %d\n", e.code);
    }
    static_assert(HADES252_MATRIX_MAX_COLS == 4096, "256 rows of 4096 columns are 32 MiB");
    return 0;
}
''')
    assert out == ["open ok", "refused -1"]


def _kernel_source():
    with open(os.path.join(abi_common.CSRC, "kernels_matrix.hpp")) as f:
        return f.read()


def test_kernel_has_no_scratch_no_lds_and_fits_its_bounds(hades_lib):
    """By the code object's metadata only."""
    co = codeobj.load()
    names = co.kernels("k_sponge_planes")
    assert len(names) == 1, sorted(co.meta)
    r = co.meta[names[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    src = _kernel_source()
    minw = re.search(r"__launch_bounds__\(kBlock, (\w+)\) k_sponge_planes\(", src).group(1)
    if not minw.isdigit():
        minw = re.search(r"^#define %s (\d+)$" % minw, src, flags=re.M).group(1)
    budget = VGPRS_PER_SIMD // int(minw) // 8 * 8         # __launch_bounds__(256, minw): minw waves per SIMD share 512 registers
    assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] + r["agpr_count"] <= budget, (r, budget)
    # LDS: the kernel declares none and host_matrix.hpp asks for none at the launch
    with open(os.path.join(abi_common.CSRC, "host_matrix.hpp")) as f:
        host = f.read()
    asked = re.findall(r"hipLaunchKernelGGL\(k_sponge_planes, dim3\(blocks_for\(m\)\), dim3\(kBlock\), ([^,]+),", host)
    assert asked == ["0"] and r["group_segment_fixed_size"] == 0
    assert "__shared__" not in src and "__syncthreads" not in src
    print("k_sponge_planes: %d VGPRs, %d AGPRs, %d SGPRs, LDS %d" % (r["vgpr_count"], r["agpr_count"], r["sgpr_count"],
                                                                    r["group_segment_fixed_size"]))


def test_build_lists_and_hashes_are_those_of_the_parent_commit():
    """Structurally: the new files are built (DEPS) and are in none of the lists that key a committed record, and the
    committed records carry today's hashes -- so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    new = {"kernels_matrix.hpp", "host_matrix.hpp"}
    assert new == set(build.MATRIX_DEPS) and new <= set(build.DEPS)
    assert not new & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                         build.HOST_DEPS + build.GRIND_DEPS + build.INVERSE_DEPS)
    assert all(os.path.exists(os.path.join(abi_common.CSRC, f)) for f in new)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    with open(os.path.join(abi_common.CSRC, "hades252.hip")) as f:
        unit = f.read()
    assert unit.index('"kernels_inverse.hpp"') < unit.index('"kernels_matrix.hpp"') < unit.index('"kernels_witness.hpp"')
    assert unit.index('"host_inverse.hpp"') < unit.index('"host_matrix.hpp"') < unit.index('"host_cipher.hpp"')
