"""CPU tier: the boundary of the inverse permutation (hades252_perm_inverse_batch / _rounds, hades252_fifth_root_batch)
without a GPU -- the symbols are declared, bound and exported, host pointers only; every argument rule answers before the
device is touched and leaves the buffer alone; the Python wrappers refuse bad arguments before they call the library; the
C++ wrappers compile and link; the code objects of the two kernels have no scratch, no spilled VGPR and fit their launch
bounds and a CU's LDS; and the new sources leave the keys of the committed counter records alone."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import abi_common
import codeobj
from abi_common import INVALID, MIS, PTR

NAMES = ["hades252_perm_inverse_batch", "hades252_perm_inverse_rounds", "hades252_fifth_root_batch"]
SENTINEL = 0xABCDEF0123456789
LDS_PER_CU = 160 * 1024                  # gfx950
VGPRS_PER_SIMD = 512                     # per lane; allocated in blocks of 8


def _p(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


def test_symbols_are_declared_bound_and_exported_host_pointers_only(hades_lib):
    abi_common.assert_declared_bound_exported(NAMES)
    m = re.search(r"^#define HADES252_ROUNDS_TOTAL (\d+)$", abi_common.header(), flags=re.M)
    assert m is not None and int(m.group(1)) == hades_lib.hades252_rounds() == 67
    text = re.sub(r"/\*.*?\*/", "", abi_common.header(), flags=re.S)
    assert not re.search(r"hades252_(perm_inverse|fifth_root)\w*_dev", text)


def test_header_says_what_the_calls_are_and_are_not():
    block = abi_common.header_block("the inverse permutation and batched fifth roots", "#define HADES252_ROUNDS_TOTAL",
                                    ("perm_inverse(perm(x)) == x", "no device-pointer form", "no canonical-bytes form",
                                     "latency form", "311 Montgomery products", "is not measured", "8-byte aligned",
                                     "hades252_perm_trace_dev", "hades252_quintic_s_box_dev", "0 -> 0"))
    assert "CONVENTION UNPINNED" not in block


def test_argument_rules_answer_before_the_device_and_leave_the_buffer_alone(hades_lib):
    batch, rounds, root = (getattr(hades_lib, n) for n in NAMES)
    buf = np.full(2 * 20 + 1, SENTINEL, dtype=np.uint64)
    # n = 0: a no-op success, even with a NULL pointer, whatever else
    assert batch(None, 0) == 0 and root(None, 0) == 0 and rounds(None, 0, 67, 0) == 0 and rounds(None, 0, 99, -1) == 0
    assert batch(_p(buf), 0) == 0 and root(MIS + 1, 0) == 0
    # NULL with n > 0
    assert batch(None, 2) == INVALID and root(None, 2) == INVALID and rounds(None, 2, 67, 0) == INVALID
    # a pointer that is not 8-byte aligned (never dereferenced)
    for off in (1, 2, 4, 7):
        assert batch(_p(buf, off), 2) == INVALID and root(_p(buf, off), 2) == INVALID
        assert rounds(_p(buf, off), 2, 5, 3) == INVALID and rounds(PTR + off, 2, 5, 3) == INVALID
    # round ranges outside 0 <= round_lo <= round_hi <= 67
    for hi, lo in ((68, 0), (67, -1), (3, 4), (0, 1), (-1, -1), (68, 68), (1 << 30, 0), (67, 68)):
        assert rounds(_p(buf), 2, hi, lo) == INVALID, (hi, lo)
    # a batch whose byte count does not fit size_t
    assert batch(PTR, (1 << 64) // 160 + 1) == INVALID and root(PTR, (1 << 64) // 32 + 1) == INVALID
    # round_hi == round_lo: a no-op success without a device, on any 8-byte aligned pointer
    for r in (0, 4, 63, 67):
        assert rounds(_p(buf), 2, r, r) == 0 and rounds(_p(buf, 8), 2, r, r) == 0
    assert (buf == SENTINEL).all()


def test_python_wrappers_refuse_bad_arguments_before_the_library(monkeypatch):
    from hades252_amd import _lib, strategy as H

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    good = np.zeros((2, 5, 4), dtype=np.uint64)
    calls = (H.perm_inverse, lambda a: H.perm_inverse_rounds(a, 5, 3))
    for f in calls:
        for states in (np.zeros((2, 5, 4), dtype=np.int64), np.zeros((2, 5, 4), dtype=np.uint32), [[[0] * 4] * 5],
                       np.zeros((2, 4, 5, 4), dtype=np.uint64)[:, 0]):            # wrong dtype, not an array, not contiguous
            with pytest.raises(TypeError):
                f(states)
        for states in (np.zeros((2, 20), dtype=np.uint64), np.zeros((2, 4, 4), dtype=np.uint64),
                       np.zeros((5, 4), dtype=np.uint64), np.zeros((2, 5, 8), dtype=np.uint64)):
            with pytest.raises(ValueError):
                f(states)
    for scalars in (np.zeros((3, 4), dtype=np.int64), [[0] * 4], np.zeros((3, 2, 4), dtype=np.uint64)[:, 0]):
        with pytest.raises(TypeError):
            H.fifth_root(scalars)
    for scalars in (np.zeros((12,), dtype=np.uint64), np.zeros((3, 5, 4), dtype=np.uint64), np.zeros((3, 8), dtype=np.uint64)):
        with pytest.raises(ValueError):
            H.fifth_root(scalars)
    for hi, lo in ((68, 0), (67, -1), (3, 4), (5.0, 3), (5, None), (True, 0)):
        with pytest.raises(ValueError):
            H.perm_inverse_rounds(good, hi, lo)
    assert H.ROUNDS_TOTAL == 67


def test_python_wrappers_no_op_cases_return_new_arrays(hades_lib):
    from hades252_amd import strategy as H
    out = H.perm_inverse(np.zeros((0, 5, 4), dtype=np.uint64))
    assert out.shape == (0, 5, 4) and out.dtype == np.uint64
    assert H.fifth_root(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)
    x = np.arange(40, dtype=np.uint64).reshape(2, 5, 4)
    y = H.perm_inverse_rounds(x, 9, 9)
    assert y is not x and (y == x).all() and not np.shares_memory(x, y)


def test_cpp_wrappers_compile_and_link(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "perm_inverse", r'''
#include "hades252.hpp"
#include <cstdio>
#include <vector>
int main() {
    using dusk_hades::BlsScalar;
    std::vector<BlsScalar> states(2 * 5);
    try {
        dusk_hades::perm_inverse(states.data(), 0);                         // no-ops: no device needed
        dusk_hades::fifth_root(states.data(), 0);
        dusk_hades::perm_inverse_rounds(states.data(), 2, 7, 7);
        std::printf("no-ops ok\n");
        dusk_hades::perm_inverse_rounds(states.data(), 2, 68, 0);
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused\n");
    }
    static_assert(HADES252_ROUNDS_TOTAL == 67, "8 full rounds and 59 partial ones");
    return 0;
}
''')
    assert out == ["no-ops ok", "refused"]


def _launch_bounds(kernel):
    with open(os.path.join(abi_common.CSRC, "kernels_inverse.hpp")) as f:
        src = f.read()
    m = re.search(r"__launch_bounds__\(kBlock, (\w+)\) %s\(" % kernel, src)
    assert m is not None, kernel
    minw = m.group(1)
    if not minw.isdigit():
        minw = re.search(r"^#define %s (\d+)$" % minw, src, flags=re.M).group(1)
    return int(minw)


@pytest.mark.parametrize("kernel,lds_at_launch", [("k_perm_inverse", 4 * 64 * (5 * 32 + 16)), ("k_fifth_root", 0)])
def test_kernels_have_no_scratch_and_fit_their_bounds(hades_lib, kernel, lds_at_launch):
    """By the code object's metadata only."""
    co = codeobj.load()
    names = co.kernels(kernel)
    assert len(names) == 1, sorted(co.meta)
    r = co.meta[names[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    minw = _launch_bounds(kernel)
    budget = VGPRS_PER_SIMD // minw // 8 * 8               # __launch_bounds__(256, minw): minw waves per SIMD share 512 registers
    assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] + r["agpr_count"] <= budget, (r, budget)
    # LDS: what the kernel declares plus what host_inverse.hpp asks for at the launch (lds_for(5): 4 waves x 64 records x
    # 176 bytes; none for the scalar kernel) fits a CU -- minw blocks' worth would be the residency the bounds allow
    with open(os.path.join(abi_common.CSRC, "host_inverse.hpp")) as f:
        host = f.read()
    asked = re.search(r"hipLaunchKernelGGL\(%s, dim3\(blocks_for\(m\)\), dim3\(kBlock\), ([^,]+)," % kernel, host).group(1)
    assert asked == ("lds_for(5)" if lds_at_launch else "0")
    assert r["group_segment_fixed_size"] + lds_at_launch <= LDS_PER_CU
    print("%s: %d VGPRs, %d AGPRs, %d SGPRs, LDS %d + %d" % (kernel, r["vgpr_count"], r["agpr_count"], r["sgpr_count"],
                                                           r["group_segment_fixed_size"], lds_at_launch))


def test_build_lists_and_hashes_are_those_of_the_parent_commit():
    """Structurally: the new files are built (DEPS) and are in none of the lists that key a committed record, and the
    committed records carry today's hashes -- so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    new = {"kernels_inverse.hpp", "hades_inverse_constants.inc", "host_inverse.hpp"}
    assert new == set(build.INVERSE_DEPS) and new <= set(build.DEPS)
    assert not new & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                         build.HOST_DEPS + build.GRIND_DEPS)
    assert all(os.path.exists(os.path.join(abi_common.CSRC, f)) for f in new)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    with open(os.path.join(abi_common.CSRC, "hades252.hip")) as f:
        unit = f.read()
    assert unit.index('"kernels_grind.hpp"') < unit.index('"hades_inverse_constants.inc"') < unit.index('"kernels_inverse.hpp"')
    assert unit.index('"host_grind.hpp"') < unit.index('"host_inverse.hpp"') < unit.index('"host_cipher.hpp"')
