"""CPU tier: the boundary of the proof-of-work grinding (hades252_grind) without a GPU -- the symbol is declared, bound and
exported; every argument rule answers before the device is touched and leaves the outputs alone; the two no-op cases behave
as the header says; the header block says CONVENTION UNPINNED and names the model; the Python wrapper refuses bad arguments
before it calls the library; the C++ wrapper compiles and links; the code object of k_grind in the built library has no
scratch, no spilled VGPR, no LDS and fits its launch bounds; and the new sources leave the keys of the committed counter
records (build.device_source_hash, build.perm_fast_hash) alone."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import abi_common
import codeobj
import grind_model as M
from abi_common import INVALID, PTR, limbs4

SENTINEL = 0xABCDEF0123456789


def _outputs(n):
    return np.full(n, SENTINEL, dtype=np.uint64), np.full(n, 7, dtype=np.uint8)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbol_is_declared_bound_and_exported(hades_lib):
    from hades252_amd import _lib
    abi_common.assert_declared_bound_exported(["hades252_grind"])
    m = re.search(r"^#define HADES252_GRIND_MAX_JOBS (\d+)$", abi_common.header(), flags=re.M)
    assert m is not None and int(m.group(1)) == _lib.GRIND_MAX_JOBS == 65535      # the y dimension of a grid
    # host pointers only: no device-pointer form is declared
    assert not re.search(r"hades252_grind\w*_dev", abi_common.header())


def test_header_says_convention_unpinned():
    abi_common.header_block("batched proof-of-work grinding", "#define HADES252_GRIND_MAX_JOBS",
                            ("CONVENTION UNPINNED", "tests/grind_model.py", "SMALLEST", "strictly",
                             "hades252_sponge_absorb_dev"))


def test_argument_rules_answer_before_the_device_and_leave_the_outputs_alone(hades_lib):
    fn = hades_lib.hades252_grind
    seeds = M.seeds_of([[1, 2, 3, 4, 5]] * 3)
    nonces, found = _outputs(3)

    def g(seeds_p=_p(seeds), n=3, word=4, out_idx=1, target=limbs4(), first=0, max_n=100, nonces_p=_p(nonces),
          found_p=_p(found)):
        return fn(seeds_p, n, word, out_idx, target, first, max_n, nonces_p, found_p)

    top = (1 << 64) - 1
    for kw in ({"seeds_p": None}, {"target": None}, {"nonces_p": None}, {"found_p": None}, {"word": -1}, {"word": 5},
               {"out_idx": -1}, {"out_idx": 5}, {"n": 65536, "seeds_p": PTR, "nonces_p": PTR, "found_p": PTR},
               {"first": 2, "max_n": top}, {"first": top, "max_n": 2}, {"first": 1 << 63, "max_n": (1 << 63) + 1},
               {"first": top - 299, "max_n": 301}):
        assert g(**kw) == INVALID, kw
        assert (nonces == SENTINEL).all() and (found == 7).all(), kw
    # n_jobs = 0: a no-op success, whatever else
    assert fn(None, 0, 9, 9, None, top, top, None, None) == 0
    assert (nonces == SENTINEL).all() and (found == 7).all()
    # max_nonces = 0: found = 0 everywhere, nonces untouched, no device needed -- at any first nonce
    for first in (0, 5, top):
        nonces, found = _outputs(3)
        assert fn(_p(seeds), 3, 4, 1, limbs4(), first, 0, _p(nonces), _p(found)) == 0
        assert (found == 0).all() and (nonces == SENTINEL).all()


def test_python_wrapper_refuses_bad_arguments_before_the_library(monkeypatch):
    from hades252_amd import _lib, strategy as H

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    good = np.zeros((2, 5, 4), dtype=np.uint64)
    for seeds in (np.zeros((2, 5, 4), dtype=np.int64), np.zeros((2, 5, 4), dtype=np.uint32), [[0] * 4] * 5,
                  np.zeros((2, 4, 5, 4), dtype=np.uint64)[:, 0]):                # wrong dtype, not an array, not contiguous
        with pytest.raises(TypeError):
            H.grind(seeds, 4, 1, 1)
    for seeds in (np.zeros((2, 20), dtype=np.uint64), np.zeros((2, 4, 4), dtype=np.uint64), np.zeros((5, 4), dtype=np.uint64),
                  np.zeros((2, 5, 8), dtype=np.uint64)):
        with pytest.raises(ValueError):
            H.grind(seeds, 4, 1, 1)
    for kw in ({"word": 5}, {"word": -1}, {"out_idx": 5}, {"out_idx": -1}, {"word": 1.0}, {"target": -1}, {"target": 1 << 256},
               {"target": 0.5}, {"first_nonce": -1}, {"max_nonces": -1}, {"first_nonce": 2, "max_nonces": (1 << 64) - 1},
               {"first_nonce": 0, "max_nonces": 1 << 64}):
        args = dict(word=4, out_idx=1, target=1, first_nonce=0, max_nonces=10)
        args.update(kw)
        with pytest.raises(ValueError):
            H.grind(good, **args)
    with pytest.raises(ValueError):
        H.grind(np.zeros((_lib.GRIND_MAX_JOBS + 1, 5, 4), dtype=np.uint64), 4, 1, 1)
    assert H.grind_target(0) == M.P and H.grind_target(20) == M.P >> 20 == M.target_bits(20)
    with pytest.raises(ValueError):
        H.grind_target(-1)


def test_python_wrapper_no_op_cases(hades_lib):
    from hades252_amd import strategy as H
    nonces, found = H.grind(np.zeros((0, 5, 4), dtype=np.uint64), 4, 1, 1)
    assert nonces.shape == (0,) and nonces.dtype == np.uint64 and found.shape == (0,) and found.dtype == bool
    nonces, found = H.grind(M.seeds_of([[1, 2, 3, 4, 5]] * 2), 4, 1, M.P, first_nonce=3, max_nonces=0)
    assert not found.any() and found.shape == (2,) and nonces.shape == (2,)


def test_cpp_wrapper_compiles_and_links(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "grind", r'''
#include "hades252.hpp"
#include <cstdio>
#include <vector>
int main() {
    using dusk_hades::BlsScalar;
    std::vector<BlsScalar> seeds(2 * 5);
    const std::uint64_t target[4] = {1, 0, 0, 0};
    std::uint64_t nonces[2] = {77, 77};
    std::uint8_t found[2] = {9, 9};
    try {
        dusk_hades::grind(seeds.data(), 2, 4, 1, target, 5, 0, nonces, found);     // an empty range: no device needed
        std::printf("%d %d %llu\n", found[0], found[1], (unsigned long long)nonces[0]);
        dusk_hades::grind(seeds.data(), 2, 5, 1, target, 0, 10, nonces, found);
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused\n");
    }
    static_assert(HADES252_GRIND_MAX_JOBS == 65535, "the y dimension of a grid");
    return 0;
}
''')
    assert out == ["0 0 77", "refused"]


def test_grind_kernel_has_no_scratch_no_lds_and_fits_its_bounds(hades_lib):
    co = codeobj.load()
    names = co.kernels("k_grind")
    assert len(names) == 1, sorted(co.meta)
    r, body = co.meta[names[0]], co.body(names[0])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and "scratch_" not in body, r
    # __launch_bounds__(256, 4): 4 waves per SIMD -> at most 128 registers (VGPRs + AGPRs: one file)
    assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] + r["agpr_count"] <= 128, r
    # no LDS at all: none declared, none asked for at the launch (host_grind.hpp passes 0), no LDS instruction
    assert r["group_segment_fixed_size"] == 0 and not re.search(r"\bds_\w+", body)
    with open(os.path.join(abi_common.CSRC, "kernels_grind.hpp")) as f:
        assert "__shared__" not in f.read()
    with open(os.path.join(abi_common.CSRC, "host_grind.hpp")) as f:
        assert re.search(r"hipLaunchKernelGGL\(k_grind, grid, dim3\(kBlock\), 0, s,", f.read())
    # one call site of the round loop and ONE word out of it: fewer multiply-adds than k_perm_fast, which leaves with five
    (fast,) = co.kernels("k_perm_fast")
    assert codeobj.mads(body) <= codeobj.mads(co.body(fast))
    # a hit leaves through a vector atomic on the job's slot, the early exit reads it with a vector load
    assert "global_atomic_umin_x2" in body


def test_build_hashes_are_those_of_the_parent_commit():
    """Structurally: the new files are built (DEPS) and are in none of the lists that key a committed record, and the
    committed records carry today's hashes -- so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    new = {"kernels_grind.hpp", "host_grind.hpp"}
    assert new == set(build.GRIND_DEPS) and new <= set(build.DEPS)
    assert not new & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                         build.HOST_DEPS)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    with open(os.path.join(abi_common.CSRC, "hades252.hip")) as f:
        unit = f.read()
    assert unit.index('"kernels_safe.hpp"') < unit.index('"kernels_grind.hpp"')
    assert unit.index('"host_safe.hpp"') < unit.index('"host_grind.hpp"') < unit.index('"host_cipher.hpp"')
