"""CPU tier: the boundary of the streaming matrix commitments (hades252_matstream_open / _absorb / _cols / _digests / _commit /
_close) without a GPU -- the symbols are declared, bound and exported, host pointers only; every rule that is decided before
the device is touched answers here (with a device in reach the rules that need an open stream are checked too: the GPU tier
calls the same function); header, ctypes table, C++ wrapper and generated Rust binding agree on the six prototypes; the
Python wrapper refuses bad arguments before it calls the library; the code objects of k_planes_absorb and k_planes_finish have
no scratch, no spilled VGPR, no LDS and fit their launch bounds; and the new sources leave the keys of the committed counter
records alone."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import abi_common
import codeobj
from abi_common import INVALID, PTR, limbs4

sys.path.insert(0, os.path.join(abi_common.ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402

NAMES = ["hades252_matstream_open", "hades252_matstream_absorb", "hades252_matstream_cols", "hades252_matstream_digests",
         "hades252_matstream_commit", "hades252_matstream_close"]
# (return type, [(type, name), ...]) as tools/gen_rust_ffi.py normalises the header's prototypes
PROTOTYPES = {
    "hades252_matstream_open": ("int", [("void **", "out"), ("size_t", "n_rows"), ("const uint64_t *", "capacity_mont")]),
    "hades252_matstream_absorb": ("int", [("void *", "ms"), ("const uint64_t *", "planes"), ("size_t", "n_cols"),
                                          ("size_t", "plane_stride")]),
    "hades252_matstream_cols": ("int", [("const void *", "ms"), ("uint64_t *", "n_cols_so_far")]),
    "hades252_matstream_digests": ("int", [("void *", "ms"), ("int", "pad_mode"), ("uint64_t *", "digests")]),
    "hades252_matstream_commit": ("int", [("void *", "ms"), ("int", "pad_mode"), ("int", "arity"), ("const uint64_t *", "tag_mont"),
                                          ("int", "out_idx"), ("const uint64_t *", "pad"), ("uint64_t *", "digests"),
                                          ("uint64_t *", "tree"), ("uint64_t *", "root")]),
    "hades252_matstream_close": ("int", [("void *", "ms")]),
}
NO_DEVICE, ERR_HIP = -4, -2
VGPRS_PER_SIMD = 512                     # per lane; allocated in blocks of 8
ODD = PTR + 4                            # not 8-byte aligned


def test_symbols_are_declared_bound_and_exported_host_pointers_only(hades_lib):
    abi_common.assert_declared_bound_exported(NAMES)
    text = re.sub(r"/\*.*?\*/", "", abi_common.header(), flags=re.S)
    assert sorted(re.findall(r"\bhades252_matstream_\w+", text)) == sorted(NAMES)
    assert not [n for n in NAMES if n.endswith(("_dev", "_dev_ex"))]
    assert hades_lib.hades252_strerror(NO_DEVICE) and hades_lib.hades252_strerror(ERR_HIP)
    m = re.search(r"^#define HADES252_ERR_NO_DEVICE \(?(-?\d+)\)?", abi_common.header(), flags=re.M)
    assert m is not None and int(m.group(1)) == NO_DEVICE
    m = re.search(r"^#define HADES252_ERR_HIP \(?(-?\d+)\)?", abi_common.header(), flags=re.M)
    assert m is not None and int(m.group(1)) == ERR_HIP


def test_header_says_what_the_calls_are_and_are_not():
    block = abi_common.header_block("streaming matrix commitments", "int hades252_matstream_open(",
                                    ("CONVENTION UNPINNED", "(j * plane_stride + r)", "hades252_matrix_row_digests",
                                     "hades252_matrix_commit", "NON-DESTRUCTIVE", "hades252_trim does not free",
                                     "hades252_sponge_blocks", "Host pointers only", "no device-pointer form",
                                     "no canonical-bytes form", "no witness form", "no latency form", "no openings",
                                     "one thread at a time", "even with NULL planes", "8-byte aligned", "plane_stride < n_rows",
                                     "overflows size_t", "overflows uint64_t", "no cap", "leaves the stream exactly as it was",
                                     "poisons the stream", "close always works", "HADES252_ERR_NO_DEVICE", "320", "Page-locked"))
    assert "(f13)" in block
    f12 = abi_common.header_block("column-major matrix commitments", "#define HADES252_MATRIX_MAX_COLS", ("(f13, below)",))
    assert "(f12)" in f12


def test_header_ctypes_cpp_and_rust_agree_on_the_prototypes():
    from hades252_amd import _lib
    parsed = {name: (ret, plist) for name, ret, plist in G.parse_header()[0]}
    ctype_of = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    with open(os.path.join(abi_common.ROOT, "rust", "src", "hip_sys.rs")) as f:
        rust = f.read()
    with open(os.path.join(abi_common.ROOT, "include", "hades252.hpp")) as f:
        hpp = f.read()
    for name in NAMES:
        assert parsed[name] == PROTOTYPES[name], name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(PROTOTYPES[name][1]), name
        for got, (ctype, pname) in zip(argtypes, PROTOTYPES[name][1]):
            if ctype in ctype_of:
                assert got is ctype_of[ctype], (name, pname)
            elif ctype == "void **":
                assert got is ctypes.POINTER(ctypes.c_void_p), (name, pname)
            else:                                                        # a pointer: void * or uint64_t *
                assert got in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), (name, pname)
        assert "    " + G.rust_signature(name, *PROTOTYPES[name]) + "\n" in rust, name
        assert re.search(r"\b%s\(" % name, hpp), name                   # the RAII class calls every one of them
    assert "class MatrixStream {" in hpp and "MatrixStream(const MatrixStream &) = delete;" in hpp
    assert "MatrixStream &operator=(const MatrixStream &) = delete;" in hpp and "MatrixStream(MatrixStream &&o) noexcept" in hpp


def rules_that_need_an_open_stream(lib):
    """Every argument rule of a call on an OPEN stream: HADES252_ERR_INVALID_ARG before the device is touched, and the
    stream exactly as it was.  Needs a device (the CPU tier runs it when one is in reach, the GPU tier always)."""
    cap, tag = limbs4(), limbs4(5, 6, 7, 8)
    n_rows = 4
    planes = np.zeros((3, n_rows, 4), dtype=np.uint64)
    p = ctypes.c_void_p(planes.ctypes.data)
    for rows in (1, n_rows):
        h, n = ctypes.c_void_p(), ctypes.c_uint64(77)
        assert lib.hades252_matstream_open(ctypes.byref(h), rows, cap) == 0 and h.value
        try:
            # nothing absorbed yet: nothing to finish
            assert lib.hades252_matstream_digests(h, 1, PTR) == INVALID
            assert lib.hades252_matstream_commit(h, 1, 2, tag, 1, None, None, None, PTR) == INVALID
            assert lib.hades252_matstream_cols(h, None) == INVALID
            assert lib.hades252_matstream_cols(h, ctypes.byref(n)) == 0 and n.value == 0
            # absorb
            assert lib.hades252_matstream_absorb(h, None, 0, 0) == 0 and lib.hades252_matstream_absorb(h, ODD, 0, 0) == 0
            assert lib.hades252_matstream_absorb(h, None, 3, n_rows) == INVALID
            for off in (1, 2, 4, 7):
                assert lib.hades252_matstream_absorb(h, PTR + off, 3, n_rows) == INVALID
            assert lib.hades252_matstream_absorb(h, PTR, 3, rows - 1) == INVALID                      # plane_stride < n_rows
            assert lib.hades252_matstream_absorb(h, PTR, 3, (1 << 64) // 32 // 3 + 1) == INVALID      # the byte count overflows
            assert lib.hades252_matstream_absorb(h, PTR, (1 << 64) - 1, rows) == INVALID
            assert lib.hades252_matstream_cols(h, ctypes.byref(n)) == 0 and n.value == 0
            assert lib.hades252_matstream_absorb(h, p, 3, n_rows) == 0
            assert lib.hades252_matstream_cols(h, ctypes.byref(n)) == 0 and n.value == 3
            # digests and commit
            for pad_mode in (-1, 2, 7):
                assert lib.hades252_matstream_digests(h, pad_mode, PTR) == INVALID
                assert lib.hades252_matstream_commit(h, pad_mode, 2, tag, 1, None, None, None, PTR) == INVALID
            assert lib.hades252_matstream_digests(h, 1, None) == INVALID and lib.hades252_matstream_digests(h, 1, ODD) == INVALID
            for arity in (-2, 0, 1, 5):
                assert lib.hades252_matstream_commit(h, 1, arity, tag, 1, None, None, None, PTR) == INVALID
            for out_idx in (-1, 5, 99):
                assert lib.hades252_matstream_commit(h, 1, 2, tag, out_idx, None, None, None, PTR) == INVALID
            assert lib.hades252_matstream_commit(h, 1, 2, None, 1, None, None, None, PTR) == INVALID
            assert lib.hades252_matstream_commit(h, 1, 2, tag, 1, None, None, None, None) == INVALID
            for k in range(4):                                          # pad, digests, tree, root: 8-byte aligned
                ptrs = [None, None, None, PTR]
                ptrs[k] = ODD
                assert lib.hades252_matstream_commit(h, 1, 2, tag, 1, *ptrs) == INVALID
            if rows == 1:                                               # one row: no tree
                assert lib.hades252_matstream_commit(h, 1, 2, tag, 1, None, None, None, PTR) == INVALID
            # the stream is exactly as it was: it still absorbs, counts and finishes
            d = np.zeros((rows, 4), dtype=np.uint64)
            assert lib.hades252_matstream_digests(h, 1, ctypes.c_void_p(d.ctypes.data)) == 0 and d.any()
            assert lib.hades252_matstream_cols(h, ctypes.byref(n)) == 0 and n.value == 3
        finally:
            assert lib.hades252_matstream_close(h) == 0


def test_argument_rules_answer_before_the_device(hades_lib):
    lib, cap, tag = hades_lib, limbs4(), limbs4(5, 6, 7, 8)
    h = ctypes.c_void_p(PTR)
    # open: *out = NULL on every failure
    assert lib.hades252_matstream_open(None, 4, cap) == INVALID
    for n_rows, cap_ in ((4, None), (0, cap), ((1 << 30) + 1, cap), ((1 << 64) - 1, cap)):
        h.value = PTR
        assert lib.hades252_matstream_open(ctypes.byref(h), n_rows, cap_) == INVALID and h.value is None, (n_rows, cap_)
    # a NULL stream
    n = ctypes.c_uint64(77)
    assert lib.hades252_matstream_absorb(None, PTR, 3, 4) == INVALID and lib.hades252_matstream_absorb(None, None, 0, 0) == INVALID
    assert lib.hades252_matstream_cols(None, ctypes.byref(n)) == INVALID and n.value == 77
    assert lib.hades252_matstream_digests(None, 1, PTR) == INVALID
    assert lib.hades252_matstream_commit(None, 1, 2, tag, 1, None, None, None, PTR) == INVALID
    assert lib.hades252_matstream_close(None) == 0
    if lib.hades252_device_count() <= 0:
        h.value = PTR
        assert lib.hades252_matstream_open(ctypes.byref(h), 4, cap) == NO_DEVICE and h.value is None
    else:
        rules_that_need_an_open_stream(lib)


def test_python_wrapper_refuses_bad_arguments_before_the_library(monkeypatch):
    from hades252_amd import _lib, strategy as H

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    for n_rows in (0, -1, (1 << 30) + 1, 2.0, True, None):
        with pytest.raises(ValueError):
            H.MatrixStream(n_rows, 1)
    ms = H.MatrixStream.__new__(H.MatrixStream)                          # an open stream of 8 rows, as far as Python can tell
    ms._h, ms.n_rows = ctypes.c_void_p(PTR), 8
    for planes in (np.zeros((3, 8, 4), dtype=np.int64), [[[0] * 4] * 8] * 3, np.zeros((3, 8, 2, 4), dtype=np.uint64)[:, :, 0]):
        with pytest.raises(TypeError):
            ms.absorb(planes)
    for planes in (np.zeros((3, 32), dtype=np.uint64), np.zeros((3, 8, 5), dtype=np.uint64), np.zeros((3, 7, 4), dtype=np.uint64)):
        with pytest.raises(ValueError):
            ms.absorb(planes)
    with pytest.raises(ValueError):
        ms.absorb(np.zeros((3, 9, 4), dtype=np.uint64), n_rows=9)        # not the stream's row count
    with pytest.raises(ValueError):
        ms.digests(pad_mode=2)
    for kw in ({"arity": 5}, {"arity": 1}, {"pad_mode": 3}, {"out_idx": 5}, {"pad": np.zeros((2, 4), dtype=np.uint64)}):
        args = dict(arity=2)
        args.update(kw)
        with pytest.raises(ValueError):
            ms.commit(args.pop("arity"), 3, **args)
    ms.n_rows = 1
    with pytest.raises(ValueError):
        ms.commit(2, 3)                                                  # one row: no tree
    ms._h = None                                                         # closed: every method says so, close is idempotent
    for f in (lambda: ms.absorb(np.zeros((3, 8, 4), dtype=np.uint64)), lambda: ms.cols, lambda: ms.digests(), lambda: ms.commit(2, 3)):
        with pytest.raises(ValueError, match="closed"):
            f()
    ms.close()
    with ms as same:
        assert same is ms


def test_cpp_wrapper_compiles_and_links(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "matrix_stream", r'''
#include "hades252.hpp"
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>
int main() {
    using dusk_hades::BlsScalar;
    using dusk_hades::MatrixStream;
    static_assert(!std::is_copy_constructible<MatrixStream>::value && !std::is_copy_assignable<MatrixStream>::value, "move-only");
    static_assert(std::is_nothrow_move_constructible<MatrixStream>::value && std::is_nothrow_move_assignable<MatrixStream>::value,
                  "movable");
    BlsScalar cap{};
    try {
        MatrixStream none(0, cap);                                         // refused before any device is touched
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused %d\n", e.code);
    }
    std::printf("close(NULL) %d\n", hades252_matstream_close(nullptr));
    if (hades252_device_count() <= 0) {
        try {
            MatrixStream ms(4, cap);
            std::printf("opened without a device\n");
        } catch (const dusk_hades::HadesPanic &e) {
            std::printf("no device %d\n", e.code);
        }
    } else {
        BlsScalar planes[2 * 4] = {}, digests[4], tag{};
        MatrixStream a(4, cap);
        MatrixStream ms(std::move(a));
        ms.absorb(planes, 2, 4);
        ms.digests(true, digests);
        (void)ms.commit(true, 2, tag);
        std::printf(ms.cols() == 2 && ms.n_rows() == 4 ? "streamed\n" : "wrong count\n");
    }
    return 0;
}
''')
    have = hades_lib.hades252_device_count() > 0
    assert out == ["refused -1", "close(NULL) 0", "streamed" if have else "no device -4"]


def _source(name):
    with open(os.path.join(abi_common.CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("kernel", ["k_planes_absorb", "k_planes_finish"])
def test_kernels_have_no_scratch_no_lds_and_fit_their_bounds(hades_lib, kernel):
    """By the code object's metadata only."""
    co = codeobj.load()
    names = co.kernels(kernel)
    assert len(names) == 1, sorted(co.meta)
    r = co.meta[names[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    src = _source("kernels_matrix_stream.hpp")
    minw = re.search(r"__launch_bounds__\(kBlock, (\w+)\) %s\(" % kernel, src).group(1)
    if not minw.isdigit():
        minw = re.search(r"^#define %s (\d+)$" % minw, src, flags=re.M).group(1)
    assert int(minw) == 3
    budget = VGPRS_PER_SIMD // int(minw) // 8 * 8         # __launch_bounds__(256, minw): minw waves per SIMD share 512 registers
    assert budget == 168
    assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] + r["agpr_count"] <= budget, (r, budget)
    # LDS: the kernels declare none and host_matrix_stream.hpp asks for none at the launches
    asked = re.findall(r"hipLaunchKernelGGL\(%s, dim3\(blocks_for\(\w+\)\), dim3\(kBlock\), ([^,]+)," % kernel,
                       _source("host_matrix_stream.hpp"))
    assert asked == ["0"] and r["group_segment_fixed_size"] == 0
    assert "__shared__" not in src and "__syncthreads" not in src
    print("%s: %d VGPRs, %d AGPRs, %d SGPRs, LDS %d" % (kernel, r["vgpr_count"], r["agpr_count"], r["sgpr_count"],
                                                      r["group_segment_fixed_size"]))


def test_build_lists_and_hashes_are_those_of_the_parent_commit():
    """Structurally: the new files are built (DEPS) and are in none of the lists that key a committed record, and the
    committed records carry today's hashes -- so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    new = {"kernels_matrix_stream.hpp", "host_matrix_stream.hpp"}
    assert new == set(build.MATRIX_STREAM_DEPS) and new <= set(build.DEPS)
    assert set(build.MATRIX_DEPS) == {"kernels_matrix.hpp", "host_matrix.hpp"}
    assert not new & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                         build.HOST_DEPS + build.GRIND_DEPS + build.INVERSE_DEPS + build.MATRIX_DEPS)
    assert all(os.path.exists(os.path.join(abi_common.CSRC, f)) for f in new)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    unit = _source("hades252.hip")
    assert '#include "kernels_matrix.hpp"\n#include "kernels_matrix_stream.hpp"\n' in unit
    assert '#include "host_matrix.hpp"\n#include "host_matrix_stream.hpp"\n' in unit
    assert unit.index('"kernels_inverse.hpp"') < unit.index('"kernels_matrix.hpp"') < unit.index('"kernels_witness.hpp"')
    assert unit.index('"host_inverse.hpp"') < unit.index('"host_matrix.hpp"') < unit.index('"host_cipher.hpp"')
    # the one-shot call is not rerouted: host_matrix.hpp knows nothing of the stream
    assert "k_planes_" not in _source("host_matrix.hpp") and "matstream" not in _source("host_matrix.hpp")
