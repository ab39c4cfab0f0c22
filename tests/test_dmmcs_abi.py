"""CPU tier: the boundary of the device-resident mixed-height commitments (hades252_dmmcs_absorb / _tree / _open / _verify)
without a GPU -- the symbols are declared, bound and exported; header, ctypes table, C++ wrapper and generated Rust binding
agree on the four prototypes; the header's f15 block states the ordering rule and what an index out of range gives; every
rule that is decided before the device is touched answers here (with a device in reach the rules that need a live handle are
checked too: the GPU tier calls the same function); the Python wrappers refuse host arrays before they call the library; the
code objects of k_dmmcs_absorb and k_dmmcs_rows have no scratch, no spilled VGPR, no LDS and fit their launch bounds; and the
new sources leave the keys of the committed counter records alone."""
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

NAMES = ["hades252_dmmcs_absorb", "hades252_dmmcs_tree", "hades252_dmmcs_open", "hades252_dmmcs_verify"]
CU64, CV, V = "const uint64_t *", "const void *", "void *"
PARTS = [("const void * const *", "d_planes"), (CU64, "n_rows"), (CU64, "n_cols"), (CU64, "plane_strides"), ("size_t", "n_parts")]
# (return type, [(type, name), ...]) as tools/gen_rust_ffi.py normalises the header's prototypes
PROTOTYPES = {
    "hades252_dmmcs_absorb": ("int", [(V, "mc")] + PARTS + [(V, "stream")]),
    "hades252_dmmcs_tree": ("int", [(CV, "mc"), ("const void **", "d_tree"), ("size_t *", "tree_bytes"), ("int *", "arity")]),
    "hades252_dmmcs_open": ("int", [(CV, "mc")] + PARTS + [(CU64, "d_indices"), ("size_t", "n_queries"), (V, "d_rows"),
                                                             (V, "d_paths"), (V, "stream")]),
    "hades252_dmmcs_verify": ("int", [(CV, "d_rows"), (CU64, "heights"), (CU64, "cols"), ("size_t", "n_groups"),
                                      (CU64, "d_indices"), (CV, "d_paths"), ("size_t", "n_queries"), ("int", "arity"),
                                      (CU64, "capacity_mont"), ("int", "pad_mode"), (CU64, "tag_mont"), (CU64, "inject_tag_mont"),
                                      ("int", "out_idx"), (V, "d_roots"), (V, "stream")]),
}
NO_DEVICE = -4
VGPRS_PER_SIMD = 512                     # per lane; allocated in blocks of 8
MIS8 = PTR + 8                           # 8-byte aligned only: no device pointer
ODD = PTR + 4                            # not even that


def _p(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


def _u64(*v):
    return np.array(v, dtype=np.uint64)


def test_symbols_are_declared_bound_and_exported(hades_lib):
    abi_common.assert_declared_bound_exported(NAMES)
    text = re.sub(r"/\*.*?\*/", "", abi_common.header(), flags=re.S)
    assert sorted(set(re.findall(r"\bhades252_dmmcs_\w+", text))) == sorted(NAMES)


def test_header_states_the_ordering_rule_and_what_the_calls_give():
    block = abi_common.header_block("device-resident mixed-height commitments", "int hades252_dmmcs_absorb(",
                                    ("CONVENTION UNPINNED", "f14, above", "hades252_mmcs_new", "in any mixture", "ONE launch",
                                     "shortest part first", "move at enqueue time", "Ordering rule", "orders NOTHING",
                                     "go on one stream, or the caller orders them", "the caller synchronises that stream",
                                     "hades252_mmcs_absorb, hades252_mmcs_commit, hades252_mmcs_free", "poisons the handle",
                                     "all-zero row", "all-zero path", "nothing outside the matrices and the tree is read",
                                     "ONE call of hades252_merkle_open_dev", "valid until the next", "last 32 bytes",
                                     "16-byte aligned", "HOST arrays", "occurs twice in the call", "33rd distinct height",
                                     "handle exactly as it was", "no successful commit yet", "no chunks", "tallest first"))
    assert "(f15)" in block
    # the block of f14 keeps its wording: it is true of its eight calls (tests/test_mmcs_abi.py holds the rest)
    f14 = abi_common.header_block("mixed-height matrix commitments", "#define HADES252_MMCS_MAX_GROUPS",
                                  ("Host pointers only", "no device-pointer form", "no row gather"))
    assert "(f14)" in f14 and "dmmcs" not in f14


def test_header_ctypes_cpp_and_rust_agree_on_the_prototypes():
    from hades252_amd import _lib
    parsed = {name: (ret, plist) for name, ret, plist in G.parse_header()[0]}
    with open(os.path.join(abi_common.ROOT, "rust", "src", "hip_sys.rs")) as f:
        rust = f.read()
    with open(os.path.join(abi_common.ROOT, "include", "hades252.hpp")) as f:
        hpp = f.read()
    for name in NAMES:
        assert parsed[name] == PROTOTYPES[name], (name, parsed[name])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(PROTOTYPES[name][1]), name
        for got, (ctype, pname) in zip(argtypes, PROTOTYPES[name][1]):
            if ctype in ("int", "size_t"):
                assert got is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[ctype], (name, pname)
            elif ctype == "const void **":
                assert got is ctypes.POINTER(ctypes.c_void_p), (name, pname)
            elif ctype in ("size_t *", "int *"):
                assert got is ctypes.POINTER({"size_t *": ctypes.c_size_t, "int *": ctypes.c_int}[ctype]), (name, pname)
            else:                                                        # a pointer: void * or uint64_t *
                assert got in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), (name, pname)
        assert PROTOTYPES[name][1][-1] == (V, "stream") or name == "hades252_dmmcs_tree"
        assert "    " + G.rust_signature(name, *PROTOTYPES[name]) + "\n" in rust, name
        assert re.search(r"\b%s\(" % name, hpp), name                   # the wrappers call every one of them
    for method in ("void absorb_dev(", "const void *tree_dev(", "void open_dev(", "inline void mmcs_verify_dev("):
        assert method in hpp, method


def rules_that_need_a_handle(lib):
    """Every argument rule of a call on a live handle: HADES252_ERR_INVALID_ARG before the device is touched, and the handle
    exactly as it was.  Needs a device (the CPU tier runs it when one is in reach, the GPU tier always).  The planes are fake
    pointers, never dereferenced: every call here is refused, or has nothing to do."""
    cap, tag, inj = limbs4(), limbs4(5, 6, 7, 8), limbs4(9, 10, 11, 12)
    h, n = ctypes.c_void_p(), ctypes.c_uint64(77)
    assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0 and h.value
    try:
        def absorb(planes, rows, cols, strides, n_parts=None):
            pl, r, c, s = _u64(*planes), _u64(*rows), _u64(*cols), _u64(*strides)
            return lib.hades252_dmmcs_absorb(h, _p(pl), _p(r), _p(c), _p(s), len(rows) if n_parts is None else n_parts, None)

        def open_(planes, rows, cols, strides, n_queries=1, idx=PTR, out_rows=PTR, paths=PTR, n_parts=None):
            pl, r, c, s = _u64(*planes), _u64(*rows), _u64(*cols), _u64(*strides)
            return lib.hades252_dmmcs_open(h, _p(pl), _p(r), _p(c), _p(s), len(rows) if n_parts is None else n_parts, idx, n_queries,
                                           out_rows, paths, None)

        def groups():
            out = []
            for rows in (8, 4, 2, 1):
                assert lib.hades252_mmcs_cols(h, rows, ctypes.byref(n)) == 0
                out.append(n.value)
            return out

        tree, nbytes, arity = ctypes.c_void_p(PTR), ctypes.c_size_t(77), ctypes.c_int(77)
        tree_args = (ctypes.byref(tree), ctypes.byref(nbytes), ctypes.byref(arity))
        assert lib.hades252_dmmcs_tree(h, *tree_args) == INVALID                                    # no commit yet
        assert open_([PTR], [8], [3], [8]) == INVALID                                               # open before commit
        assert absorb([PTR] * 33, range(1, 34), [1] * 33, [40] * 33) == INVALID                     # 33 parts
        assert absorb([PTR], [8], [3], [8], n_parts=0) == INVALID                                   # 0 parts
        assert absorb([PTR, PTR], [8, 8], [3, 2], [8, 8]) == INVALID                                # a height twice in one call
        assert absorb([PTR, PTR, PTR], [8, 4, 8], [3, 2, 1], [8, 8, 8]) == INVALID
        for bad in (MIS8, ODD, PTR + 1, 0):
            assert absorb([PTR, bad], [8, 4], [3, 2], [8, 4]) == INVALID                            # misaligned or NULL planes
        assert absorb([PTR, PTR], [8, 4], [3, 2], [8, 3]) == INVALID                                # stride < height
        for rows in (0, (1 << 30) + 1, (1 << 64) - 1):
            assert absorb([PTR], [rows], [3], [max(rows, 8)]) == INVALID
        assert absorb([PTR], [8], [3], [(1 << 64) // 32 // 3 + 1]) == INVALID                       # the byte count overflows
        assert groups() == [0, 0, 0, 0]                                                             # nothing was created
        # a part without columns is skipped whatever else it holds; a call of such parts only is a no-op success
        assert absorb([0, ODD], [8, 0], [0, 0], [0, 0]) == 0 and absorb([0, 0], [8, 8], [0, 0], [0, 0]) == 0
        assert groups() == [0, 0, 0, 0]
        # two real groups from the host, then the device rules on a handle that holds something
        planes = np.zeros((3, 8, 4), dtype=np.uint64)
        assert lib.hades252_mmcs_absorb(h, _p(planes), 8, 3, 8) == 0 and lib.hades252_mmcs_absorb(h, _p(planes), 4, 2, 8) == 0
        assert absorb([PTR], [8], [(1 << 64) - 3], [8]) == INVALID                                  # the column total overflows
        assert absorb([PTR, PTR], [2, 8], [1, (1 << 64) - 3], [2, 8]) == INVALID and groups() == [3, 2, 0, 0]   # ... and creates nothing
        assert open_([PTR, PTR], [8, 4], [3, 2], [8, 8]) == INVALID                                 # still no commit
        root = np.zeros(4, dtype=np.uint64)
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, None, _p(root)) == 0
        assert lib.hades252_dmmcs_tree(h, *tree_args) == 0
        assert tree.value not in (None, PTR) and tree.value % 16 == 0 and nbytes.value == 15 * 32 and arity.value == 2
        for k in range(3):
            args = list(tree_args)
            args[k] = None
            assert lib.hades252_dmmcs_tree(h, *args) == INVALID
        assert lib.hades252_dmmcs_tree(None, *tree_args) == INVALID
        # open: the heights fall strictly, are the handle's, and start at the tree's
        assert open_([PTR, PTR], [8, 4], [3, 2], [8, 8], n_queries=0) == 0 and open_([0], [5], [0], [0], n_queries=0) == 0
        for rows in ([4, 8], [8, 8], [4], [8, 2], [8, 4, 1], [16, 8], [8, 0]):
            assert open_([PTR] * len(rows), rows, [1] * len(rows), [16] * len(rows)) == INVALID, rows
        assert open_([PTR, PTR], [8, 4], [3, 2], [8, 8], n_parts=0) == INVALID
        assert open_([PTR] * 33, [8] * 33, [1] * 33, [8] * 33) == INVALID
        assert open_([PTR, PTR], [8, 4], [3, 0], [8, 8]) == INVALID and open_([PTR, PTR], [8, 4], [(1 << 30) + 1, 2], [8, 8]) == INVALID
        assert open_([PTR, PTR], [8, 4], [3, 2], [8, 3]) == INVALID and open_([PTR, PTR], [8, 4], [3, 2], [7, 4]) == INVALID
        for bad in (MIS8, ODD, 0):
            assert open_([PTR, bad], [8, 4], [3, 2], [8, 8]) == INVALID
            assert open_([PTR, PTR], [8, 4], [3, 2], [8, 8], out_rows=bad) == INVALID
            assert open_([PTR, PTR], [8, 4], [3, 2], [8, 8], paths=bad) == INVALID
        assert open_([PTR, PTR], [8, 4], [3, 2], [8, 8], idx=ODD) == INVALID and open_([PTR, PTR], [8, 4], [3, 2], [8, 8], idx=None) == INVALID
        assert open_([PTR, PTR], [8, 4], [3, 2], [8, 8], n_queries=(1 << 30) + 1) == INVALID
        assert open_([PTR, PTR], [8, 4], [3, 1 << 20], [8, 8], n_queries=1 << 11) == INVALID        # n_queries x n_cols above 2^30
        assert open_([PTR], [8], [1], [8], n_queries=(1 << 29) // 3 + 1) == INVALID                 # the paths' lanes above 2^30
        assert groups() == [3, 2, 0, 0]
        # a 33rd distinct height, counted over the call: 30 new ones fit, 31 do not
        tall = list(range(9, 40))
        assert absorb([PTR] * 31, tall, [1] * 31, [64] * 31) == INVALID and groups() == [3, 2, 0, 0]
        assert lib.hades252_mmcs_cols(h, 9, ctypes.byref(n)) == 0 and n.value == 0
    finally:
        assert lib.hades252_mmcs_free(h) == 0


def test_argument_rules_answer_before_the_device(hades_lib):
    lib, cap, tag, inj = hades_lib, limbs4(), limbs4(5, 6, 7, 8), limbs4(9, 10, 11, 12)
    one, ptrs = _u64(8), _u64(PTR)
    # a NULL handle
    assert lib.hades252_dmmcs_absorb(None, _p(ptrs), _p(one), _p(one), _p(one), 1, None) == INVALID
    assert lib.hades252_dmmcs_open(None, _p(ptrs), _p(one), _p(one), _p(one), 1, PTR, 1, PTR, PTR, None) == INVALID
    assert lib.hades252_dmmcs_open(None, None, None, None, None, 0, None, 0, None, None, None) == INVALID
    tree, nbytes, arity = ctypes.c_void_p(PTR), ctypes.c_size_t(77), ctypes.c_int(77)
    assert lib.hades252_dmmcs_tree(None, ctypes.byref(tree), ctypes.byref(nbytes), ctypes.byref(arity)) == INVALID
    assert (tree.value, nbytes.value, arity.value) == (PTR, 77, 77)
    # verify: n_queries = 0 first, then every rule, then the device
    assert lib.hades252_dmmcs_verify(None, None, None, 0, None, None, 0, 9, None, 9, None, None, 9, None, None) == 0
    hs, cs = _u64(8, 4, 1), _u64(5, 3, 2)
    good = dict(rows=PTR, heights=_p(hs), cols=_p(cs), n_groups=3, indices=PTR, paths=PTR, n_queries=4, arity=2, cap=cap,
                pad_mode=1, tag=tag, inj=inj, out_idx=1, roots=PTR)

    def verify(**kw):
        a = dict(good, **kw)
        return lib.hades252_dmmcs_verify(a["rows"], a["heights"], a["cols"], a["n_groups"], a["indices"], a["paths"], a["n_queries"],
                                         a["arity"], a["cap"], a["pad_mode"], a["tag"], a["inj"], a["out_idx"], a["roots"], None)

    for name in ("rows", "heights", "cols", "indices", "paths", "roots", "cap", "tag", "inj"):
        assert verify(**{name: None}) == INVALID, name
    for name in ("rows", "paths", "roots"):
        assert verify(**{name: MIS8}) == INVALID and verify(**{name: ODD}) == INVALID, name       # device pointers: 16 bytes
    assert verify(indices=ODD) == INVALID
    for kw in ({"n_groups": 0}, {"n_groups": 33}, {"arity": 1}, {"arity": 5}, {"pad_mode": 2}, {"pad_mode": -1}, {"out_idx": -1},
               {"out_idx": 5}, {"n_queries": (1 << 30) + 1}, {"n_queries": (1 << 64) - 1}):
        assert verify(**kw) == INVALID, kw
    for heights in ((8, 4, 4), (4, 8, 1), (8, 3, 1), (8, 4, 0), (6, 2, 1), (1, 1, 1)):
        assert verify(heights=_p(_u64(*heights))) == INVALID, heights
    assert verify(heights=_p(_u64(1)), cols=_p(_u64(5)), n_groups=1) == INVALID                      # heights[0] >= arity
    assert verify(arity=4) == INVALID and verify(arity=3) == INVALID                                # 8 is no power of 4 or 3
    for cols in ((5, 0, 2), (5, 3, (1 << 30) + 1)):
        assert verify(cols=_p(_u64(*cols))) == INVALID, cols
    assert verify(heights=_p(_u64(1 << 30, 4, 1)), cols=_p(_u64(1 << 30, 1 << 30, 1 << 30)), n_queries=1 << 30) == INVALID   # bytes overflow
    if lib.hades252_device_count() <= 0:
        assert verify() == NO_DEVICE
    else:
        rules_that_need_a_handle(lib)


def test_python_wrappers_refuse_host_arrays_before_the_library(monkeypatch):
    import torch
    from hades252_amd import _lib, strategy as H

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    mc = H.Mmcs.__new__(H.Mmcs)                                          # a live handle, as far as Python can tell
    mc._h, mc._heights = ctypes.c_void_p(PTR), [8, 4]
    host = [np.zeros((3, 8, 4), dtype=np.uint64), np.zeros((3, 8, 4), dtype=np.int64), torch.zeros((3, 8, 4), dtype=torch.int64),
            [[[0] * 4] * 8] * 3]
    for planes in host:
        with pytest.raises(TypeError):
            mc.absorb_dev([planes])
        with pytest.raises(TypeError):
            mc.absorb_dev([(planes, 8)])
        with pytest.raises(TypeError):
            mc.open_dev([planes], torch.zeros(1, dtype=torch.int64))
        with pytest.raises(TypeError):
            H.mmcs_verify_dev(planes, [8], [3], planes, planes, 2, 1, 2, 3)
    for parts in ([], None, torch.zeros((3, 8, 4), dtype=torch.int64), [torch.zeros((1, 1, 4), dtype=torch.int64)] * 33):
        with pytest.raises((TypeError, ValueError)):
            mc.absorb_dev(parts)
        with pytest.raises((TypeError, ValueError)):
            mc.open_dev(parts, torch.zeros(1, dtype=torch.int64))
    mc._h = None                                                         # closed: every method says so
    for f in (lambda: mc.absorb_dev([]), lambda: mc.open_dev([], None), lambda: mc.tree_dev()):
        with pytest.raises(ValueError, match="closed"):
            f()


def wrappers_refuse_wrong_shapes(torch, H, monkeypatch):
    """The shape rules of the Python wrappers on device tensors, before the library (the GPU tier runs this)."""
    from hades252_amd import _lib

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    mc = H.Mmcs.__new__(H.Mmcs)
    mc._h, mc._heights = ctypes.c_void_p(PTR), [8, 4]

    def dev(*shape, dtype=torch.int64):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    idx = dev(2)
    for planes in (dev(3, 32), dev(3, 8, 5), dev(3, 8, 2, 4), dev(3, 8, 4)[:, ::2]):
        with pytest.raises(ValueError):
            mc.absorb_dev([planes])
        with pytest.raises(ValueError):
            mc.open_dev([planes], idx)
    with pytest.raises(TypeError):
        mc.absorb_dev([dev(3, 8, 4, dtype=torch.int32)])
    for n_rows in (9, 0, -1, 2.0, True, (1 << 30) + 1):
        with pytest.raises(ValueError):
            mc.absorb_dev([(dev(3, 8, 4), n_rows)])
    with pytest.raises(ValueError):
        mc.absorb_dev([dev(3, 8, 4), dev(2, 8, 4)])                      # a height twice in one call
    mc._heights = list(range(1, 33))
    with pytest.raises(ValueError):
        mc.absorb_dev([dev(1, 33, 4)])                                   # a 33rd distinct height
    mc._heights = [8, 4]
    for parts in ([dev(3, 4, 4), dev(3, 8, 4)], [dev(3, 8, 4), dev(3, 2, 4)], [dev(3, 8, 4), dev(0, 4, 4)]):
        with pytest.raises(ValueError):
            mc.open_dev(parts, idx)                                      # not falling, not the handle's, no columns
    with pytest.raises(ValueError):
        mc.open_dev([dev(3, 8, 4)], dev(2, 1))
    rows, paths = dev(2, 10, 4), dev(2, 3, 1, 4)
    ok = dict(rows_t=rows, heights=[8, 4, 1], cols=[5, 3, 2], indices_t=idx, paths_t=paths, arity=2, capacity_mont=1, tag_mont=2,
              inject_tag_mont=3)
    for kw in ({"heights": [8, 4]}, {"heights": [8, 8, 1]}, {"heights": [8, 3, 1]}, {"cols": [5, 3, 3]}, {"cols": [5, 0, 5]},
               {"arity": 4}, {"indices_t": dev(1)}, {"paths_t": dev(2, 2, 1, 4)}, {"rows_t": dev(2, 40)}, {"pad_mode": 2},
               {"out_idx": 5}, {"rows_t": dev(2, 10, 4, dtype=torch.int32)}):
        with pytest.raises(ValueError):
            H.mmcs_verify_dev(**dict(ok, **kw))


def test_cpp_wrapper_compiles_and_links(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "dmmcs", r'''
#include "hades252.hpp"
#include <cstdint>
#include <cstdio>
int main() {
    using dusk_hades::BlsScalar;
    using dusk_hades::Mmcs;
    const void *planes[1] = {nullptr};
    const std::uint64_t rows[1] = {8}, cols[1] = {0}, strides[1] = {8};
    std::printf("absorb %d\n", hades252_dmmcs_absorb(nullptr, planes, rows, cols, strides, 1, nullptr));
    BlsScalar cap{}, tag{}, inject{};
    try {
        dusk_hades::mmcs_verify_dev(nullptr, rows, rows, 1, nullptr, nullptr, 0, 2, cap, true, tag, inject, 1, nullptr);
        std::printf("verified nothing\n");
        dusk_hades::mmcs_verify_dev(nullptr, rows, rows, 1, nullptr, nullptr, 1, 2, cap, true, tag, inject, 1, nullptr);
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused %d\n", e.code);
    }
    if (hades252_device_count() > 0) {
        Mmcs mc(cap);
        mc.absorb_dev(planes, rows, cols, strides, 1);                      // a part without columns: skipped
        try {
            (void)mc.tree_dev();
            std::printf("a tree before the commit\n");
        } catch (const dusk_hades::HadesPanic &e) {
            std::printf("no tree yet %d\n", e.code);
        }
        try {
            mc.open_dev(planes, rows, strides, strides, 1, nullptr, 1, nullptr, nullptr);
            std::printf("opened before the commit\n");
        } catch (const dusk_hades::HadesPanic &e) {
            std::printf("no opening yet %d\n", e.code);
        }
    }
    return 0;
}
''')
    have = hades_lib.hades252_device_count() > 0
    assert out == ["absorb -1", "verified nothing", "refused -1"] + (["no tree yet -1", "no opening yet -1"] if have else [])


def _source(name):
    with open(os.path.join(abi_common.CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("kernel", ["k_dmmcs_absorb", "k_dmmcs_rows"])
def test_kernels_have_no_scratch_no_lds_and_fit_their_bounds(hades_lib, kernel):
    """By the code object's metadata only: one instance each (neither is templated)."""
    co = codeobj.load()
    names = co.kernels(kernel)
    assert len(names) == 1, sorted(co.meta)
    src = _source("kernels_dmmcs.hpp")
    minw = re.search(r"__launch_bounds__\(kBlock, (\d+)\) %s\(" % kernel, src).group(1)
    assert int(minw) == 3
    budget = VGPRS_PER_SIMD // int(minw) // 8 * 8         # __launch_bounds__(256, minw): minw waves per SIMD share 512 registers
    assert budget == 168
    r = co.meta[names[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] + r["agpr_count"] <= budget, (r, budget)
    assert r["group_segment_fixed_size"] == 0
    print("%s: %d VGPRs, %d AGPRs, %d SGPRs, LDS %d" % (names[0], r["vgpr_count"], r["agpr_count"], r["sgpr_count"],
                                                      r["group_segment_fixed_size"]))
    # LDS: the kernels declare none and abi_dmmcs.hpp asks for none at the launches
    asked = re.findall(r"hipLaunchKernelGGL\(%s, dim3\(\(unsigned\)n_blocks\), dim3\(kBlock\), ([^,]+)," % kernel, _source("abi_dmmcs.hpp"))
    assert asked == ["0"]
    assert "__shared__" not in src and "__syncthreads" not in src


def test_build_lists_and_hashes_are_those_of_the_parent_commit():
    """Structurally: the new files are built (DEPS) and are in none of the lists that key a committed record, and the
    committed records carry today's hashes -- so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    new = ["kernels_dmmcs.hpp", "abi_dmmcs.hpp"]
    assert build.DMMCS_DEPS == new and set(new) <= set(build.DEPS)
    assert not set(new) & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                              build.HOST_DEPS + build.GRIND_DEPS + build.INVERSE_DEPS + build.MATRIX_DEPS + build.MATRIX_STREAM_DEPS +
                              build.MMCS_DEPS)
    assert all(os.path.exists(os.path.join(abi_common.CSRC, f)) for f in new)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    unit = _source("hades252.hip")
    assert '#include "kernels_mmcs.hpp"\n#include "kernels_dmmcs.hpp"\n' in unit
    assert '#include "host_mmcs.hpp"\n#include "abi_dmmcs.hpp"\n' in unit
    # every new launch lives in abi_dmmcs.hpp; the paths and the verification are the existing calls, not second kernels
    host = _source("abi_dmmcs.hpp")
    assert len(re.findall(r"hipLaunchKernelGGL\(", host)) == 2
    assert len(re.findall(r"\bhades252_merkle_open_dev\(", re.sub(r"//[^\n]*", "", host))) == 1
    assert len(re.findall(r"\bmmcs_launch_verify\(", host)) == 1 and "HostCall" not in host and "hipMemcpy" not in host
    assert "hipStreamSynchronize" not in host and "hipDeviceSynchronize" not in host
    assert "dmmcs" not in _source("kernels_matrix_stream.hpp") and "dmmcs" not in _source("host_matrix_stream.hpp")
