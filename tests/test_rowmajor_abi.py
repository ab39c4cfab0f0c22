"""CPU tier: the boundary of the row-major forms of the mixed-height commitments (hades252_rmmcs_absorb_rows,
hades252_rmmcs_absorb_ex, hades252_rmmcs_open_ex) without a GPU -- the symbols are declared, bound and exported; header, ctypes
table, C++ wrapper and generated Rust binding agree on the three prototypes; the header's f16 block says what a row-major part
is and what the calls give; every rule that is decided before the device is touched answers here (with a device in reach the
rules that need a live handle are checked too: the GPU tier calls the same function); the Python wrappers refuse wrong shapes
before they call the library; and the new sources are built beside the old ones, in none of the lists that key a committed
record."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import abi_common
from abi_common import INVALID, PTR, limbs4

sys.path.insert(0, os.path.join(abi_common.ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402

NAMES = ["hades252_rmmcs_absorb_rows", "hades252_rmmcs_absorb_ex", "hades252_rmmcs_open_ex"]
CU64, CU32, CV, V = "const uint64_t *", "const uint32_t *", "const void *", "void *"
PARTS = [("const void * const *", "d_mats"), (CU64, "n_rows"), (CU64, "n_cols"), (CU64, "strides"), (CU32, "layouts"), ("size_t", "n_parts")]
# (return type, [(type, name), ...]) as tools/gen_rust_ffi.py normalises the header's prototypes
PROTOTYPES = {
    "hades252_rmmcs_absorb_rows": ("int", [(V, "mc"), (CU64, "rows"), ("size_t", "n_rows"), ("size_t", "n_cols"), ("size_t", "row_stride")]),
    "hades252_rmmcs_absorb_ex": ("int", [(V, "mc")] + PARTS + [(V, "stream")]),
    "hades252_rmmcs_open_ex": ("int", [(CV, "mc")] + PARTS + [(CU64, "d_indices"), ("size_t", "n_queries"), (V, "d_rows"),
                                                                (V, "d_paths"), (V, "stream")]),
}
NO_DEVICE = -4
COLS, ROWS = 0, 1                        # HADES252_LAYOUT_COLS, HADES252_LAYOUT_ROWS
MIS8 = PTR + 8                           # 8-byte aligned only: no device pointer
ODD = PTR + 4                            # not even that


def _p(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


def _u64(*v):
    return np.array(v, dtype=np.uint64)


def _u32(*v):
    return np.array(v, dtype=np.uint32)


def test_symbols_are_declared_bound_and_exported(hades_lib):
    abi_common.assert_declared_bound_exported(NAMES)
    from hades252_amd import _lib
    for value, name in ((COLS, "COLS"), (ROWS, "ROWS")):
        m = re.search(r"^#define HADES252_LAYOUT_%s (\d+) " % name, abi_common.header(), flags=re.M)
        assert m is not None and int(m.group(1)) == value == getattr(_lib, "LAYOUT_" + name)


def test_header_says_what_a_row_major_part_is_and_what_the_calls_give():
    block = abi_common.header_block("row-major matrices for mixed-height commitments", "#define HADES252_LAYOUT_COLS",
                                    ("CONVENTION UNPINNED", "f14 / f15, above", "hades252_mmcs_new", "ROW-MAJOR PART",
                                     "base + (r * stride + j) * 32", "stride >= n_cols", "fully reduced and not checked",
                                     "DEFINED as absorbing the column-major matrix", "byte for byte", "no\n * transpose anywhere",
                                     "column total mod 4", "mix freely on one handle and one group", "HOST array",
                                     "layouts = NULL means every part is column-major", "byte-identical to hades252_dmmcs_absorb",
                                     "ONE launch", "shortest part first", "its layout included", "a layout other than 0 or 1",
                                     "strides[p] < n_cols[p]", "overflows size_t", "allocates nothing", "handle exactly as it\n * was",
                                     "16-byte aligned", "all-zero row", "all-zero path",
                                     "nothing outside the matrices and the tree is read", "Two launches", "hades252_merkle_open_dev",
                                     "one pitched 2-D\n *                            copy per tile", "one contiguous",
                                     "tile t + 1 copied while tile t is absorbed", "8-byte aligned", "33rd distinct height",
                                     "poisons the handle", "untouched and keep their own kernels"))
    assert "(f16)" in block
    text = abi_common.header()
    assert text.index("(f15)") < text.index("(f16)") < text.index("synthetic inputs and digests")


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
            if ctype == "size_t":
                assert got is ctypes.c_size_t, (name, pname)
            else:                                                        # a pointer
                assert got is ctypes.c_void_p, (name, pname)
        assert "    " + G.rust_signature(name, *PROTOTYPES[name]) + "\n" in rust, name
        assert re.search(r"\b%s\(" % name, hpp), name                   # the wrappers call every one of them
    assert "pub const HADES252_LAYOUT_COLS: i32 = 0;" in rust and "pub const HADES252_LAYOUT_ROWS: i32 = 1;" in rust
    assert "void absorb_rows(" in hpp and len(re.findall(r"void absorb_dev\(", hpp)) == 2 == len(re.findall(r"void open_dev\(", hpp))


def rules_that_need_a_handle(lib):
    """Every argument rule of the three calls on a live handle: HADES252_ERR_INVALID_ARG before the device is touched, and
    hades252_mmcs_cols unchanged after each refusal.  Needs a device (the CPU tier runs it when one is in reach, the GPU tier
    always).  The device matrices are fake pointers, never dereferenced: every device-form call here is refused, or has
    nothing to do; the host matrices that are absorbed are real and tiny."""
    cap, tag, inj = limbs4(), limbs4(5, 6, 7, 8), limbs4(9, 10, 11, 12)
    h, n = ctypes.c_void_p(), ctypes.c_uint64(77)
    assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0 and h.value
    try:
        def absorb(mats, rows, cols, strides, layouts, n_parts=None, null=None):
            a = [_u64(*mats), _u64(*rows), _u64(*cols), _u64(*strides), None if layouts is None else _u32(*layouts)]
            ptrs = [None if x is None or k == null else _p(x) for k, x in enumerate(a)]
            return lib.hades252_rmmcs_absorb_ex(h, *ptrs, len(rows) if n_parts is None else n_parts, None)

        def open_(mats, rows, cols, strides, layouts, n_queries=1, idx=PTR, out_rows=PTR, paths=PTR, n_parts=None, null=None):
            a = [_u64(*mats), _u64(*rows), _u64(*cols), _u64(*strides), None if layouts is None else _u32(*layouts)]
            ptrs = [None if x is None or k == null else _p(x) for k, x in enumerate(a)]
            return lib.hades252_rmmcs_open_ex(h, *ptrs, len(rows) if n_parts is None else n_parts, idx, n_queries, out_rows, paths, None)

        def groups(heights=(8, 4, 2, 1)):
            out = []
            for rows in heights:
                assert lib.hades252_mmcs_cols(h, rows, ctypes.byref(n)) == 0
                out.append(n.value)
            return out

        def refused(rc, want=(0, 0, 0, 0)):
            assert rc == INVALID and groups() == list(want)

        host = np.zeros((8, 5, 4), dtype=np.uint64)                      # a row-major host matrix: 8 rows, row stride 5
        # ---- on an empty handle: nothing is created by a refused call
        refused(open_([PTR], [8], [3], [3], [ROWS]))                                                # open before commit
        refused(absorb([PTR] * 33, range(1, 34), [1] * 33, [40] * 33, [ROWS] * 33))                 # 33 parts
        refused(absorb([PTR], [8], [3], [3], [ROWS], n_parts=0))                                    # 0 parts
        for k in range(4):
            refused(absorb([PTR], [8], [3], [3], [ROWS], null=k))                                   # a NULL array (layouts may be)
        for bad in (2, 3, 0xFFFFFFFF):
            refused(absorb([PTR], [8], [3], [3], [bad]))                                            # a layout that is none
            refused(absorb([PTR, PTR], [8, 4], [3, 2], [3, 4], [ROWS, bad]))
        refused(absorb([PTR], [8], [3], [2], [ROWS]))                                               # row stride < width
        refused(absorb([PTR, PTR], [8, 4], [3, 2], [8, 1], [COLS, ROWS]))
        refused(absorb([PTR], [8], [3], [7], [COLS]))                                               # plane stride < height
        refused(absorb([PTR], [8], [3], [7], None))                                                 # ... with NULL layouts
        refused(absorb([PTR], [8], [9], [8], [ROWS]))                                               # (8 would do column-major)
        refused(absorb([PTR, PTR], [8, 8], [3, 2], [3, 2], [ROWS, ROWS]))                           # a height twice in one call
        refused(absorb([PTR, PTR, PTR], [8, 4, 8], [3, 2, 1], [3, 4, 8], [ROWS, COLS, COLS]))       # ... in two layouts
        for bad in (MIS8, ODD, PTR + 1, 0):
            refused(absorb([PTR, bad], [8, 4], [3, 2], [3, 2], [ROWS, ROWS]))                       # misaligned or NULL matrix
        for rows in (0, (1 << 30) + 1, (1 << 64) - 1):
            refused(absorb([PTR], [rows], [3], [3], [ROWS]))
        refused(absorb([PTR], [8], [3], [(1 << 64) // 32 // 8 + 1], [ROWS]))                        # n_rows * stride * 32 overflows
        refused(absorb([PTR], [8], [3], [(1 << 64) // 32 // 3 + 1], [COLS]))                        # n_cols * stride * 32 overflows
        # a part without columns is skipped whatever else it holds, its layout included
        assert absorb([0, ODD], [8, 0], [0, 0], [0, 0], [7, 99]) == 0 and absorb([0, 0], [8, 8], [0, 0], [0, 0], [2, 2]) == 0
        assert groups() == [0, 0, 0, 0]
        # ---- the host form
        rows_ = lib.hades252_rmmcs_absorb_rows
        assert rows_(None, _p(host), 8, 3, 5) == INVALID
        assert rows_(h, None, 8, 0, 0) == 0 and rows_(h, None, 0, 0, 0) == 0 and groups() == [0, 0, 0, 0]   # n_cols = 0: a no-op
        refused(rows_(h, None, 8, 3, 5))
        refused(rows_(h, _p(host, 4), 8, 3, 5))                                                     # not 8-byte aligned
        refused(rows_(h, _p(host), 8, 3, 2))                                                        # row stride < width
        for rows in (0, (1 << 30) + 1, (1 << 64) - 1):
            refused(rows_(h, _p(host), rows, 3, 5))
        refused(rows_(h, _p(host), 8, 3, (1 << 64) // 32 // 8 + 1))                                 # the byte count overflows
        # two real groups, one from each host form, then the rules on a handle that holds something
        planes = np.zeros((2, 8, 4), dtype=np.uint64)
        assert rows_(h, _p(host), 8, 3, 5) == 0 and lib.hades252_mmcs_absorb(h, _p(planes), 4, 2, 8) == 0
        assert rows_(h, _p(host, 32), 4, 1, 5) == 0                                                 # both layouts feed one group
        have = (3, 3, 0, 0)
        refused(rows_(h, _p(host), 8, (1 << 64) - 3, (1 << 64) - 3), have)                          # overflow: the bytes, then the total
        refused(absorb([PTR], [8], [(1 << 64) - 3], [8], [COLS]), have)                             # the column total overflows
        refused(absorb([PTR, PTR], [2, 8], [1, (1 << 64) - 3], [1, 8], [ROWS, COLS]), have)         # ... and creates nothing
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS]), have)                      # still no commit
        root = np.zeros(4, dtype=np.uint64)
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, None, _p(root)) == 0
        # open_ex: the rules of hades252_dmmcs_open, and the layouts'
        assert open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], n_queries=0) == 0
        assert open_([0], [5], [0], [0], [9], n_queries=0) == 0 and open_([0], [5], [0], [0], None, n_queries=0) == 0
        for k in range(4):
            refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], null=k), have)
        for rows in ([4, 8], [8, 8], [4], [8, 2], [8, 4, 1], [16, 8], [8, 0]):
            refused(open_([PTR] * len(rows), rows, [1] * len(rows), [16] * len(rows), [ROWS] * len(rows)), have)
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], n_parts=0), have)
        refused(open_([PTR] * 33, [8] * 33, [1] * 33, [8] * 33, [ROWS] * 33), have)
        refused(open_([PTR, PTR], [8, 4], [3, 0], [3, 3], [ROWS, ROWS]), have)                      # no skipped part in an opening
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, 2]), have)                         # a layout that is none
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 2], [ROWS, ROWS]), have)                      # row stride < width
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, COLS]), have)                      # plane stride < height
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], None), have)
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, (1 << 64) // 32 // 4 + 1], [ROWS, ROWS]), have)
        for bad in (MIS8, ODD, 0):
            refused(open_([PTR, bad], [8, 4], [3, 3], [3, 3], [ROWS, ROWS]), have)
            refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], out_rows=bad), have)
            refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], paths=bad), have)
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], idx=ODD), have)
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], idx=None), have)
        refused(open_([PTR, PTR], [8, 4], [3, 3], [3, 3], [ROWS, ROWS], n_queries=(1 << 30) + 1), have)
        refused(open_([PTR, PTR], [8, 4], [3, 1 << 20], [3, 1 << 20], [ROWS, ROWS], n_queries=1 << 11), have)
        # a 33rd distinct height, counted over the call: 30 new ones fit, 31 do not
        tall = list(range(9, 40))
        refused(absorb([PTR] * 31, tall, [1] * 31, [64] * 31, [ROWS, COLS] * 15 + [ROWS]), have)
        assert lib.hades252_mmcs_cols(h, 9, ctypes.byref(n)) == 0 and n.value == 0
        # ... and for the host form: thirty more real groups of one column fill the handle, the 33rd height is refused
        one = np.zeros((64, 1, 4), dtype=np.uint64)
        for rows in tall[:30]:
            assert rows_(h, _p(one), rows, 1, 1) == 0
        refused(rows_(h, _p(one), tall[30], 1, 1), have)
        refused(absorb([PTR], [tall[30]], [1], [1], [ROWS]), have)
        assert groups(tall) == [1] * 30 + [0]
        assert rows_(h, _p(one), tall[0], 1, 1) == 0 and groups(tall[:1]) == [2]                    # an old height still absorbs
    finally:
        assert lib.hades252_mmcs_free(h) == 0


def test_argument_rules_answer_before_the_device(hades_lib):
    lib = hades_lib
    one, ptrs, lay = _u64(8), _u64(PTR), _u32(ROWS)
    host = np.zeros((8, 3, 4), dtype=np.uint64)
    # a NULL handle, whatever else: arrays, NULL arrays, n_parts outside 1 .. 32, nothing to do
    assert lib.hades252_rmmcs_absorb_rows(None, _p(host), 8, 3, 3) == INVALID
    assert lib.hades252_rmmcs_absorb_rows(None, None, 8, 0, 0) == INVALID
    for n_parts in (1, 0, 33):
        assert lib.hades252_rmmcs_absorb_ex(None, _p(ptrs), _p(one), _p(one), _p(one), _p(lay), n_parts, None) == INVALID
        assert lib.hades252_rmmcs_open_ex(None, _p(ptrs), _p(one), _p(one), _p(one), _p(lay), n_parts, PTR, 1, PTR, PTR, None) == INVALID
    assert lib.hades252_rmmcs_absorb_ex(None, None, None, None, None, None, 1, None) == INVALID
    assert lib.hades252_rmmcs_open_ex(None, None, None, None, None, None, 0, None, 0, None, None, None) == INVALID
    if lib.hades252_device_count() <= 0:                                 # no device, no handle: nothing else can be asked
        h = ctypes.c_void_p(PTR)
        assert lib.hades252_mmcs_new(ctypes.byref(h), limbs4()) == NO_DEVICE and not h.value
    else:
        rules_that_need_a_handle(lib)


def _no_library(monkeypatch):
    from hades252_amd import _lib

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)


def test_python_wrappers_refuse_host_arrays_before_the_library(monkeypatch):
    import torch
    from hades252_amd import strategy as H
    _no_library(monkeypatch)
    mc = H.Mmcs.__new__(H.Mmcs)                                          # a live handle, as far as Python can tell
    mc._h, mc._heights = ctypes.c_void_p(PTR), [8, 4]
    for rows in (np.zeros((8, 3, 4), dtype=np.uint64), np.zeros((8, 3, 4), dtype=np.int64), torch.zeros((8, 3, 4), dtype=torch.int64),
                 [[[0] * 4] * 3] * 8):
        with pytest.raises(TypeError):
            mc.absorb_dev([rows], [ROWS])
        with pytest.raises(TypeError):
            mc.open_dev([rows], torch.zeros(1, dtype=torch.int64), [ROWS])
    # absorb_rows: a C-contiguous uint64 [n_rows, row_stride, 4], n_cols inside the stride
    for rows in (np.zeros((8, 3, 4), dtype=np.int64), torch.zeros((8, 3, 4), dtype=torch.int64), [[[0] * 4] * 3] * 8,
                 np.zeros((8, 6, 4), dtype=np.uint64)[:, :3]):
        with pytest.raises(TypeError):
            mc.absorb_rows(rows)
    for rows in (np.zeros((8, 12), dtype=np.uint64), np.zeros((8, 3, 5), dtype=np.uint64), np.zeros((0, 3, 4), dtype=np.uint64)):
        with pytest.raises(ValueError):
            mc.absorb_rows(rows)
    for n_cols in (4, -1, 2.0, True):
        with pytest.raises(ValueError):
            mc.absorb_rows(np.zeros((8, 3, 4), dtype=np.uint64), n_cols)
    mc._heights = list(range(1, 33))
    with pytest.raises(ValueError):
        mc.absorb_rows(np.zeros((33, 1, 4), dtype=np.uint64))            # a 33rd distinct height
    mc._h = None                                                         # closed: every method says so
    for f in (lambda: mc.absorb_rows(None), lambda: mc.absorb_dev([], []), lambda: mc.open_dev([], None, [])):
        with pytest.raises(ValueError, match="closed"):
            f()


def wrappers_refuse_wrong_shapes(torch, H, monkeypatch):
    """The shape rules of the Python wrappers on row-major device tensors, before the library (the GPU tier runs this)."""
    _no_library(monkeypatch)
    mc = H.Mmcs.__new__(H.Mmcs)
    mc._h, mc._heights = ctypes.c_void_p(PTR), [8, 4]

    def dev(*shape, dtype=torch.int64):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    idx = dev(2)
    bad = [dev(8, 12), dev(8, 3, 5), dev(8, 3, 2, 4),
           dev(8, 6, 4)[:, ::2],                                         # every other scalar: stride(1) != 4
           dev(3, 8, 4).permute(1, 0, 2),                                # a column-major matrix seen as rows: stride(1) != 4
           dev(8, 3, 8)[:, :, :4],                                       # half scalars
           dev(8, 3, 4).view(-1)[1:1 + 7 * 12].view(7, 3, 4)]            # 8 bytes off: not 16-byte aligned
    for rows in bad:
        with pytest.raises(ValueError):
            mc.absorb_dev([rows], [ROWS])
        with pytest.raises(ValueError):
            mc.open_dev([rows], idx, [ROWS])
    with pytest.raises(TypeError):
        mc.absorb_dev([dev(8, 3, 4, dtype=torch.int32)], [ROWS])
    for layouts in ([2], [ROWS, ROWS], [], ROWS, [True], [None]):
        with pytest.raises(ValueError):
            mc.absorb_dev([dev(8, 3, 4)], layouts)
        with pytest.raises(ValueError):
            mc.open_dev([dev(8, 3, 4)], idx, layouts)
    with pytest.raises(ValueError):
        mc.absorb_dev([dev(8, 3, 4), dev(2, 8, 4)], [ROWS, COLS])        # a height twice in one call, in two layouts
    mc._heights = list(range(1, 33))
    with pytest.raises(ValueError):
        mc.absorb_dev([dev(33, 1, 4)], [ROWS])                           # a 33rd distinct height
    mc._heights = [8, 4]
    for parts in ([dev(4, 3, 4), dev(8, 3, 4)], [dev(8, 3, 4), dev(2, 3, 4)], [dev(8, 3, 4), dev(4, 0, 4)]):
        with pytest.raises(ValueError):
            mc.open_dev(parts, idx, [ROWS, ROWS])                        # not falling, not the handle's, no columns
    with pytest.raises(ValueError):
        mc.open_dev([dev(8, 3, 4)], dev(2, 1), [ROWS])


def _source(name):
    with open(os.path.join(abi_common.CSRC, name)) as f:
        return f.read()


def test_build_lists_hashes_and_launches():
    """Structurally: the new files are built (DEPS) beside the old ones and are in none of the lists that key a committed
    record or name another feature; the committed records carry today's hashes; the kernels keep the launch bounds of their
    siblings; abi_rowmajor.hpp holds the two new launches, one call for the paths, and nothing that waits or copies."""
    from hades252_amd import build
    new = ["kernels_rowmajor.hpp", "abi_rowmajor.hpp", "host_rowmajor.hpp"]
    assert build.ROWMAJOR_DEPS == new and set(new) <= set(build.DEPS)
    assert not set(new) & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                              build.HOST_DEPS + build.GRIND_DEPS + build.INVERSE_DEPS + build.MATRIX_DEPS + build.MATRIX_STREAM_DEPS +
                              build.MMCS_DEPS + build.DMMCS_DEPS)
    assert all(os.path.exists(os.path.join(abi_common.CSRC, f)) for f in new)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    unit = _source("hades252.hip")
    assert '#include "kernels_dmmcs.hpp"\n#include "kernels_rowmajor.hpp"\n' in unit
    assert '#include "abi_dmmcs.hpp"\n#include "abi_rowmajor.hpp"\n#include "host_rowmajor.hpp"\n' in unit
    kernels = _source("kernels_rowmajor.hpp")
    for kernel in ("k_rm_absorb", "k_rm_rows"):
        assert len(re.findall(r"__global__ void __launch_bounds__\(kBlock, 3\) %s\(" % kernel, kernels)) == 1, kernel
    assert len(re.findall(r"__global__", kernels)) == 2 and "__shared__" not in kernels and "__syncthreads" not in kernels
    host = _source("abi_rowmajor.hpp")
    assert re.findall(r"hipLaunchKernelGGL\((\w+), dim3\(\(unsigned\)n_blocks\), dim3\(kBlock\), 0,", host) == ["k_rm_absorb", "k_rm_rows"]
    assert len(re.findall(r"hipLaunchKernelGGL\(", host)) == 2
    assert len(re.findall(r"\bhades252_merkle_open_dev\(", re.sub(r"//[^\n]*", "", host))) == 1
    assert "HostCall" not in host and "hipMemcpy" not in host and "Synchronize" not in host
    # the host form: one more launch of the same absorb kernel, one pitched copy per tile or one contiguous one
    tiles = _source("host_rowmajor.hpp")
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", tiles) == ["k_rm_absorb"]
    assert len(re.findall(r"hipMemcpy2DAsync\(", tiles)) == 1 == len(re.findall(r"hipMemcpyAsync\(", tiles))
    assert "hipMemcpy2DAsync(d, gw * 32, from, row_stride * 32, gw * 32, m, hipMemcpyHostToDevice, pp.s_in)" in tiles
    # the old entry points keep their kernels: nothing of the new family in their files
    for old in ("kernels_dmmcs.hpp", "abi_dmmcs.hpp", "host_mmcs.hpp", "host_matrix_stream.hpp", "kernels_matrix_stream.hpp"):
        assert "k_rm_" not in _source(old) and "rowmajor" not in _source(old), old
