"""CPU tier: the boundary of the mixed-height matrix commitments (hades252_mmcs_new / _absorb / _cols / _commit / _free /
_tree_bytes / _open / _verify) without a GPU -- the symbols are declared, bound and exported, host pointers only; every rule
that is decided before the device is touched answers here (with a device in reach the rules that need a handle are checked
too: the GPU tier calls the same function); hades252_mmcs_open and hades252_mmcs_tree_bytes need no device and really run,
against the fixture; header, ctypes table, C++ wrapper and generated Rust binding agree on the eight prototypes; the Python
wrappers refuse bad arguments before they call the library; the code objects of k_mmcs_inject and k_mmcs_verify have no
scratch, no spilled VGPR, no LDS and fit their launch bounds; and the new sources leave the keys of the committed counter
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
import mmcs_model as MM
from abi_common import INVALID, PTR, limbs4

sys.path.insert(0, os.path.join(abi_common.ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402

NAMES = ["hades252_mmcs_new", "hades252_mmcs_absorb", "hades252_mmcs_cols", "hades252_mmcs_commit", "hades252_mmcs_free",
         "hades252_mmcs_tree_bytes", "hades252_mmcs_open", "hades252_mmcs_verify"]
U64, CU64 = "uint64_t *", "const uint64_t *"
# (return type, [(type, name), ...]) as tools/gen_rust_ffi.py normalises the header's prototypes
PROTOTYPES = {
    "hades252_mmcs_new": ("int", [("void **", "out"), (CU64, "capacity_mont")]),
    "hades252_mmcs_absorb": ("int", [("void *", "mc"), (CU64, "planes"), ("size_t", "n_rows"), ("size_t", "n_cols"),
                                     ("size_t", "plane_stride")]),
    "hades252_mmcs_cols": ("int", [("const void *", "mc"), ("size_t", "n_rows"), (U64, "n_cols_so_far")]),
    "hades252_mmcs_commit": ("int", [("void *", "mc"), ("int", "pad_mode"), ("int", "arity"), (CU64, "tag_mont"),
                                     (CU64, "inject_tag_mont"), ("int", "out_idx"), (U64, "tree"), (U64, "root")]),
    "hades252_mmcs_free": ("int", [("void *", "mc")]),
    "hades252_mmcs_tree_bytes": ("size_t", [("size_t", "max_rows"), ("int", "arity")]),
    "hades252_mmcs_open": ("int", [(CU64, "tree"), ("size_t", "max_rows"), ("int", "arity"), (CU64, "indices"),
                                   ("size_t", "n_queries"), (U64, "paths_out")]),
    "hades252_mmcs_verify": ("int", [(CU64, "rows"), (CU64, "heights"), (CU64, "cols"), ("size_t", "n_groups"), (CU64, "indices"),
                                     (CU64, "paths"), ("size_t", "n_queries"), ("int", "arity"), (CU64, "capacity_mont"),
                                     ("int", "pad_mode"), (CU64, "tag_mont"), (CU64, "inject_tag_mont"), ("int", "out_idx"),
                                     (U64, "roots")]),
}
NO_DEVICE, ERR_HIP = -4, -2
VGPRS_PER_SIMD = 512                     # per lane; allocated in blocks of 8
ODD = PTR + 4                            # not 8-byte aligned
SENTINEL = 0xABCDEF0123456789


def _p(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


def _u64(*v):
    return np.array(v, dtype=np.uint64)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(abi_common.ROOT, "tests", "golden", "mmcs_kat.json")) as f:
        return json.load(f)["cases"]


def test_symbols_are_declared_bound_and_exported_host_pointers_only(hades_lib):
    abi_common.assert_declared_bound_exported(NAMES)
    text = re.sub(r"/\*.*?\*/", "", abi_common.header(), flags=re.S)
    assert sorted(re.findall(r"\bhades252_mmcs_\w+", text)) == sorted(NAMES)
    assert not [n for n in NAMES if n.endswith(("_dev", "_dev_ex"))]
    m = re.search(r"^#define HADES252_MMCS_MAX_GROUPS (\d+)$", abi_common.header(), flags=re.M)
    from hades252_amd import _lib
    assert m is not None and int(m.group(1)) == _lib.MMCS_MAX_GROUPS == 32


def test_header_says_what_the_calls_are_and_are_not():
    block = abi_common.header_block("mixed-height matrix commitments", "#define HADES252_MMCS_MAX_GROUPS",
                                    ("CONVENTION UNPINNED", "h_0 > h_1 >", "hades252_matrix_row_digests", "hades252_merkle_level_dev",
                                     "perm([inject_tag, node_l[i], leaf_g[i], 0, 0])[out_idx]", "hades252_merkle_open_dev",
                                     "hades252_matstream_commit", "hades252_matstream_absorb", "32 (a^D + ... + a + 1)",
                                     "all-zero path", "NON-DESTRUCTIVE", "160 bytes of state and 32 of", "hades252_trim does not free",
                                     "interleave freely", "creates nothing", "33rd distinct height", "allocates nothing",
                                     "handle exactly as it was", "hades252_mmcs_tree_bytes(h_0, arity) bytes", "may be NULL, root may not",
                                     "query-major", "tallest first", "not range-checked", "hades252_merkle_verify_dev",
                                     "hades252_sponge_blocks", "D + (G - 1)", "ONE launch", "2^18", "Host pointers only",
                                     "no device-pointer form", "no canonical-bytes form", "no witness form", "no multiproofs",
                                     "no row gather", "one thread at a time", "even with NULL planes", "8-byte aligned",
                                     "plane_stride < n_rows", "overflows size_t", "overflows uint64_t", "poisons the handle",
                                     "free always works", "free(NULL) succeeds", "HADES252_ERR_NO_DEVICE", "plain host gather, no device"))
    assert "(f14)" in block
    # the blocks of f12 and f13 keep their wording (tests/test_matrix_abi.py and tests/test_matrix_stream_abi.py hold the rest)
    assert "(f12)" in abi_common.header_block("column-major matrix commitments", "#define HADES252_MATRIX_MAX_COLS", ("(f13, below)",))
    assert "(f13)" in abi_common.header_block("streaming matrix commitments", "int hades252_matstream_open(", ("no openings",))


def test_header_ctypes_cpp_and_rust_agree_on_the_prototypes():
    from hades252_amd import _lib
    parsed = {name: (ret, plist) for name, ret, plist in G.parse_header()[0]}
    ctype_of = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    with open(os.path.join(abi_common.ROOT, "rust", "src", "hip_sys.rs")) as f:
        rust = f.read()
    with open(os.path.join(abi_common.ROOT, "include", "hades252.hpp")) as f:
        hpp = f.read()
    for name in NAMES:
        assert parsed[name] == PROTOTYPES[name], (name, parsed[name])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctype_of[PROTOTYPES[name][0]] and len(argtypes) == len(PROTOTYPES[name][1]), name
        for got, (ctype, pname) in zip(argtypes, PROTOTYPES[name][1]):
            if ctype in ctype_of:
                assert got is ctype_of[ctype], (name, pname)
            elif ctype == "void **":
                assert got is ctypes.POINTER(ctypes.c_void_p), (name, pname)
            else:                                                        # a pointer: void * or uint64_t *
                assert got in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), (name, pname)
        assert "    " + G.rust_signature(name, *PROTOTYPES[name]) + "\n" in rust, name
        assert re.search(r"\b%s\(" % name, hpp), name                   # the wrappers call every one of them
    assert "class Mmcs {" in hpp and "Mmcs(const Mmcs &) = delete;" in hpp
    assert "Mmcs &operator=(const Mmcs &) = delete;" in hpp and "Mmcs(Mmcs &&o) noexcept" in hpp


def rules_that_need_a_handle(lib):
    """Every argument rule of a call on a live handle: HADES252_ERR_INVALID_ARG before the device is touched, and the handle
    exactly as it was.  Needs a device (the CPU tier runs it when one is in reach, the GPU tier always)."""
    cap, tag, inj = limbs4(), limbs4(5, 6, 7, 8), limbs4(9, 10, 11, 12)
    planes = np.zeros((3, 8, 4), dtype=np.uint64)
    p = _p(planes)
    h, n = ctypes.c_void_p(), ctypes.c_uint64(77)
    assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0 and h.value
    try:
        root = np.full(4, SENTINEL, dtype=np.uint64)
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, None, _p(root)) == INVALID            # no group yet
        assert lib.hades252_mmcs_cols(h, 8, None) == INVALID
        assert lib.hades252_mmcs_cols(h, 8, ctypes.byref(n)) == 0 and n.value == 0                   # no such group
        # absorb: n_cols = 0 creates nothing, whatever else is passed
        assert lib.hades252_mmcs_absorb(h, None, 8, 0, 0) == 0 and lib.hades252_mmcs_absorb(h, ODD, 0, 0, 0) == 0
        assert lib.hades252_mmcs_absorb(h, None, 8, 3, 8) == INVALID
        for off in (1, 2, 4, 7):
            assert lib.hades252_mmcs_absorb(h, PTR + off, 8, 3, 8) == INVALID
        for n_rows in (0, (1 << 30) + 1, (1 << 64) - 1):
            assert lib.hades252_mmcs_absorb(h, PTR, n_rows, 3, max(n_rows, 8)) == INVALID
        assert lib.hades252_mmcs_absorb(h, PTR, 8, 3, 7) == INVALID                                  # plane_stride < n_rows
        assert lib.hades252_mmcs_absorb(h, PTR, 8, 3, (1 << 64) // 32 // 3 + 1) == INVALID           # the byte count overflows
        n.value = 77
        assert lib.hades252_mmcs_cols(h, 8, ctypes.byref(n)) == 0 and n.value == 0
        assert lib.hades252_mmcs_absorb(h, p, 8, 3, 8) == 0 and lib.hades252_mmcs_absorb(h, p, 3, 2, 8) == 0
        assert lib.hades252_mmcs_absorb(h, PTR, 8, (1 << 64) - 3, 8) == INVALID                      # the column total overflows
        assert lib.hades252_mmcs_cols(h, 8, ctypes.byref(n)) == 0 and n.value == 3
        assert lib.hades252_mmcs_cols(h, 3, ctypes.byref(n)) == 0 and n.value == 2
        # commit: heights 8 and 3 -- 3 is no power of two, 8 no power of three
        for arity in (2, 3, 4):
            assert lib.hades252_mmcs_commit(h, 1, arity, tag, inj, 1, None, _p(root)) == INVALID
    finally:
        assert lib.hades252_mmcs_free(h) == 0
    assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0 and h.value
    try:
        assert lib.hades252_mmcs_absorb(h, p, 1, 3, 8) == 0
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, None, _p(root)) == INVALID             # the tallest is below the arity
        assert lib.hades252_mmcs_absorb(h, p, 4, 3, 8) == 0
        for pad_mode in (-1, 2, 7):
            assert lib.hades252_mmcs_commit(h, pad_mode, 2, tag, inj, 1, None, _p(root)) == INVALID
        for arity in (-2, 0, 1, 5):
            assert lib.hades252_mmcs_commit(h, 1, arity, tag, inj, 1, None, _p(root)) == INVALID
        assert lib.hades252_mmcs_commit(h, 1, 3, tag, inj, 1, None, _p(root)) == INVALID             # 4 is no power of 3
        for out_idx in (-1, 5, 99):
            assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, out_idx, None, _p(root)) == INVALID
        assert lib.hades252_mmcs_commit(h, 1, 2, None, inj, 1, None, _p(root)) == INVALID
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, None, 1, None, _p(root)) == INVALID
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, None, None) == INVALID
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, ODD, _p(root)) == INVALID
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, None, ODD) == INVALID
        assert (root == SENTINEL).all()
        # a 33rd distinct height
        for rows in (2, 3, 5, 6, 7, 8):
            assert lib.hades252_mmcs_absorb(h, p, rows, 1, 8) == 0
        tall = np.zeros((1, 40, 4), dtype=np.uint64)
        for rows in range(9, 33):
            assert lib.hades252_mmcs_absorb(h, _p(tall), rows, 1, 40) == 0                           # 32 groups: 1 .. 32 rows
        assert lib.hades252_mmcs_absorb(h, _p(tall), 33, 1, 40) == INVALID
        assert lib.hades252_mmcs_cols(h, 33, ctypes.byref(n)) == 0 and n.value == 0
        assert lib.hades252_mmcs_absorb(h, _p(tall), 32, 1, 40) == 0                                 # a known height still absorbs
        assert lib.hades252_mmcs_cols(h, 32, ctypes.byref(n)) == 0 and n.value == 2
        assert lib.hades252_mmcs_cols(h, 4, ctypes.byref(n)) == 0 and n.value == 3                   # exactly as it was
    finally:
        assert lib.hades252_mmcs_free(h) == 0
    # the handle of the first checks still commits: heights 4 and 1
    assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0
    try:
        assert lib.hades252_mmcs_absorb(h, p, 4, 3, 8) == 0 and lib.hades252_mmcs_absorb(h, p, 1, 2, 8) == 0
        assert lib.hades252_mmcs_commit(h, 1, 3, tag, inj, 1, None, _p(root)) == INVALID and (root == SENTINEL).all()
        assert lib.hades252_mmcs_commit(h, 1, 2, tag, inj, 1, None, _p(root)) == 0 and (root != SENTINEL).all()
    finally:
        assert lib.hades252_mmcs_free(h) == 0


def test_argument_rules_answer_before_the_device(hades_lib):
    lib, cap, tag, inj = hades_lib, limbs4(), limbs4(5, 6, 7, 8), limbs4(9, 10, 11, 12)
    h = ctypes.c_void_p(PTR)
    # new: *out = NULL on every failure
    assert lib.hades252_mmcs_new(None, cap) == INVALID
    assert lib.hades252_mmcs_new(ctypes.byref(h), None) == INVALID and h.value is None
    # a NULL handle
    n = ctypes.c_uint64(77)
    assert lib.hades252_mmcs_absorb(None, PTR, 8, 3, 8) == INVALID and lib.hades252_mmcs_absorb(None, None, 0, 0, 0) == INVALID
    assert lib.hades252_mmcs_cols(None, 8, ctypes.byref(n)) == INVALID and n.value == 77
    assert lib.hades252_mmcs_commit(None, 1, 2, tag, inj, 1, None, PTR) == INVALID
    assert lib.hades252_mmcs_free(None) == 0
    # verify: n_queries = 0 first, then every rule, then the device
    assert lib.hades252_mmcs_verify(None, None, None, 0, None, None, 0, 9, None, 9, None, None, 9, None) == 0
    hs, cs = _u64(8, 4, 1), _u64(5, 3, 2)
    good = dict(rows=PTR, heights=_p(hs), cols=_p(cs), n_groups=3, indices=PTR, paths=PTR, n_queries=4, arity=2, cap=cap,
                pad_mode=1, tag=tag, inj=inj, out_idx=1, roots=PTR)

    def verify(**kw):
        a = dict(good, **kw)
        return lib.hades252_mmcs_verify(a["rows"], a["heights"], a["cols"], a["n_groups"], a["indices"], a["paths"], a["n_queries"],
                                        a["arity"], a["cap"], a["pad_mode"], a["tag"], a["inj"], a["out_idx"], a["roots"])

    for name in ("rows", "heights", "cols", "indices", "paths", "roots", "cap", "tag", "inj"):
        assert verify(**{name: None}) == INVALID, name
    for name in ("rows", "indices", "paths", "roots"):
        assert verify(**{name: ODD}) == INVALID, name
    big = np.zeros(8, dtype=np.uint64)
    big[1:4], big[5:8] = hs, cs
    assert verify(heights=_p(big, 4)) == INVALID and verify(cols=_p(big, 36)) == INVALID          # misaligned tables
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
    # open: no device at all
    assert lib.hades252_mmcs_open(None, 0, 0, None, 0, None) == 0
    for kw in ((None, 8, 2, PTR, 1, PTR), (PTR, 8, 2, None, 1, PTR), (PTR, 8, 2, PTR, 1, None), (ODD, 8, 2, PTR, 1, PTR),
               (PTR, 8, 2, ODD, 1, PTR), (PTR, 8, 2, PTR, 1, ODD), (PTR, 6, 2, PTR, 1, PTR), (PTR, 1, 2, PTR, 1, PTR),
               (PTR, 0, 2, PTR, 1, PTR), (PTR, 8, 3, PTR, 1, PTR), (PTR, 8, 1, PTR, 1, PTR), (PTR, 8, 5, PTR, 1, PTR),
               (PTR, 1 << 31, 2, PTR, 1, PTR), (PTR, 8, 2, PTR, (1 << 64) // 32 // 3 + 1, PTR)):
        assert lib.hades252_mmcs_open(*kw) == INVALID, kw
    if lib.hades252_device_count() <= 0:
        h.value = PTR
        assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == NO_DEVICE and h.value is None
        assert verify() == NO_DEVICE
    else:
        rules_that_need_a_handle(lib)


def test_tree_bytes_and_open_run_without_a_device(hades_lib, H, golden):
    lib = hades_lib
    for arity in (2, 3, 4):
        for d in range(1, 6):
            want = 32 * sum(arity ** l for l in range(d + 1))
            assert lib.hades252_mmcs_tree_bytes(arity ** d, arity) == want == H.mmcs_tree_bytes(arity ** d, arity)
            assert want == 32 * MM.tree_nodes(arity ** d, arity)
        for bad in (0, 1, arity + 1, arity ** 2 + arity, (1 << 64) - 1):
            assert lib.hades252_mmcs_tree_bytes(bad, arity) == 0, (bad, arity)
    assert lib.hades252_mmcs_tree_bytes(1 << 30, 2) == 32 * ((1 << 31) - 1) and lib.hades252_mmcs_tree_bytes(1 << 30, 4) == 32 * (((1 << 32) - 1) // 3)
    assert lib.hades252_mmcs_tree_bytes(1 << 31, 2) == 0 and lib.hades252_mmcs_tree_bytes(3 ** 19, 3) == 0   # above 2^30 rows
    for bad in (-1, 0, 1, 5):
        assert lib.hades252_mmcs_tree_bytes(16, bad) == 0
    # the one-group case: the tree of f13 behind the digests
    assert lib.hades252_mmcs_tree_bytes(16, 2) == 16 * 32 + lib.hades252_merkle_tree_bytes(16, 2)
    for c in golden:
        arity, h0 = c["arity"], c["heights"][0]
        tree = MM.unhex(c["tree"])
        assert tree.nbytes == lib.hades252_mmcs_tree_bytes(h0, arity)
        depth = MM.depth_of(h0, arity)
        idx = np.array(list(range(h0)) + [h0, c["opening"]["index"], 0, (1 << 64) - 1, c["opening"]["index"]], dtype=np.uint64)
        want = MM.open_paths(tree, h0, arity, idx.tolist())
        assert want[c["opening"]["index"]].tobytes() == MM.unhex(c["opening"]["path"]).tobytes()
        guard = 3
        out = np.full((idx.size + 2 * guard, depth, arity - 1, 4), SENTINEL, dtype=np.uint64)     # sentinel rows around the output
        assert lib.hades252_mmcs_open(_p(tree), h0, arity, _p(idx), idx.size, _p(out, guard * depth * (arity - 1) * 32)) == 0
        assert (out[:guard] == SENTINEL).all() and (out[guard + idx.size:] == SENTINEL).all()
        assert out[guard:guard + idx.size].tobytes() == want.tobytes()
        assert not out[guard + h0].any() and not out[guard + h0 + 3].any()                         # an index >= h_0: zeros
        assert H.mmcs_open(tree, h0, arity, idx).tobytes() == want.tobytes()


def test_python_wrappers_refuse_bad_arguments_before_the_library(monkeypatch):
    from hades252_amd import _lib, strategy as H

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    mc = H.Mmcs.__new__(H.Mmcs)                                          # a live handle, as far as Python can tell
    mc._h, mc._heights = ctypes.c_void_p(PTR), [8, 4]
    for planes in (np.zeros((3, 8, 4), dtype=np.int64), [[[0] * 4] * 8] * 3, np.zeros((3, 8, 2, 4), dtype=np.uint64)[:, :, 0]):
        with pytest.raises(TypeError):
            mc.absorb(planes)
    for planes in (np.zeros((3, 32), dtype=np.uint64), np.zeros((3, 8, 5), dtype=np.uint64)):
        with pytest.raises(ValueError):
            mc.absorb(planes)
    for n_rows in (9, 0, -1, 2.0, True, (1 << 30) + 1):
        with pytest.raises(ValueError):
            mc.absorb(np.zeros((3, 8, 4), dtype=np.uint64), n_rows=n_rows)
    for n_rows in (0, -1, 2.0, True, None, (1 << 30) + 1):
        with pytest.raises(ValueError):
            mc.cols(n_rows)
    assert mc.heights == [8, 4]
    for kw in ({"arity": 5}, {"arity": 1}, {"arity": 3}, {"arity": 4}, {"pad_mode": 3}, {"out_idx": 5}, {"out_idx": True}):
        args = dict(arity=2)
        args.update(kw)
        with pytest.raises(ValueError):
            mc.commit(args.pop("arity"), 3, 4, **args)
    mc._heights = [1]
    with pytest.raises(ValueError):
        mc.commit(2, 3, 4)                                               # the tallest is below the arity
    mc._heights = []
    with pytest.raises(ValueError):
        mc.commit(2, 3, 4)                                               # nothing absorbed
    mc._heights = list(range(1, 33))
    with pytest.raises(ValueError):
        mc.absorb(np.zeros((1, 33, 4), dtype=np.uint64))                 # a 33rd distinct height
    mc._h = None                                                         # closed: every method says so, close is idempotent
    for f in (lambda: mc.absorb(np.zeros((3, 8, 4), dtype=np.uint64)), lambda: mc.cols(8), lambda: mc.commit(2, 3, 4)):
        with pytest.raises(ValueError, match="closed"):
            f()
    mc.close()
    with mc as same:
        assert same is mc
    # mmcs_open and mmcs_verify
    tree = np.zeros((15, 4), dtype=np.uint64)
    for args in ((tree, 8, 5, [0]), (tree, 6, 2, [0]), (tree, 1, 2, [0]), (tree, 8.0, 2, [0]), (tree[:14], 8, 2, [0]),
                 (tree, 16, 2, [0]), (tree, 1 << 31, 2, [0])):
        with pytest.raises(ValueError):
            H.mmcs_open(*args)
    with pytest.raises(TypeError):
        H.mmcs_open(tree.astype(np.int64), 8, 2, [0])
    rows, paths = np.zeros((2, 10, 4), dtype=np.uint64), np.zeros((2, 3, 1, 4), dtype=np.uint64)
    ok = dict(rows=rows, heights=[8, 4, 1], cols=[5, 3, 2], indices=[0, 1], paths=paths, arity=2, capacity_mont=1, tag_mont=2,
              inject_tag_mont=3)
    for kw in ({"heights": [8, 4]}, {"heights": [8, 8, 1]}, {"heights": [4, 8, 1]}, {"heights": [8, 3, 1]}, {"heights": [8, 4, 0]},
               {"heights": []}, {"heights": [1], "cols": [10]}, {"cols": [5, 3, 3]}, {"cols": [5, 0, 5]}, {"arity": 4}, {"arity": 1},
               {"indices": [0]}, {"paths": paths[:1]}, {"paths": np.zeros((2, 2, 1, 4), dtype=np.uint64)},
               {"rows": np.zeros((2, 40), dtype=np.uint64)}, {"pad_mode": 2}, {"out_idx": 5},
               {"heights": [1 << 33] + [1 << k for k in range(31, -1, -1)], "cols": [1] * 33}):
        with pytest.raises(ValueError):
            H.mmcs_verify(**dict(ok, **kw))
    with pytest.raises(TypeError):
        H.mmcs_verify(**dict(ok, rows=rows.astype(np.int64)))


def test_cpp_wrapper_compiles_and_links(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "mmcs", r'''
#include "hades252.hpp"
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>
int main() {
    using dusk_hades::BlsScalar;
    using dusk_hades::Mmcs;
    static_assert(!std::is_copy_constructible<Mmcs>::value && !std::is_copy_assignable<Mmcs>::value, "move-only");
    static_assert(std::is_nothrow_move_constructible<Mmcs>::value && std::is_nothrow_move_assignable<Mmcs>::value, "movable");
    BlsScalar cap{}, tag{}, inject{};
    std::printf("tree bytes %zu %zu\n", dusk_hades::mmcs_tree_bytes(8, 2), dusk_hades::mmcs_tree_bytes(6, 2));
    BlsScalar tree[15] = {}, path[3];
    tree[1].limbs[0] = 7;
    const std::uint64_t index = 0;
    dusk_hades::mmcs_open(tree, 8, 2, &index, 1, path);                    // plain host code
    std::printf("sibling %llu\n", (unsigned long long)path[0].limbs[0]);
    try {
        dusk_hades::mmcs_open(tree, 6, 2, &index, 1, path);
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused %d\n", e.code);
    }
    std::printf("free(NULL) %d\n", hades252_mmcs_free(nullptr));
    if (hades252_device_count() <= 0) {
        try {
            Mmcs mc(cap);
            std::printf("made without a device\n");
        } catch (const dusk_hades::HadesPanic &e) {
            std::printf("no device %d\n", e.code);
        }
    } else {
        BlsScalar planes[2 * 4] = {}, roots[1], rows[3] = {};
        Mmcs a(cap);
        Mmcs mc(std::move(a));
        mc.absorb(planes, 4, 2, 4);
        mc.absorb(planes, 1, 1, 4);
        BlsScalar all[7];
        const BlsScalar root = mc.commit(true, 2, tag, inject, 1, all);
        BlsScalar p2[2];
        dusk_hades::mmcs_open(all, 4, 2, &index, 1, p2);
        const std::uint64_t heights[2] = {4, 1}, cols[2] = {2, 1};
        dusk_hades::mmcs_verify(rows, heights, cols, 2, &index, p2, 1, 2, cap, true, tag, inject, 1, roots);
        bool same = mc.cols(4) == 2 && mc.cols(1) == 1 && mc.cols(2) == 0;
        for (int k = 0; k < 4; k++) same = same && roots[0].limbs[k] == root.limbs[k] && all[6].limbs[k] == root.limbs[k];
        std::printf(same ? "committed and verified\n" : "wrong root\n");
    }
    return 0;
}
''')
    have = hades_lib.hades252_device_count() > 0
    assert out == ["tree bytes 480 0", "sibling 7", "refused -1", "free(NULL) 0", "committed and verified" if have else "no device -4"]


def _source(name):
    with open(os.path.join(abi_common.CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("kernel,instances", [("k_mmcs_inject", 1), ("k_mmcs_verify", 3)])
def test_kernels_have_no_scratch_no_lds_and_fit_their_bounds(hades_lib, kernel, instances):
    """By the code object's metadata only."""
    co = codeobj.load()
    names = co.kernels(kernel)
    assert len(names) == instances, sorted(co.meta)
    src = _source("kernels_mmcs.hpp")
    minw = re.search(r"__launch_bounds__\(kBlock, (\d+)\) %s\(" % kernel, src).group(1)
    assert int(minw) == 3
    budget = VGPRS_PER_SIMD // int(minw) // 8 * 8         # __launch_bounds__(256, minw): minw waves per SIMD share 512 registers
    assert budget == 168
    for name in names:
        r = co.meta[name]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
        assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] + r["agpr_count"] <= budget, (r, budget)
        assert r["group_segment_fixed_size"] == 0
        print("%s: %d VGPRs, %d AGPRs, %d SGPRs, LDS %d" % (name, r["vgpr_count"], r["agpr_count"], r["sgpr_count"],
                                                          r["group_segment_fixed_size"]))
    # LDS: the kernels declare none and host_mmcs.hpp asks for none at the launches
    asked = re.findall(r"hipLaunchKernelGGL\(%s(?:<A>)?, dim3\(blocks_for\(\w+\)\), dim3\(kBlock\), ([^,]+)," % kernel,
                       _source("host_mmcs.hpp"))
    assert asked == ["0"]
    assert "__shared__" not in src and "__syncthreads" not in src


def test_build_lists_and_hashes_are_those_of_the_parent_commit():
    """Structurally: the new files are built (DEPS) and are in none of the lists that key a committed record, and the
    committed records carry today's hashes -- so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    new = {"kernels_mmcs.hpp", "host_mmcs.hpp"}
    assert new == set(build.MMCS_DEPS) and new <= set(build.DEPS)
    assert not new & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                         build.HOST_DEPS + build.GRIND_DEPS + build.INVERSE_DEPS + build.MATRIX_DEPS + build.MATRIX_STREAM_DEPS)
    assert all(os.path.exists(os.path.join(abi_common.CSRC, f)) for f in new)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    unit = _source("hades252.hip")
    assert '#include "kernels_matrix_stream.hpp"\n#include "kernels_mmcs.hpp"\n' in unit
    assert '#include "host_matrix_stream.hpp"\n#include "host_mmcs.hpp"\n' in unit
    # the streams are called, not edited: host_matrix_stream.hpp knows nothing of this file
    assert "mmcs" not in _source("host_matrix_stream.hpp") and "mmcs" not in _source("kernels_matrix_stream.hpp")
    host = _source("host_mmcs.hpp")
    assert "mstream_absorb_tiles(ms, planes, n_cols, plane_stride)" in host and "hades252_merkle_level_dev(" in host
    assert "hades252_merkle_build_dev(" in host
