"""CPU tier: the boundary of the mixed-height commitment witnesses (hades252_wmmcs_perms / _steps / _inputs / _witness)
without a GPU -- the symbols are declared, bound and exported and none ends in _dev; the header's f17 block sits after f16
and says what enters every step; header, ctypes table, C++ wrapper and generated Rust binding agree on the four prototypes;
hades252_wmmcs_perms and hades252_wmmcs_steps are pure host code and really run, against the model over a grid of shapes;
every rule that is decided before the device is touched answers here; the code objects of k_mmcs_inputs have no scratch, no
spilled VGPR, no LDS and fit their launch bounds; and the new sources leave the keys of the committed counter records
alone."""
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_common
import codeobj
import mmcs_model as MM
import mmcs_witness_model as WM
from abi_common import INVALID, PTR, limbs4

sys.path.insert(0, os.path.join(abi_common.ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402

NAMES = ["hades252_wmmcs_perms", "hades252_wmmcs_steps", "hades252_wmmcs_inputs", "hades252_wmmcs_witness"]
CU64, CV, V = "const uint64_t *", "const void *", "void *"
SHAPE = [(CU64, "heights"), (CU64, "cols"), ("size_t", "n_groups"), ("int", "arity"), ("int", "pad_mode")]
OPENINGS = [(CV, "d_rows"), (CU64, "heights"), (CU64, "cols"), ("size_t", "n_groups"), (CU64, "d_indices"), (CV, "d_paths"),
            ("size_t", "n_queries"), ("int", "arity"), (CU64, "capacity_mont"), ("int", "pad_mode"), (CU64, "tag_mont"),
            (CU64, "inject_tag_mont"), ("int", "out_idx")]
# (return type, [(type, name), ...]) as tools/gen_rust_ffi.py normalises the header's prototypes
PROTOTYPES = {
    "hades252_wmmcs_perms": ("size_t", SHAPE),
    "hades252_wmmcs_steps": ("int", SHAPE + [("uint32_t *", "steps"), ("size_t", "n_steps")]),
    "hades252_wmmcs_inputs": ("int", OPENINGS + [(V, "d_inputs"), (V, "d_roots"), (V, "stream")]),
    "hades252_wmmcs_witness": ("int", OPENINGS + [(V, "d_inputs"), (V, "d_wires"), (V, "d_roots"), (V, "stream")]),
}
NO_DEVICE = -4
VGPRS_PER_SIMD = 512                     # per lane; allocated in blocks of 8
MIS8 = PTR + 8                           # 8-byte aligned only: no device pointer
ODD = PTR + 4                            # not even that


def _p(a, offset=0):
    return ctypes.c_void_p(a.ctypes.data + offset)


def _u64(*v):
    return np.array(v, dtype=np.uint64)


def test_symbols_are_declared_bound_and_exported_and_none_ends_in_dev(hades_lib):
    abi_common.assert_declared_bound_exported(NAMES)
    text = re.sub(r"/\*.*?\*/", "", abi_common.header(), flags=re.S)
    assert sorted(set(re.findall(r"\bhades252_wmmcs_\w+", text))) == sorted(NAMES)
    assert not [n for n in NAMES if n.endswith(("_dev", "_dev_ex"))]
    assert not [n for n in NAMES if n.startswith(("hades252_mmcs_", "hades252_dmmcs_"))]
    from hades252_amd import _lib
    for value, name in enumerate(("SPONGE", "INJECT", "CLIMB")):
        m = re.search(r"^#define HADES252_WMMCS_%s (\d+) " % name, abi_common.header(), flags=re.M)
        assert m is not None and int(m.group(1)) == value == getattr(_lib, "WMMCS_" + name) == getattr(WM, name)


def test_header_says_what_enters_every_step_and_sits_after_f16():
    block = abi_common.header_block("gadget witnesses of mixed-height commitment openings", "#define HADES252_WMMCS_SPONGE",
                                    ("CONVENTION UNPINNED", "f14 / f15 / f16", "\"w\" for witness", "DEVICE\n * memory",
                                     "nothing is synchronised and nothing is downloaded", "hades252_dmmcs_verify", "HOST arrays",
                                     "fully reduced and not checked", "+ D + (G - 1) permutations", "rec = t * n + q",
                                     "step-major, query within the step", "[capacity, v0, v1, v2, v3]", "a single 1",
                                     "added into words 1..4", "[inject_tag, node, digest, 0, 0]",
                                     "digest is word 1 of the previous permutation's output", "[tag, the arity children, 0 ...]",
                                     "(index / arity^level) % arity", "word 1 of group 0's last sponge output",
                                     "not range-checked", "or 0 for a shape hades252_mmcs_verify would refuse", "Pure host code",
                                     "(kind, group, ordinal)", "n_steps other than P", "160 B", "rec * 160", "may be NULL",
                                     "byte for byte those of hades252_dmmcs_verify", "ONE launch", "hades252_perm_trace_scaled_dev",
                                     "972 * P * n scalars, wire-major", "wires == hades252_perm_witness_dev(inputs) byte for byte",
                                     "r2[out_idx] of the last step's record is the root", "NOT a\n *                           fused kernel",
                                     "n_queries = 0 is a no-op success", "16-byte\n * aligned", "above 2^30", "HADES252_ERR_HIP",
                                     "no\n * handle to poison"))
    assert "(f17)" in block
    text = abi_common.header()
    assert text.index("(f16)") < text.index("(f17)") < text.index("synthetic inputs and digests")
    # the blocks before it keep their wording: it is true of their own calls
    for f, start, end in (("(f14)", "mixed-height matrix commitments", "#define HADES252_MMCS_MAX_GROUPS"),
                          ("(f15)", "device-resident mixed-height commitments", "int hades252_dmmcs_absorb("),
                          ("(f16)", "row-major matrices for mixed-height commitments", "#define HADES252_LAYOUT_COLS")):
        old = abi_common.header_block(start, end, (f,))
        assert "no witness form" in old.lower() and "wmmcs" not in old


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
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[PROTOTYPES[name][0]], name
        assert len(argtypes) == len(PROTOTYPES[name][1]), name
        for got, (ctype, pname) in zip(argtypes, PROTOTYPES[name][1]):
            if ctype in ("int", "size_t"):
                assert got is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[ctype], (name, pname)
            else:                                                        # a pointer: void *, uint32_t * or uint64_t *
                assert got in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), (name, pname)
        assert "    " + G.rust_signature(name, *PROTOTYPES[name]) + "\n" in rust, name
        assert re.search(r"\b%s\(" % name, hpp), name                   # the wrappers call every one of them
    for name in ("SPONGE", "INJECT", "CLIMB"):
        assert "pub const HADES252_WMMCS_%s: i32 = " % name in rust
    for method in ("inline std::size_t mmcs_perms(", "inline void mmcs_steps(", "inline void mmcs_inputs_dev(",
                   "inline void mmcs_witness_dev("):
        assert method in hpp, method
    assert subprocess.run([sys.executable, os.path.join(abi_common.ROOT, "tools", "gen_rust_ffi.py"), "--check"]).returncode == 0


def _shapes():
    """(arity, heights, cols, pad_mode): arities 2 .. 4, one to three groups, a group of height 1 included, cols from
    {1, 3, 4, 5, 8}, both pad modes."""
    for arity in (2, 3, 4):
        for heights in ((arity ** 3,), (arity,), (arity ** 3, arity), (arity ** 2, 1), (arity ** 3, arity ** 2, 1),
                        (arity ** 4, arity ** 2, arity)):
            for k, cols in enumerate(itertools.product((1, 3, 4, 5, 8), repeat=len(heights))):
                if len(heights) == 3 and k % 7:                          # every seventh of the 125 triples
                    continue
                for pad_mode in (0, 1):
                    yield arity, heights, cols, pad_mode


def test_perms_and_steps_are_the_models_over_a_grid(hades_lib):
    lib, seen = hades_lib, 0
    for arity, heights, cols, pad_mode in _shapes():
        hs, cs = _u64(*heights), _u64(*cols)
        want = WM.steps(heights, cols, arity, pad_mode)
        n = lib.hades252_wmmcs_perms(_p(hs), _p(cs), len(heights), arity, pad_mode)
        assert n == len(want) == MM.permutations(cols, MM.depth_of(heights[0], arity), pad_mode), (arity, heights, cols, pad_mode)
        steps = np.full((n + 1, 3), 0xA5A5A5A5, dtype=np.uint32)
        assert lib.hades252_wmmcs_steps(_p(hs), _p(cs), len(heights), arity, pad_mode, _p(steps), n) == 0
        assert [tuple(int(v) for v in s) for s in steps[:n]] == want, (arity, heights, cols, pad_mode)
        assert (steps[n] == 0xA5A5A5A5).all()
        for bad in (n - 1, n + 1, 0):
            assert lib.hades252_wmmcs_steps(_p(hs), _p(cs), len(heights), arity, pad_mode, _p(steps), bad) == INVALID
        seen += 1
    assert seen > 300


def test_perms_and_steps_through_python_are_the_models(hades_lib):
    from hades252_amd import strategy as H
    for arity, heights, cols, pad_mode, _, _ in MM.GOLDEN_CASES:
        assert H.mmcs_perms(heights, cols, arity, pad_mode) == MM.permutations(cols, MM.depth_of(heights[0], arity), pad_mode)
        steps = H.mmcs_steps(heights, cols, arity, pad_mode)
        assert steps.dtype == np.uint32 and [tuple(int(v) for v in s) for s in steps] == WM.steps(heights, cols, arity, pad_mode)
    assert H.mmcs_perms((1 << 20, 1 << 16), (8, 4), 2) == 26             # the measured shape of tools/time_mmcs_witness.py
    for bad in (dict(heights=(8, 8)), dict(heights=(8, 3)), dict(cols=(5, 0)), dict(arity=5), dict(pad_mode=2), dict(heights=(1,), cols=(3,))):
        kw = dict(dict(heights=(8, 4), cols=(5, 3), arity=2, pad_mode=1), **bad)
        with pytest.raises(ValueError):
            H.mmcs_perms(**kw)
        with pytest.raises(ValueError):
            H.mmcs_steps(**kw)


def test_refused_shapes_give_zero_permutations_and_no_steps(hades_lib):
    lib = hades_lib
    hs, cs = _u64(8, 4, 1), _u64(5, 3, 2)
    steps = np.zeros((64, 3), dtype=np.uint32)

    def both(heights, cols, n_groups=3, arity=2, pad_mode=1):
        n = lib.hades252_wmmcs_perms(heights, cols, n_groups, arity, pad_mode)
        rc = lib.hades252_wmmcs_steps(heights, cols, n_groups, arity, pad_mode, _p(steps), 9)
        return n, rc

    assert both(_p(hs), _p(cs)) == (9, 0)
    for kw in (dict(heights=None), dict(cols=None), dict(heights=_p(hs, 4)), dict(cols=_p(cs, 4)), dict(n_groups=0), dict(n_groups=33),
               dict(arity=1), dict(arity=5), dict(pad_mode=2), dict(pad_mode=-1), dict(arity=3), dict(arity=4)):
        assert both(**dict(dict(heights=_p(hs), cols=_p(cs)), **kw)) == (0, INVALID), kw
    for heights in ((8, 4, 4), (4, 8, 1), (8, 3, 1), (8, 4, 0), (6, 2, 1), (1, 1, 1)):
        assert both(_p(_u64(*heights)), _p(cs)) == (0, INVALID), heights
    assert both(_p(_u64(1)), _p(_u64(5)), n_groups=1) == (0, INVALID)                               # heights[0] >= arity
    for cols in ((5, 0, 2), (5, 3, (1 << 30) + 1)):
        assert both(_p(hs), _p(_u64(*cols))) == (0, INVALID), cols
    assert lib.hades252_wmmcs_steps(_p(hs), _p(cs), 3, 2, 1, None, 9) == INVALID
    assert lib.hades252_wmmcs_steps(_p(hs), _p(cs), 3, 2, 1, _p(steps, 2), 9) == INVALID


def test_argument_rules_answer_before_the_device(hades_lib):
    lib, cap, tag, inj = hades_lib, limbs4(), limbs4(5, 6, 7, 8), limbs4(9, 10, 11, 12)
    # n_queries = 0 first, whatever else
    assert lib.hades252_wmmcs_inputs(None, None, None, 0, None, None, 0, 9, None, 9, None, None, 9, None, None, None) == 0
    assert lib.hades252_wmmcs_witness(None, None, None, 0, None, None, 0, 9, None, 9, None, None, 9, None, None, None, None) == 0
    hs, cs = _u64(8, 4, 1), _u64(5, 3, 2)
    good = dict(rows=PTR, heights=_p(hs), cols=_p(cs), n_groups=3, indices=PTR, paths=PTR, n_queries=4, arity=2, cap=cap,
                pad_mode=1, tag=tag, inj=inj, out_idx=1, inputs=PTR, wires=PTR, roots=PTR)

    def inputs(**kw):
        a = dict(good, **kw)
        return lib.hades252_wmmcs_inputs(a["rows"], a["heights"], a["cols"], a["n_groups"], a["indices"], a["paths"], a["n_queries"],
                                         a["arity"], a["cap"], a["pad_mode"], a["tag"], a["inj"], a["out_idx"], a["inputs"],
                                         a["roots"], None)

    def witness(**kw):
        a = dict(good, **kw)
        return lib.hades252_wmmcs_witness(a["rows"], a["heights"], a["cols"], a["n_groups"], a["indices"], a["paths"], a["n_queries"],
                                          a["arity"], a["cap"], a["pad_mode"], a["tag"], a["inj"], a["out_idx"], a["inputs"],
                                          a["wires"], a["roots"], None)

    for call in (inputs, witness):
        for name in ("rows", "heights", "cols", "indices", "paths", "cap", "tag", "inj", "inputs"):
            assert call(**{name: None}) == INVALID, name
        for name in ("rows", "paths", "inputs", "roots"):
            assert call(**{name: MIS8}) == INVALID and call(**{name: ODD}) == INVALID, name       # device pointers: 16 bytes
        assert call(indices=ODD) == INVALID
        for kw in ({"n_groups": 0}, {"n_groups": 33}, {"arity": 1}, {"arity": 5}, {"pad_mode": 2}, {"pad_mode": -1}, {"out_idx": -1},
                   {"out_idx": 5}, {"n_queries": (1 << 30) + 1}, {"n_queries": (1 << 64) - 1}):
            assert call(**kw) == INVALID, kw
        for heights in ((8, 4, 4), (4, 8, 1), (8, 3, 1), (8, 4, 0), (6, 2, 1), (1, 1, 1)):
            assert call(heights=_p(_u64(*heights))) == INVALID, heights
        assert call(heights=_p(_u64(1)), cols=_p(_u64(5)), n_groups=1) == INVALID                    # heights[0] >= arity
        assert call(arity=4) == INVALID and call(arity=3) == INVALID                                # 8 is no power of 4 or 3
        for cols in ((5, 0, 2), (5, 3, (1 << 30) + 1)):
            assert call(cols=_p(_u64(*cols))) == INVALID, cols
        assert call(heights=_p(_u64(1 << 30, 4, 1)), cols=_p(_u64(1 << 30, 1 << 30, 1 << 30)), n_queries=1 << 30) == INVALID   # bytes overflow
        # P * n_queries above 2^30: this shape has P = 9
        assert call(n_queries=(1 << 30) // 9 + 1) == INVALID and call(n_queries=1 << 30) == INVALID
    for bad in (None, MIS8, ODD):
        assert witness(wires=bad) == INVALID
    # with every rule met the device is next: none here, or a launch the caller must not make with fake pointers
    if lib.hades252_device_count() <= 0:
        assert inputs() == NO_DEVICE and witness() == NO_DEVICE and inputs(roots=None) == NO_DEVICE
        assert inputs(n_queries=(1 << 30) // 9) == NO_DEVICE


def test_python_wrappers_refuse_host_arrays_before_the_library(monkeypatch):
    import torch
    from hades252_amd import _lib, strategy as H

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    for a in (np.zeros((2, 10, 4), dtype=np.uint64), torch.zeros((2, 10, 4), dtype=torch.int64), [[[0] * 4] * 10] * 2):
        for f in (H.mmcs_inputs_dev, H.mmcs_witness_dev):
            with pytest.raises(TypeError):
                f(a, [8, 4, 1], [5, 3, 2], a, a, 2, 1, 2, 3)


def wrappers_refuse_wrong_shapes(torch, H, monkeypatch):
    """The shape rules of the Python wrappers on device tensors, before the library (the GPU tier runs this)."""
    from hades252_amd import _lib

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)

    def dev(*shape, dtype=torch.int64):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    ok = dict(rows_t=dev(2, 10, 4), heights=[8, 4, 1], cols=[5, 3, 2], indices_t=dev(2), paths_t=dev(2, 3, 1, 4), arity=2,
              capacity_mont=1, tag_mont=2, inject_tag_mont=3)
    for f in (H.mmcs_inputs_dev, H.mmcs_witness_dev):
        for kw in ({"heights": [8, 4]}, {"heights": [8, 8, 1]}, {"heights": [8, 3, 1]}, {"cols": [5, 3, 3]}, {"cols": [5, 0, 5]},
                   {"arity": 4}, {"indices_t": dev(1)}, {"paths_t": dev(2, 2, 1, 4)}, {"rows_t": dev(2, 40)}, {"pad_mode": 2},
                   {"out_idx": 5}, {"rows_t": dev(2, 10, 4, dtype=torch.int32)}):
            with pytest.raises(ValueError):
                f(**dict(ok, **kw))


def test_cpp_wrapper_compiles_and_links(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "wmmcs", r'''
#include "hades252.hpp"
#include <cstdint>
#include <cstdio>
int main() {
    using dusk_hades::BlsScalar;
    const std::uint64_t heights[3] = {8, 4, 1}, cols[3] = {5, 3, 2};
    std::uint32_t steps[27];
    std::printf("perms %zu %zu\n", dusk_hades::mmcs_perms(heights, cols, 3, 2, true), dusk_hades::mmcs_perms(heights, cols, 3, 3, true));
    dusk_hades::mmcs_steps(heights, cols, 3, 2, true, steps, 9);
    std::printf("steps %u %u %u / %u %u %u / %d\n", steps[6], steps[7], steps[8], steps[24], steps[25], steps[26], HADES252_WMMCS_CLIMB);
    BlsScalar cap{}, tag{}, inject{};
    try {
        dusk_hades::mmcs_steps(heights, cols, 3, 2, true, steps, 8);
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused %d\n", e.code);
    }
    try {
        dusk_hades::mmcs_inputs_dev(nullptr, heights, cols, 3, nullptr, nullptr, 0, 2, cap, true, tag, inject, 1, nullptr);
        dusk_hades::mmcs_witness_dev(nullptr, heights, cols, 3, nullptr, nullptr, 0, 2, cap, true, tag, inject, 1, nullptr, nullptr);
        std::printf("witnessed nothing\n");
        dusk_hades::mmcs_witness_dev(nullptr, heights, cols, 3, nullptr, nullptr, 1, 2, cap, true, tag, inject, 1, nullptr, nullptr);
        std::printf("not refused\n");
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("refused %d\n", e.code);
    }
    return 0;
}
''')
    assert out == ["perms 9 0", "steps 2 0 0 / 1 2 0 / 2", "refused -1", "witnessed nothing", "refused -1"]


def _source(name):
    with open(os.path.join(abi_common.CSRC, name)) as f:
        return f.read()


def test_kernels_have_no_scratch_no_lds_and_fit_their_bounds(hades_lib):
    """By the code object's metadata only: k_mmcs_inputs<2>, <3> and <4>."""
    co = codeobj.load()
    names = co.kernels("k_mmcs_inputs")
    assert len(names) == 3, sorted(co.meta)
    src = _source("kernels_wmmcs.hpp")
    minw = re.search(r"__launch_bounds__\(kBlock, (\d+)\) k_mmcs_inputs\(", src).group(1)
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
    # LDS: the kernel declares none and abi_wmmcs.hpp asks for none at the launch
    asked = re.findall(r"hipLaunchKernelGGL\(k_mmcs_inputs<A>, dim3\(blocks_for\(\w+\)\), dim3\(kBlock\), ([^,]+),", _source("abi_wmmcs.hpp"))
    assert asked == ["0"]
    assert "__shared__" not in src and "__syncthreads" not in src


def test_build_lists_hashes_and_launches():
    """Structurally: the new files are built (DEPS) beside the old ones and are in none of the lists that key a committed
    record or name another feature; the committed records carry today's hashes; abi_wmmcs.hpp holds ONE launch, one call of
    the witness entry point, and nothing that waits or copies; the files of f14 to f16 know nothing of the new family."""
    from hades252_amd import build
    new = ["kernels_wmmcs.hpp", "abi_wmmcs.hpp"]
    assert build.WMMCS_DEPS == new and set(new) <= set(build.DEPS)
    assert not set(new) & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.UNRECORDED_KERNEL_DEPS + build.PERM_FAST_DEPS +
                              build.HOST_DEPS + build.GRIND_DEPS + build.INVERSE_DEPS + build.MATRIX_DEPS + build.MATRIX_STREAM_DEPS +
                              build.MMCS_DEPS + build.DMMCS_DEPS + build.ROWMAJOR_DEPS)
    assert all(os.path.exists(os.path.join(abi_common.CSRC, f)) for f in new)
    with open(os.path.join(abi_common.ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1
    unit = _source("hades252.hip")
    assert '#include "kernels_rowmajor.hpp"\n#include "kernels_wmmcs.hpp"\n' in unit
    assert '#include "abi_rowmajor.hpp"\n#include "host_rowmajor.hpp"\n#include "abi_wmmcs.hpp"\n' in unit
    host = re.sub(r"//[^\n]*", "", _source("abi_wmmcs.hpp"))
    assert len(re.findall(r"hipLaunchKernelGGL\(", host)) == 1
    assert len(re.findall(r"\bhades252_perm_witness_dev\(", host)) == 1 and len(re.findall(r"\bmmcs_verify_shape\(", host)) == 1
    assert "HostCall" not in host and "hipMemcpy" not in host and "Synchronize" not in host
    for old in ("kernels_mmcs.hpp", "host_mmcs.hpp", "kernels_dmmcs.hpp", "abi_dmmcs.hpp", "kernels_rowmajor.hpp", "abi_rowmajor.hpp",
                "host_rowmajor.hpp", "kernels_witness.hpp", "abi_witness.hpp"):
        assert "wmmcs" not in _source(old) and "k_mmcs_inputs" not in _source(old), old
