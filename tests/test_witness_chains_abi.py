"""CPU tier: the boundary of the chain witnesses (hades252_sponge_witness_dev, hades252_merkle_open_witness_dev) without a
GPU -- the symbols are declared, bound and exported; every argument rule answers before the device is touched; the C++
wrappers compile and link; hades252_sponge_blocks matches the model; the new sources leave the keys of the committed
counter records alone; and the code object of the sponge witness kernel in the built library has k_perm_witness's budget."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import witness_chain_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hades252_amd", "csrc")
SYMS = ["hades252_sponge_blocks", "hades252_sponge_witness_dev", "hades252_merkle_open_witness_dev"]
INVALID = -1

# fake, never dereferenced: every call below must be refused by the argument checks (or be a no-op success)
A = 0x10000            # 16-byte aligned
MIS = A + 8            # misaligned


def test_symbols_are_declared_bound_and_exported(hades_lib):
    from hades252_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hades252.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(raw, s), s


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "hades252.h")).read()
    block = text[text.index("gadget witnesses of permutation chains"):text.index("size_t hades252_sponge_blocks")]
    for needle in ("rec = s * n + i", "CONVENTION UNPINNED", "hades252_perm_witness_dev(inputs) byte for byte",
                   "selection and add gates", "2^30"):
        assert needle in block, needle
    assert text.index("int hades252_perm_witness_dev") < text.index("size_t hades252_sponge_blocks")


@pytest.mark.parametrize("pad_mode", [0, 1])
def test_sponge_blocks_matches_the_model(hades_lib, pad_mode):
    for m in list(range(0, 40)) + [1 << 20, (1 << 32) + 3]:
        assert hades_lib.hades252_sponge_blocks(m, pad_mode) == W.sponge_blocks(m, pad_mode), m
    assert hades_lib.hades252_sponge_blocks(2 ** 64 - 1, pad_mode) == (2 ** 64 - 1 + pad_mode + 3) // 4
    assert hades_lib.hades252_sponge_blocks(5, 2) == 0 and hades_lib.hades252_sponge_blocks(5, -1) == 0


def _cap():
    return (ctypes.c_uint64 * 4)(1, 2, 3, 4)


def test_sponge_witness_argument_rules(hades_lib):
    f = hades_lib.hades252_sponge_witness_dev
    cap = _cap()

    def call(msgs=A, n=5, m=3, c=cap, pad=1, inp=A, wires=A, dig=None):
        return f(msgs, n, m, c, pad, inp, wires, dig, None)

    assert call(msgs=None, n=0, c=None, pad=7, inp=None, wires=None) == 0        # n = 0: a no-op success
    for kw in ({"msgs": None}, {"c": None}, {"pad": 2}, {"pad": -1}, {"msgs": MIS}, {"dig": MIS}, {"inp": None},
               {"wires": None}, {"inp": MIS}, {"wires": MIS}, {"n": (1 << 30) + 1},
               {"n": 1 << 28, "m": 16},                      # 5 blocks x 2^28 > 2^30 records
               {"n": 1, "m": 4 << 30},                       # 2^30 + 1 blocks of one message
               {"n": 3, "m": 2 ** 64 - 1}):                  # a block count that would overflow S * n
        assert call(**kw) == INVALID, kw


def test_merkle_open_witness_argument_rules(hades_lib):
    f = hades_lib.hades252_merkle_open_witness_dev
    tag = _cap()

    def call(leaves=A, tree=A, n=16, arity=4, t=tag, pad=None, idx=A, nq=3, inp=A, wires=A, bad=None):
        return f(leaves, tree, n, arity, t, pad, idx, nq, inp, wires, bad, None)

    assert call(leaves=None, tree=None, t=None, idx=None, nq=0, inp=None, wires=None) == 0
    for kw in ({"n": 1}, {"arity": 1}, {"arity": 5}, {"n": 1, "nq": 0},      # the tree's shape first
               {"leaves": None}, {"tree": None}, {"idx": None}, {"t": None}, {"inp": None}, {"wires": None},
               {"leaves": MIS}, {"tree": MIS}, {"pad": MIS}, {"inp": MIS}, {"wires": MIS}, {"bad": A + 2},
               {"nq": (1 << 29) + 1},                        # depth 2 x (2^29 + 1) > 2^30 records
               {"nq": 2 ** 63}):
        assert call(**kw) == INVALID, kw


def test_python_layer_checks_shapes():
    from hades252_amd import strategy as H
    assert H.sponge_blocks(0, 1) == 1 and H.sponge_blocks(3, 1) == 1 and H.sponge_blocks(4, 1) == 2
    assert H.sponge_blocks(0, 0) == 1 and H.sponge_blocks(4, 0) == 1 and H.sponge_blocks(5, 0) == 2
    with pytest.raises(ValueError):
        H.sponge_blocks(3, 2)
    with pytest.raises(TypeError):                               # host memory is not a device batch
        H.sponge_witness(__import__("numpy").zeros((2, 4)), 1, 1)


def test_cpp_wrappers_compile_and_link(hades_lib, tmp_path):
    src = tmp_path / "witness.cpp"
    src.write_text(r'''
#include "hades252.hpp"
#include <cstdio>
int main() {
    using dusk_hades::BlsScalar;
    const BlsScalar cap{}, tag{};
    std::printf("%zu\n", dusk_hades::sponge_blocks(5, true));
    try {
        dusk_hades::sponge_witness(nullptr, 3, 2, cap, true, nullptr, nullptr);       // refused before the device
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("%s\n", e.what());
    }
    try {
        dusk_hades::merkle_open_witness(nullptr, nullptr, 16, 4, tag, nullptr, nullptr, 2, nullptr, nullptr);
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "witness"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", CSRC,
                    "-lhades252", "-Wl,-rpath," + CSRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "2" and len(out) == 3, out


def test_counter_records_stay_keyed():
    """The new sources stay out of build.device_source_hash and perm_fast_hash (they define no kernel of a committed counter
    record and leave every file that does byte for byte), so bench.py keeps replaying its counter-backed traffic."""
    from hades252_amd import build
    new = {"kernels_witness.hpp", "abi_witness.hpp"}
    assert new <= set(build.UNRECORDED_KERNEL_DEPS) and new <= set(build.DEPS)
    assert not new & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS + build.PERM_FAST_DEPS)
    with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as f:
        rec = json.load(f)
    assert rec["secondary_kernels"]["device_source_hash"] == build.device_source_hash()
    assert json.dumps(rec).count(build.perm_fast_hash()) >= 1


LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")


@pytest.fixture(scope="module")
def code_object(hades_lib, tmp_path_factory):
    """(resource metadata, disassembly) of the witness kernels, read from the gfx950 code object INSIDE the built library."""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not available")
    objcopy, bundler, readelf, objdump = tools
    from hades252_amd import _lib
    tmp_path = tmp_path_factory.mktemp("codeobj")
    fat, co = tmp_path / "fatbin", tmp_path / "gfx950.co"
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=%s" % fat, _lib.LIB_PATH, str(tmp_path / "scratch.so")],
                   check=True)
    subprocess.run([bundler, "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--output=%s" % co], check=True)
    notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    res = {}
    for entry in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if m is None or "witness" not in m.group(1):
            continue
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)$", entry, re.M)
                           if k in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                    "private_segment_fixed_size")}
    text = subprocess.run([objdump, "-d", str(co)], check=True, capture_output=True, text=True).stdout
    parts = re.split(r"^[0-9a-f]+ <(\S+)>:$", text, flags=re.M)
    bodies = {parts[i]: parts[i + 1] for i in range(1, len(parts), 2) if "witness" in parts[i]}
    return res, bodies


def test_sponge_witness_kernel_has_the_perm_witness_budget(code_object):
    res, bodies = code_object
    (perm,) = [k for k in bodies if "k_perm_witness" in k]
    chain = [k for k in bodies if "k_witness_sponge" in k]
    assert len(chain) == 2, sorted(bodies)                       # pad_mode 0 and 1
    ref = len(re.findall(r"\bv_mad_[iu]64_[iu]32\b", bodies[perm]))
    for name in chain:
        mads = len(re.findall(r"\bv_mad_[iu]64_[iu]32\b", bodies[name]))
        assert abs(mads - ref) <= 0.02 * ref, (name, mads, ref)
        assert "scratch_" not in bodies[name]
        r = res[name]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 152 and r["sgpr_spill_count"] <= 8, (name, r)
    for name in (k for k in res if "k_witness_path_states" in k):
        assert res[name]["private_segment_fixed_size"] == 0, (name, res[name])
