"""CPU tier: the boundary of the cipher witnesses (hades252_cipher_{encrypt,decrypt}_witness_dev) without a GPU -- the symbols
are declared, bound and exported; hades252_cipher_perms matches the model; every argument rule answers before the device is
touched; the C++ wrappers compile and link; the new code leaves the keys of the committed counter records alone; and the
code object of k_witness_cipher in the built library, both directions, has k_perm_witness's budget."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import cipher_witness_model as CW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hades252_amd", "csrc")
SYMS = ["hades252_cipher_perms", "hades252_cipher_encrypt_witness_dev", "hades252_cipher_decrypt_witness_dev"]
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
    start = text.index("gadget witnesses of the cipher")
    block = text[start:text.index("size_t hades252_cipher_perms")]
    for needle in ("CONVENTION UNPINNED", "rec = s * n", "hades252_perm_witness_dev(inputs) byte for byte", "REDUCED mod p",
                   "2^30", "may be NULL"):
        assert needle in block, needle
    # after the cipher section (whose first phrase and whose decrypt prototypes come first)
    assert text.index("int hades252_cipher_decrypt(") < start


def test_cipher_perms_matches_the_model(hades_lib):
    for m in list(range(0, 40)) + [CW.MAX_LEN - 1, CW.MAX_LEN, CW.MAX_LEN + 1, 1 << 40, 2 ** 64 - 1]:
        assert hades_lib.hades252_cipher_perms(m) == CW.cipher_perms(m), m
    assert hades_lib.hades252_cipher_perms(0) == 0 and hades_lib.hades252_cipher_perms(CW.MAX_LEN + 1) == 0


def _dom():
    return (ctypes.c_uint64 * 4)(1, 2, 3, 4)


def test_encrypt_witness_argument_rules(hades_lib):
    f = hades_lib.hades252_cipher_encrypt_witness_dev
    dom = _dom()

    def call(msgs=A, keys=A, nonces=A, n=5, m=3, d=dom, inp=A, wires=A, out=None):
        return f(msgs, keys, nonces, n, m, d, inp, wires, out, None)

    assert call(msgs=None, keys=None, nonces=None, n=0, m=0, d=None, inp=None, wires=None) == 0    # n = 0: a no-op
    for kw in ({"msgs": None}, {"keys": None}, {"nonces": None}, {"d": None}, {"m": 0}, {"m": CW.MAX_LEN + 1},
               {"msgs": MIS}, {"keys": MIS}, {"nonces": MIS}, {"out": MIS}, {"inp": None}, {"wires": None},
               {"inp": MIS}, {"wires": MIS}, {"n": (1 << 30) + 1},
               {"n": 1 << 29, "m": 5},                       # 3 permutations x 2^29 > 2^30 records
               {"n": (1 << 28) + 1, "m": 9}):               # 4 x (2^28 + 1) > 2^30
        assert call(**kw) == INVALID, kw


def test_decrypt_witness_argument_rules(hades_lib):
    f = hades_lib.hades252_cipher_decrypt_witness_dev
    dom = _dom()

    def call(ciphers=A, keys=A, nonces=A, n=5, m=3, d=dom, inp=A, wires=A, out=None, ok=None, rej=None):
        return f(ciphers, keys, nonces, n, m, d, inp, wires, out, ok, rej, None)

    assert call(ciphers=None, keys=None, nonces=None, n=0, m=0, d=None, inp=None, wires=None, rej=A + 1) == 0
    for kw in ({"ciphers": None}, {"keys": None}, {"nonces": None}, {"d": None}, {"m": 0}, {"m": CW.MAX_LEN + 1},
               {"ciphers": MIS}, {"keys": MIS}, {"nonces": MIS}, {"out": MIS}, {"rej": A + 2}, {"inp": None},
               {"wires": None}, {"inp": MIS}, {"wires": MIS}, {"n": (1 << 30) + 1},
               {"n": 1 << 29, "m": 5}, {"n": (1 << 28) + 1, "m": 9}):
        assert call(**kw) == INVALID, kw


def test_python_layer_checks_shapes():
    import numpy as np
    from hades252_amd import strategy as H
    assert H.cipher_perms(1) == 2 and H.cipher_perms(4) == 2 and H.cipher_perms(5) == 3
    for bad in (0, CW.MAX_LEN + 1):
        with pytest.raises(ValueError):
            H.cipher_perms(bad)
    with pytest.raises(TypeError):                               # host memory is not a device batch
        H.cipher_encrypt_witness(np.zeros((2, 4)), np.zeros((4, 4)), np.zeros((2, 4)), 1)
    with pytest.raises(TypeError):
        H.cipher_decrypt_witness(np.zeros((4, 4)), np.zeros((4, 4)), np.zeros((2, 4)), 1)


def test_cpp_wrappers_compile_and_link(hades_lib, tmp_path):
    src = tmp_path / "cipher_witness.cpp"
    src.write_text(r'''
#include "hades252.hpp"
#include <cstdio>
int main() {
    std::printf("%zu %zu\n", dusk_hades::cipher_perms(2), dusk_hades::cipher_perms(0));
    try {
        dusk_hades::cipher_encrypt_witness(nullptr, nullptr, nullptr, 3, 2, dusk_hades::CIPHER_DOMAIN, nullptr, nullptr);
    } catch (const dusk_hades::HadesPanic &e) {                  // refused before the device
        std::printf("%s\n", e.what());
    }
    try {
        dusk_hades::cipher_decrypt_witness(nullptr, nullptr, nullptr, 3, 2, dusk_hades::CIPHER_DOMAIN, nullptr, nullptr);
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "cipher_witness"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", CSRC,
                    "-lhades252", "-Wl,-rpath," + CSRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "2 0" and len(out) == 3, out


def test_counter_records_stay_keyed():
    """The cipher witness lives in kernels_witness.hpp / abi_witness.hpp, outside build.device_source_hash and
    perm_fast_hash, so bench.py keeps replaying its counter-backed traffic."""
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


def test_cipher_witness_kernel_has_the_perm_witness_budget(code_object):
    res, bodies = code_object
    (perm,) = [k for k in bodies if "k_perm_witness" in k]
    chain = [k for k in bodies if "k_witness_cipher" in k]
    assert len(chain) == 2, sorted(bodies)                       # encrypt and decrypt
    ref = len(re.findall(r"\bv_mad_[iu]64_[iu]32\b", bodies[perm]))
    for name in chain:
        mads = len(re.findall(r"\bv_mad_[iu]64_[iu]32\b", bodies[name]))
        assert abs(mads - ref) <= 0.02 * ref, (name, mads, ref)
        assert "scratch_" not in bodies[name]
        r = res[name]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 152 and r["sgpr_spill_count"] <= 8, (name, r)
