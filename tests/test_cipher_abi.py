"""CPU tier: the boundary of the batched Poseidon cipher (hades252_cipher_*) without a GPU -- the symbols are declared,
bound and exported; every argument rule answers before the device is touched; the C++ wrappers compile and link; the code
object of k_cipher / k_cipher_lanes in the built library has no scratch and fits its launch bounds; and the cipher's sources
leave the key of the committed secondary-kernel counter record alone."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hades252_amd", "csrc")
SYMS = ["hades252_cipher_encrypt_dev", "hades252_cipher_decrypt_dev", "hades252_cipher_encrypt", "hades252_cipher_decrypt"]
INVALID = -1

# fake, never dereferenced: every call below must be refused by the argument checks
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
    assert "#define HADES252_CIPHER_MAX_LEN 1024" in open(os.path.join(ROOT, "include", "hades252.h")).read()
    assert _lib.CIPHER_MAX_LEN == 1024


def test_header_says_convention_unpinned():
    text = open(os.path.join(ROOT, "include", "hades252.h")).read()
    block = text[text.index("batched Poseidon cipher"):text.index("#define HADES252_CIPHER_MAX_LEN")]
    assert "CONVENTION UNPINNED" in block and "hades252_from_bytes_dev" in block


def _dom():
    return (ctypes.c_uint64 * 4)(1, 2, 3, 4)


def test_device_entry_points_argument_rules(hades_lib):
    enc, dec = hades_lib.hades252_cipher_encrypt_dev, hades_lib.hades252_cipher_decrypt_dev
    d = _dom()

    def e(msgs=A, keys=A, nonces=A, n=5, m=2, dom=d, out=A):
        return enc(msgs, keys, nonces, n, m, dom, out, None)

    def x(c=A, keys=A, nonces=A, n=5, m=2, dom=d, out=A, ok=A, rej=None):
        return dec(c, keys, nonces, n, m, dom, out, ok, rej, None)

    # n = 0: a no-op success, whatever else is passed
    assert e(msgs=None, keys=None, nonces=None, n=0, m=0, dom=None, out=None) == 0
    assert x(c=None, keys=None, nonces=None, n=0, m=0, dom=None, out=None, ok=None) == 0
    for kw in ({"msgs": None}, {"keys": None}, {"nonces": None}, {"out": None}, {"dom": None}, {"m": 0}, {"m": 1025},
               {"msgs": MIS}, {"keys": MIS}, {"nonces": MIS}, {"out": MIS}, {"n": (1 << 30) + 1}):
        assert e(**kw) == INVALID, kw
    for kw in ({"c": None}, {"keys": None}, {"nonces": None}, {"out": None}, {"ok": None}, {"dom": None}, {"m": 0},
               {"m": 1025}, {"c": MIS}, {"keys": MIS}, {"nonces": MIS}, {"out": MIS}, {"rej": A + 2},
               {"n": (1 << 30) + 1}):
        assert x(**kw) == INVALID, kw


def test_host_entry_points_argument_rules(hades_lib):
    enc, dec = hades_lib.hades252_cipher_encrypt, hades_lib.hades252_cipher_decrypt
    d = _dom()
    rej = ctypes.c_size_t(7)
    assert enc(None, None, None, 0, 2, d, None) == 0
    assert dec(None, None, None, 0, 2, d, None, None, ctypes.byref(rej)) == 0 and rej.value == 0
    for args in ((None, A, A), (A, None, A), (A, A, None)):
        assert enc(*args, 3, 2, d, A) == INVALID
        assert dec(*args, 3, 2, d, A, A, None) == INVALID
    assert enc(A, A, A, 3, 2, None, A) == INVALID and enc(A, A, A, 3, 2, d, None) == INVALID
    assert enc(A, A, A, 3, 0, d, A) == INVALID and enc(A, A, A, 3, 1025, d, A) == INVALID
    assert dec(A, A, A, 3, 2, d, A, None, None) == INVALID and dec(A, A, A, 3, 1025, d, A, A, None) == INVALID
    too_many = (2**64 - 1) // (3 * 32) + 1                    # n x (M + 1) x 32 bytes would not fit size_t
    assert enc(A, A, A, too_many, 2, d, A) == INVALID and dec(A, A, A, too_many, 2, d, A, A, None) == INVALID


def test_python_layer_checks_shapes():
    import numpy as np
    from hades252_amd import strategy as H
    assert H.CIPHER_DOMAIN == (1 << 32) * (1 << 256) % 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    text = open(os.path.join(ROOT, "include", "hades252.h")).read()
    limbs = re.search(r"#define HADES252_CIPHER_DOMAIN_MONT \{([^}]*)\}", text).group(1).split(",")
    assert sum(int(v.strip().rstrip("ul"), 16) << (64 * k) for k, v in enumerate(limbs)) == H.CIPHER_DOMAIN
    z = np.zeros((3, 4), dtype=np.uint64)
    with pytest.raises(ValueError):                              # 3 messages of 2 scalars need 6
        H.cipher_encrypt_host(z, np.zeros((6, 4), dtype=np.uint64), z, 2)
    with pytest.raises(ValueError):                              # two key scalars per message
        H.cipher_encrypt_host(np.zeros((6, 4), dtype=np.uint64), z, z, 2)
    with pytest.raises(ValueError):
        H.cipher_decrypt_host(np.zeros((6, 4), dtype=np.uint64), np.zeros((6, 4), dtype=np.uint64), z, 2)
    with pytest.raises(ValueError):
        H.cipher_encrypt_host(z, np.zeros((6, 4), dtype=np.uint64), z, 0)
    with pytest.raises(TypeError):
        H.cipher_encrypt_host(z.astype(np.int64), np.zeros((6, 4), dtype=np.uint64), z, 1)


def test_python_layer_refuses_tensors_on_different_devices():
    import torch
    from hades252_amd import strategy as H
    H._same_device("cipher_encrypt", torch.device("cuda", 0), torch.device("cuda", 0))
    with pytest.raises(ValueError, match="every tensor must be on"):
        H._same_device("cipher_encrypt", torch.device("cuda", 0), torch.device("cuda", 0), torch.device("cuda", 1))


def test_cpp_wrappers_compile_and_link(hades_lib, tmp_path):
    src = tmp_path / "cipher.cpp"
    src.write_text(r'''
#include "hades252.hpp"
#include <cstdio>
#include <vector>
int main() {
    using dusk_hades::BlsScalar;
    const std::size_t n = 3, m = 2;
    std::vector<BlsScalar> msgs(n * m), keys(n * 2), nonces(n), ciphers(n * (m + 1)), back(n * m);
    std::vector<std::uint8_t> ok(n);
    const BlsScalar domain = dusk_hades::CIPHER_DOMAIN;
    try {
        dusk_hades::cipher_encrypt(msgs.data(), keys.data(), nonces.data(), n, m, domain, ciphers.data());
        std::size_t rejected = dusk_hades::cipher_decrypt(ciphers.data(), keys.data(), nonces.data(), n, m, domain,
                                                          back.data(), ok.data());
        std::printf("%zu\n", rejected);
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "cipher"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", CSRC,
                    "-lhades252", "-Wl,-rpath," + CSRC, "-o", str(exe)], check=True)
    assert exe.exists()


LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")


@pytest.fixture(scope="module")
def cipher_resources(hades_lib, tmp_path_factory):
    """The resource metadata of the cipher kernels, read from the gfx950 code object INSIDE the built library (no second
    compile: the code object of libhades252.so is unbundled and its AMDGPU metadata note read)."""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not available")
    objcopy, bundler, readelf = tools
    from hades252_amd import _lib
    tmp_path = tmp_path_factory.mktemp("codeobj")
    fat, co = tmp_path / "fatbin", tmp_path / "gfx950.co"
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=%s" % fat, _lib.LIB_PATH, str(tmp_path / "scratch.so")],
                   check=True)
    subprocess.run([bundler, "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--output=%s" % co], check=True)
    notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    res = {}
    for entry in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:          # one entry of amdhsa.kernels per kernel
        m = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if m is None or "k_cipher" not in m.group(1):
            continue
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)$", entry, re.M)
                           if k in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                    "private_segment_fixed_size")}
    return res


def test_cipher_kernels_have_no_scratch_and_fit_their_bounds(cipher_resources):
    lane = [k for k in cipher_resources if "k_cipherI" in k]
    wave = [k for k in cipher_resources if "k_cipher_lanes" in k]
    assert len(lane) == 2 and len(wave) == 4, sorted(cipher_resources)
    for name, r in cipher_resources.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
    for name in lane:         # __launch_bounds__(256, 3): 3 waves per SIMD -> at most 168 VGPRs (+ AGPRs: one file)
        r = cipher_resources[name]
        assert r["vgpr_count"] + r["agpr_count"] <= 168, (name, r)
    for name in wave:         # __launch_bounds__(256): 1 wave per SIMD admits 512, the lanes arithmetic needs <= 128
        r = cipher_resources[name]
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, r)


def test_counter_record_of_the_secondary_kernels_stays_keyed():
    """The cipher's sources stay out of build.device_source_hash (they define and launch none of the kernels of the
    committed `secondary_kernels` counter record), so adding them leaves that record valid for bench.py."""
    import json
    from hades252_amd import build
    assert {"kernels_cipher.hpp", "abi_cipher.hpp"} <= set(build.DEPS)
    assert not {"kernels_cipher.hpp", "abi_cipher.hpp"} & set(build.DEVICE_DEPS + build.LAUNCH_POLICY_DEPS)
    with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as f:
        sec = json.load(f)["secondary_kernels"]
    assert sec["device_source_hash"] == build.device_source_hash()
