"""CPU tier: the boundary of the batched Poseidon cipher (hades252_cipher_*) without a GPU -- the symbols are declared,
bound and exported; every argument rule answers before the device is touched; the C++ wrappers compile and link; the code
object of k_cipher / k_cipher_lanes in the built library has no scratch and fits its launch bounds; and the cipher's sources
leave the key of the committed secondary-kernel counter record alone."""
import ctypes
import re

import pytest

import abi_common
import codeobj
from abi_common import INVALID, MIS, PTR, limbs4

SYMS = ["hades252_cipher_encrypt_dev", "hades252_cipher_decrypt_dev", "hades252_cipher_encrypt", "hades252_cipher_decrypt"]


def test_symbols_are_declared_bound_and_exported(hades_lib):
    from hades252_amd import _lib
    abi_common.assert_declared_bound_exported(SYMS)
    assert "#define HADES252_CIPHER_MAX_LEN 1024" in abi_common.header()
    assert _lib.CIPHER_MAX_LEN == 1024


def test_header_says_convention_unpinned():
    abi_common.header_block("batched Poseidon cipher", "#define HADES252_CIPHER_MAX_LEN",
                            ("CONVENTION UNPINNED", "hades252_from_bytes_dev"))


def test_device_entry_points_argument_rules(hades_lib):
    enc, dec = hades_lib.hades252_cipher_encrypt_dev, hades_lib.hades252_cipher_decrypt_dev
    d = limbs4()

    def e(msgs=PTR, keys=PTR, nonces=PTR, n=5, m=2, dom=d, out=PTR):
        return enc(msgs, keys, nonces, n, m, dom, out, None)

    def x(c=PTR, keys=PTR, nonces=PTR, n=5, m=2, dom=d, out=PTR, ok=PTR, rej=None):
        return dec(c, keys, nonces, n, m, dom, out, ok, rej, None)

    # n = 0: a no-op success, whatever else is passed
    assert e(msgs=None, keys=None, nonces=None, n=0, m=0, dom=None, out=None) == 0
    assert x(c=None, keys=None, nonces=None, n=0, m=0, dom=None, out=None, ok=None) == 0
    for kw in ({"msgs": None}, {"keys": None}, {"nonces": None}, {"out": None}, {"dom": None}, {"m": 0}, {"m": 1025},
               {"msgs": MIS}, {"keys": MIS}, {"nonces": MIS}, {"out": MIS}, {"n": (1 << 30) + 1}):
        assert e(**kw) == INVALID, kw
    for kw in ({"c": None}, {"keys": None}, {"nonces": None}, {"out": None}, {"ok": None}, {"dom": None}, {"m": 0},
               {"m": 1025}, {"c": MIS}, {"keys": MIS}, {"nonces": MIS}, {"out": MIS}, {"rej": PTR + 2},
               {"n": (1 << 30) + 1}):
        assert x(**kw) == INVALID, kw


def test_host_entry_points_argument_rules(hades_lib):
    enc, dec = hades_lib.hades252_cipher_encrypt, hades_lib.hades252_cipher_decrypt
    d = limbs4()
    rej = ctypes.c_size_t(7)
    assert enc(None, None, None, 0, 2, d, None) == 0
    assert dec(None, None, None, 0, 2, d, None, None, ctypes.byref(rej)) == 0 and rej.value == 0
    for args in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
        assert enc(*args, 3, 2, d, PTR) == INVALID
        assert dec(*args, 3, 2, d, PTR, PTR, None) == INVALID
    assert enc(PTR, PTR, PTR, 3, 2, None, PTR) == INVALID and enc(PTR, PTR, PTR, 3, 2, d, None) == INVALID
    assert enc(PTR, PTR, PTR, 3, 0, d, PTR) == INVALID and enc(PTR, PTR, PTR, 3, 1025, d, PTR) == INVALID
    assert dec(PTR, PTR, PTR, 3, 2, d, PTR, None, None) == INVALID and dec(PTR, PTR, PTR, 3, 1025, d, PTR, PTR, None) == INVALID
    too_many = (2**64 - 1) // (3 * 32) + 1                    # n x (M + 1) x 32 bytes would not fit size_t
    assert enc(PTR, PTR, PTR, too_many, 2, d, PTR) == INVALID and dec(PTR, PTR, PTR, too_many, 2, d, PTR, PTR, None) == INVALID


def test_python_layer_checks_shapes():
    import numpy as np
    from hades252_amd import strategy as H
    assert H.CIPHER_DOMAIN == (1 << 32) * (1 << 256) % 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    limbs = re.search(r"#define HADES252_CIPHER_DOMAIN_MONT \{([^}]*)\}", abi_common.header()).group(1).split(",")
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
    abi_common.compile_and_run(tmp_path, "cipher", r'''
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
''', run=False)       # it would touch a device: link only


def test_cipher_kernels_have_no_scratch_and_fit_their_bounds(hades_lib):
    co = codeobj.load()
    lane, wave = co.kernels("k_cipher"), co.kernels("k_cipher_lanes")
    assert len(lane) == 2 and len(wave) == 4, sorted(co.meta)
    for name in lane + wave:
        r = co.meta[name]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
    for name in lane:         # __launch_bounds__(256, 3): 3 waves per SIMD -> at most 168 VGPRs (+ AGPRs: one file)
        r = co.meta[name]
        assert r["vgpr_count"] + r["agpr_count"] <= 168, (name, r)
    for name in wave:         # __launch_bounds__(256): 1 wave per SIMD admits 512, the lanes arithmetic needs <= 128
        r = co.meta[name]
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, r)


def test_counter_record_of_the_secondary_kernels_stays_keyed():
    """The cipher's sources stay out of build.device_source_hash (they define and launch none of the kernels of the
    committed `secondary_kernels` counter record), so adding them leaves that record valid for bench.py."""
    abi_common.assert_outside_counter_records(["kernels_cipher.hpp", "abi_cipher.hpp"])
