"""CPU tier: the boundary of the cipher witnesses (hades252_cipher_{encrypt,decrypt}_witness_dev) without a GPU -- the symbols
are declared, bound and exported; hades252_cipher_perms matches the model; every argument rule answers before the device is
touched; the C++ wrappers compile and link; the new code leaves the keys of the committed counter records alone; and the
code object of k_witness_cipher in the built library, both directions, has k_perm_witness's budget."""
import pytest

import abi_common
import cipher_witness_model as CW
import codeobj
from abi_common import INVALID, MIS, PTR, limbs4

SYMS = ["hades252_cipher_perms", "hades252_cipher_encrypt_witness_dev", "hades252_cipher_decrypt_witness_dev"]


def test_symbols_are_declared_bound_and_exported(hades_lib):
    abi_common.assert_declared_bound_exported(SYMS)


def test_header_states_the_contract():
    abi_common.header_block("gadget witnesses of the cipher", "size_t hades252_cipher_perms",
                            ("CONVENTION UNPINNED", "rec = s * n", "hades252_perm_witness_dev(inputs) byte for byte",
                             "REDUCED mod p", "2^30", "may be NULL"))
    text = abi_common.header()
    start = text.index("gadget witnesses of the cipher")
    # after the cipher section (whose first phrase and whose decrypt prototypes come first)
    assert text.index("int hades252_cipher_decrypt(") < start


def test_cipher_perms_matches_the_model(hades_lib):
    for m in list(range(0, 40)) + [CW.MAX_LEN - 1, CW.MAX_LEN, CW.MAX_LEN + 1, 1 << 40, 2 ** 64 - 1]:
        assert hades_lib.hades252_cipher_perms(m) == CW.cipher_perms(m), m
    assert hades_lib.hades252_cipher_perms(0) == 0 and hades_lib.hades252_cipher_perms(CW.MAX_LEN + 1) == 0


def test_encrypt_witness_argument_rules(hades_lib):
    f = hades_lib.hades252_cipher_encrypt_witness_dev
    dom = limbs4()

    def call(msgs=PTR, keys=PTR, nonces=PTR, n=5, m=3, d=dom, inp=PTR, wires=PTR, out=None):
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
    dom = limbs4()

    def call(ciphers=PTR, keys=PTR, nonces=PTR, n=5, m=3, d=dom, inp=PTR, wires=PTR, out=None, ok=None, rej=None):
        return f(ciphers, keys, nonces, n, m, d, inp, wires, out, ok, rej, None)

    assert call(ciphers=None, keys=None, nonces=None, n=0, m=0, d=None, inp=None, wires=None, rej=PTR + 1) == 0
    for kw in ({"ciphers": None}, {"keys": None}, {"nonces": None}, {"d": None}, {"m": 0}, {"m": CW.MAX_LEN + 1},
               {"ciphers": MIS}, {"keys": MIS}, {"nonces": MIS}, {"out": MIS}, {"rej": PTR + 2}, {"inp": None},
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
    out = abi_common.compile_and_run(tmp_path, "cipher_witness", r'''
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
    assert out[0] == "2 0" and len(out) == 3, out


def test_counter_records_stay_keyed():
    """The cipher witness lives in kernels_witness.hpp / abi_witness.hpp, outside build.device_source_hash and
    perm_fast_hash, so bench.py keeps replaying its counter-backed traffic."""
    abi_common.assert_outside_counter_records(["kernels_witness.hpp", "abi_witness.hpp"])


def test_cipher_witness_kernel_has_the_perm_witness_budget(hades_lib):
    co = codeobj.load()
    chain = co.kernels("k_witness_cipher")
    assert len(chain) == 2, sorted(co.meta)                      # encrypt and decrypt
    codeobj.assert_perm_witness_budget(co, chain)
