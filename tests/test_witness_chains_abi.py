"""CPU tier: the boundary of the chain witnesses (hades252_sponge_witness_dev, hades252_merkle_open_witness_dev) without a
GPU -- the symbols are declared, bound and exported; every argument rule answers before the device is touched; the C++
wrappers compile and link; hades252_sponge_blocks matches the model; the new sources leave the keys of the committed
counter records alone; and the code object of the sponge witness kernel in the built library has k_perm_witness's budget."""
import pytest

import abi_common
import codeobj
import witness_chain_model as W
from abi_common import INVALID, MIS, PTR, limbs4

SYMS = ["hades252_sponge_blocks", "hades252_sponge_witness_dev", "hades252_merkle_open_witness_dev"]


def test_symbols_are_declared_bound_and_exported(hades_lib):
    abi_common.assert_declared_bound_exported(SYMS)


def test_header_states_the_contract():
    abi_common.header_block("gadget witnesses of permutation chains", "size_t hades252_sponge_blocks",
                            ("rec = s * n + i", "CONVENTION UNPINNED", "hades252_perm_witness_dev(inputs) byte for byte",
                             "selection and add gates", "2^30"))
    text = abi_common.header()
    assert text.index("int hades252_perm_witness_dev") < text.index("size_t hades252_sponge_blocks")


@pytest.mark.parametrize("pad_mode", [0, 1])
def test_sponge_blocks_matches_the_model(hades_lib, pad_mode):
    for m in list(range(0, 40)) + [1 << 20, (1 << 32) + 3]:
        assert hades_lib.hades252_sponge_blocks(m, pad_mode) == W.sponge_blocks(m, pad_mode), m
    assert hades_lib.hades252_sponge_blocks(2 ** 64 - 1, pad_mode) == (2 ** 64 - 1 + pad_mode + 3) // 4
    assert hades_lib.hades252_sponge_blocks(5, 2) == 0 and hades_lib.hades252_sponge_blocks(5, -1) == 0


def test_sponge_witness_argument_rules(hades_lib):
    f = hades_lib.hades252_sponge_witness_dev
    cap = limbs4()

    def call(msgs=PTR, n=5, m=3, c=cap, pad=1, inp=PTR, wires=PTR, dig=None):
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
    tag = limbs4()

    def call(leaves=PTR, tree=PTR, n=16, arity=4, t=tag, pad=None, idx=PTR, nq=3, inp=PTR, wires=PTR, bad=None):
        return f(leaves, tree, n, arity, t, pad, idx, nq, inp, wires, bad, None)

    assert call(leaves=None, tree=None, t=None, idx=None, nq=0, inp=None, wires=None) == 0
    for kw in ({"n": 1}, {"arity": 1}, {"arity": 5}, {"n": 1, "nq": 0},      # the tree's shape first
               {"leaves": None}, {"tree": None}, {"idx": None}, {"t": None}, {"inp": None}, {"wires": None},
               {"leaves": MIS}, {"tree": MIS}, {"pad": MIS}, {"inp": MIS}, {"wires": MIS}, {"bad": PTR + 2},
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
    out = abi_common.compile_and_run(tmp_path, "witness", r'''
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
    assert out[0] == "2" and len(out) == 3, out


def test_counter_records_stay_keyed():
    """The new sources stay out of build.device_source_hash and perm_fast_hash (they define no kernel of a committed counter
    record and leave every file that does byte for byte), so bench.py keeps replaying its counter-backed traffic."""
    abi_common.assert_outside_counter_records(["kernels_witness.hpp", "abi_witness.hpp"])


def test_sponge_witness_kernel_has_the_perm_witness_budget(hades_lib):
    co = codeobj.load()
    chain = co.kernels("k_witness_sponge")
    assert len(chain) == 2, sorted(co.meta)                      # pad_mode 0 and 1
    codeobj.assert_perm_witness_budget(co, chain)
    for name in co.kernels("k_witness_path_states"):
        assert co.meta[name]["private_segment_fixed_size"] == 0, (name, co.meta[name])
