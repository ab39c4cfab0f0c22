"""CPU tier: the boundary of the duplex sponge witnesses (hades252_safe_witness_dev, hades252_safe_{absorb,squeeze}_witness_dev)
without a GPU -- the symbols are declared, bound and exported; the header states the contract; every argument rule answers
before the device is touched and leaves *cursor and *step alone; the Python layer checks types; the C++ wrappers compile and
link; the new code leaves the keys of the committed counter records alone; and the code object of k_witness_duplex in the
built library has k_perm_witness's budget."""
import ctypes

import pytest

import abi_common
import codeobj
import safe_model as M
from abi_common import INVALID, MIS, PTR, limbs4
from safe_model import A, Q

SYMS = ["hades252_safe_witness_dev", "hades252_safe_absorb_witness_dev", "hades252_safe_squeeze_witness_dev"]


def _calls(pattern):
    words = M.encode(pattern)
    return (ctypes.c_uint32 * max(len(words), 1))(*words), len(words)


def test_symbols_are_declared_bound_and_exported(hades_lib):
    abi_common.assert_declared_bound_exported(SYMS)


def test_header_states_the_contract():
    abi_common.header_block("gadget witnesses of the duplex sponge", "int hades252_safe_witness_dev",
                            ("CONVENTION UNPINNED", "rec = s * n", "hades252_perm_witness_dev(inputs) byte for byte", "2^30",
                             "may be NULL", "*step + q <= total_steps", "on success only", "read, not changed",
                             "no one-per-wave latency form"))
    text = abi_common.header()
    start = text.index("gadget witnesses of the duplex sponge")
    # after the cipher-witness section, which follows the plain duplex sponge
    assert text.index("batched duplex sponge") < text.index("gadget witnesses of the cipher") < start
    assert text.index("int hades252_cipher_decrypt_witness_dev(") < start


def test_one_shot_argument_rules(hades_lib):
    f = hades_lib.hades252_safe_witness_dev
    arr, k = _calls([A(3), Q(2), A(2), Q(1)])                      # S = 2
    tag = limbs4()

    def call(d_in=PTR, n=5, calls=arr, n_calls=k, t=tag, inp=PTR, wires=PTR, out=None):
        return f(d_in, n, calls, n_calls, t, inp, wires, out, None)

    assert call(d_in=None, n=0, calls=None, n_calls=0, t=None, inp=None, wires=None) == 0          # n = 0: a no-op
    assert call(n=0, out=MIS) == 0
    for kw in ({"d_in": None}, {"t": None}, {"calls": None}, {"n_calls": 0}, {"n_calls": 65}, {"d_in": MIS}, {"out": MIS},
               {"inp": None}, {"wires": None}, {"inp": MIS}, {"wires": MIS}, {"n": (1 << 30) + 1},
               {"n": (1 << 29) + 1}):                                # 2 permutations x (2^29 + 1) > 2^30 records
        assert call(**kw) == INVALID, kw
    for bad in ([Q(1)], [A(1)], [A(1), Q(1), A(1)], [A(0), Q(1)], [A(1), Q(0)], [A((1 << 20) + 1), Q(1)]):
        barr, bk = _calls(bad)
        assert call(calls=barr, n_calls=bk) == INVALID, bad
    s16, k16 = _calls([A(1), Q(64)])                                # S = 16: 2^26 sponges are 2^30 records, one more is not
    assert call(calls=s16, n_calls=k16, n=(1 << 26) + 1) == INVALID


@pytest.mark.parametrize("kind", ["absorb", "squeeze"])
def test_streaming_argument_rules_leave_cursor_and_step_alone(hades_lib, kind):
    absorb = kind == "absorb"
    f = hades_lib.hades252_safe_absorb_witness_dev if absorb else hades_lib.hades252_safe_squeeze_witness_dev

    def call(states=PTR, n=4, words=PTR, length=3, cur=None, inp=PTR, wires=PTR, total=8, step=None):
        if absorb:
            return f(states, n, words, length, cur, inp, wires, total, step, None)
        return f(states, n, length, words, cur, inp, wires, total, step, None)

    for start in (0, 2 | (4 << 4), 1 << 4, 4 | (4 << 4)):          # fresh, after absorbs (a full block last), after a squeeze
        for step0 in (0, 3):
            cur, step = ctypes.c_uint32(start), ctypes.c_size_t(step0)
            c, s = ctypes.byref(cur), ctypes.byref(step)
            assert call(n=0, cur=c, step=s) == 0                    # a no-op: the cursor and the step stay
            assert call(states=None, n=0, words=None, cur=None, inp=None, wires=None, step=None) == 0
            for kw in ({"states": None}, {"words": None}, {"states": MIS}, {"words": MIS}, {"length": 0},
                       {"length": (1 << 20) + 1}, {"n": (1 << 30) + 1}, {"cur": None}, {"inp": None}, {"wires": None},
                       {"inp": MIS}, {"wires": MIS}, {"step": None},
                       {"n": 1 << 28, "total": 5},                   # 5 x 2^28 > 2^30 records
                       {"total": step0 - 1 if step0 else 0, "length": 9},   # *step (+ q) past total_steps
                       {"total": step0 + 1, "length": 9}):           # 9 words run at least 2 permutations: one step of room
                kw = dict({"cur": c, "step": s}, **kw)
                assert call(**kw) == INVALID, (kind, start, step0, kw)
                assert cur.value == start and step.value == step0, kw
    for bad in (5, 1 | (2 << 4), 5 << 4, 1 << 8):                   # not a cursor this library hands out
        cur, step = ctypes.c_uint32(bad), ctypes.c_size_t(0)
        assert call(cur=ctypes.byref(cur), step=ctypes.byref(step)) == INVALID, bad
        assert cur.value == bad and step.value == 0


def test_python_layer_checks_types_and_patterns():
    import numpy as np
    from hades252_amd import strategy as H
    assert issubclass(H.SafeWitnessSponge, H.SafeSponge)
    for name in ("absorb", "squeeze", "finish", "wires", "inputs"):
        assert hasattr(H.SafeWitnessSponge, name), name
    with pytest.raises(TypeError):                               # host memory is not a device batch
        H.safe_witness(np.zeros((2, 5, 4), dtype=np.uint64), [A(3), Q(2), A(2), Q(1)], 1)
    with pytest.raises(ValueError):
        H.safe_witness(np.zeros((2, 5, 4), dtype=np.uint64), [Q(1)], 1)


def test_cpp_wrappers_compile_and_link(hades_lib, tmp_path):
    out = abi_common.compile_and_run(tmp_path, "safe_witness", r'''
#include "hades252.hpp"
#include <cstdio>
int main() {
    const std::uint32_t calls[2] = {dusk_hades::safe_absorb(3), dusk_hades::safe_squeeze(2)};
    std::printf("%zu\n", dusk_hades::safe_pattern(calls, 2).n_perms);
    dusk_hades::BlsScalar tag{};
    std::uint32_t cursor = 0;
    std::size_t step = 0;
    try {
        dusk_hades::safe_witness(nullptr, 3, calls, 2, tag, nullptr, nullptr);
    } catch (const dusk_hades::HadesPanic &e) {                  // refused before the device
        std::printf("%s\n", e.what());
    }
    try {
        dusk_hades::safe_absorb_witness_dev(nullptr, 3, nullptr, 3, cursor, nullptr, nullptr, 1, step);
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("%s\n", e.what());
    }
    try {
        dusk_hades::safe_squeeze_witness_dev(nullptr, 3, 2, nullptr, cursor, nullptr, nullptr, 1, step);
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("%s\n", e.what());
    }
    std::printf("%u %zu\n", cursor, step);
    return 0;
}
''')
    assert out[0] == "1" and out[-1] == "0 0" and len(out) == 5, out


def test_counter_records_stay_keyed():
    """The duplex sponge witness lives in kernels_witness.hpp / abi_witness.hpp, outside build.device_source_hash and
    perm_fast_hash, so bench.py keeps replaying its counter-backed traffic."""
    abi_common.assert_outside_counter_records(["kernels_witness.hpp", "abi_witness.hpp"])


def test_duplex_witness_kernel_has_the_perm_witness_budget(hades_lib):
    co = codeobj.load()
    (name,) = co.kernels("k_witness_duplex")                     # one kernel: one-shot and streaming
    print(name, co.meta[name], "v_mad", codeobj.mads(co.body(name)))
    codeobj.assert_perm_witness_budget(co, [name])
