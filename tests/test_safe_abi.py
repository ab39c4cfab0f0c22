"""CPU tier: the boundary of the batched duplex sponge (hades252_safe_*) without a GPU -- the symbols are declared, bound and
exported; hades252_safe_pattern agrees with the model on valid patterns and refuses every class of invalid one; every
argument rule of the device and host entry points answers before the device is touched and leaves the cursor alone; the
Python SafeSponge refuses departures from its pattern; the C++ wrappers compile and link; the code object of k_safe /
k_safe_lanes in the built library has no scratch and fits its launch bounds; and the new sources leave the key of the
committed secondary-kernel counter record alone."""
import ctypes
import random

import pytest

import abi_common
import codeobj
import safe_model as M
from abi_common import INVALID, MIS, PTR, limbs4
from safe_model import A, Q

SYMS = ["hades252_safe_pattern", "hades252_safe_hash_dev", "hades252_safe_absorb_dev", "hades252_safe_squeeze_dev",
        "hades252_safe_hash"]

INVALID_PATTERNS = {
    "empty": [],
    "squeeze first": [Q(1), A(1), Q(1)],
    "absorb last": [A(1), Q(1), A(1)],
    "only an absorb": [A(3)],
    "zero-length absorb": [A(0), Q(1)],
    "zero-length squeeze": [A(1), Q(0)],
    "zero-length call in the middle": [A(1), Q(1), A(0), Q(1)],
    "65 calls": [A(1)] * 64 + [Q(1)],
    "2^20 + 1 words in": [A((1 << 20) + 1), Q(1)],
    "2^20 + 1 words in, split": [A(1 << 20), A(1), Q(1)],
    "2^20 + 1 words out": [A(1), Q((1 << 20) + 1)],
    "2^20 + 1 words out, split": [A(1), Q(1 << 19), A(1), Q((1 << 19) + 1)],
}


def _calls(pattern):
    words = M.encode(pattern)
    return (ctypes.c_uint32 * max(len(words), 1))(*words), len(words)


def test_symbols_are_declared_bound_and_exported(hades_lib):
    from hades252_amd import _lib
    abi_common.assert_declared_bound_exported(SYMS)
    header = abi_common.header()
    for line, value in (("#define HADES252_SAFE_MAX_CALLS 64", _lib.SAFE_MAX_CALLS),
                        ("#define HADES252_SAFE_MAX_WORDS 1048576", _lib.SAFE_MAX_WORDS),
                        ("#define HADES252_SAFE_ABSORB 2147483648u", _lib.SAFE_ABSORB)):
        assert line in header and int(line.split()[-1].rstrip("u")) == value
    assert (_lib.SAFE_MAX_CALLS, _lib.SAFE_MAX_WORDS, _lib.SAFE_ABSORB) == (M.MAX_CALLS, M.MAX_WORDS, M.ABSORB_BIT)


def test_header_says_convention_unpinned():
    abi_common.header_block("batched duplex sponge", "#define HADES252_SAFE_MAX_CALLS",
                            ("CONVENTION UNPINNED", "recalled from dusk-safe", "tests/safe_model.py",
                             "1 025 .. 16 384"))                # says which sizes have no form of their own


def test_pattern_against_the_model(hades_lib):
    fn = hades_lib.hades252_safe_pattern
    rng = random.Random(8)
    pats = [[A(L), Q(1)] for L in range(1, 14)] + [[A(1), Q(64)], [A(1 << 20), Q(1 << 20)], [A(1)] * 63 + [Q(1)],
                                                   M.cipher_pattern(2), M.cipher_pattern(7)]
    for _ in range(300):
        pat = [A(rng.randrange(1, 40))]
        for _ in range(rng.randrange(0, 20)):
            pat.append((rng.choice(["absorb", "squeeze"]), rng.randrange(1, 40)))
        pats.append(pat + [Q(rng.randrange(1, 40))])
    for pat in pats:
        assert M.valid(pat)
        arr, k = _calls(pat)
        n_in, n_out, n_perms = ctypes.c_size_t(7), ctypes.c_size_t(7), ctypes.c_size_t(7)
        assert fn(arr, k, ctypes.byref(n_in), ctypes.byref(n_out), ctypes.byref(n_perms)) == 0, pat
        assert (n_in.value, n_out.value, n_perms.value) == (M.words_in(pat), M.words_out(pat), M.perms_closed_form(pat)), pat
        assert fn(arr, k, None, None, None) == 0               # each result is optional


@pytest.mark.parametrize("what", sorted(INVALID_PATTERNS))
def test_every_class_of_invalid_pattern_is_refused_everywhere(hades_lib, what):
    pat = INVALID_PATTERNS[what]
    assert not M.valid(pat)
    arr, k = _calls(pat)
    n_in = ctypes.c_size_t(7)
    assert hades_lib.hades252_safe_pattern(arr, k, ctypes.byref(n_in), None, None) == INVALID and n_in.value == 7
    assert hades_lib.hades252_safe_hash_dev(PTR, 5, arr, k, limbs4(), PTR, None) == INVALID
    assert hades_lib.hades252_safe_hash(PTR, 5, arr, k, limbs4(), PTR) == INVALID
    from hades252_amd import strategy as H
    with pytest.raises(ValueError):
        H.safe_pattern(pat)
    with pytest.raises(ValueError):
        H.safe_tag_input(pat, 0)


def test_one_shot_argument_rules(hades_lib):
    arr, k = _calls([A(3), Q(2)])
    dev, host = hades_lib.hades252_safe_hash_dev, hades_lib.hades252_safe_hash

    def d(inp=PTR, n=5, calls=arr, n_calls=k, tag=limbs4(), out=PTR):
        return dev(inp, n, calls, n_calls, tag, out, None)

    assert d(inp=None, n=0, calls=None, n_calls=0, tag=None, out=None) == 0      # n = 0: a no-op success, whatever else
    assert host(None, 0, None, 0, None, None) == 0
    for kw in ({"inp": None}, {"out": None}, {"tag": None}, {"calls": None}, {"n_calls": 0}, {"n_calls": 65}, {"inp": MIS},
               {"out": MIS}, {"n": (1 << 30) + 1}):
        assert d(**kw) == INVALID, kw
    assert hades_lib.hades252_safe_pattern(None, 2, None, None, None) == INVALID
    for args in ((None, 3, arr, k, limbs4(), PTR), (PTR, 3, None, k, limbs4(), PTR), (PTR, 3, arr, k, None, PTR),
                 (PTR, 3, arr, k, limbs4(), None), (PTR, 3, arr, 0, limbs4(), PTR)):
        assert host(*args) == INVALID
    too_many = (2**64 - 1) // (5 * 32) + 1                       # n x (n_in + n_out) x 32 bytes would not fit size_t
    assert host(PTR, too_many, arr, k, limbs4(), PTR) == INVALID


def test_streaming_argument_rules_leave_the_cursor_alone(hades_lib):
    absorb, squeeze = hades_lib.hades252_safe_absorb_dev, hades_lib.hades252_safe_squeeze_dev
    for start in (0, 2 | (4 << 4), 1 << 4):                       # fresh, after an absorb, after a squeeze
        cur = ctypes.c_uint32(start)
        c = ctypes.byref(cur)
        assert absorb(None, 0, None, 0, None, None) == 0 and squeeze(None, 0, 0, None, None, None) == 0
        assert absorb(PTR, 0, PTR, 3, c, None) == 0 and cur.value == start         # a no-op: the cursor stays
        for args in ((None, 4, PTR, 3, c), (PTR, 4, None, 3, c), (MIS, 4, PTR, 3, c), (PTR, 4, MIS, 3, c), (PTR, 4, PTR, 0, c),
                     (PTR, 4, PTR, (1 << 20) + 1, c), (PTR, (1 << 30) + 1, PTR, 3, c), (PTR, 4, PTR, 3, None)):
            assert absorb(*args, None) == INVALID, args
            assert cur.value == start
        for args in ((None, 4, 3, PTR, c), (PTR, 4, 3, None, c), (MIS, 4, 3, PTR, c), (PTR, 4, 3, MIS, c), (PTR, 4, 0, PTR, c),
                     (PTR, 4, (1 << 20) + 1, PTR, c), (PTR, (1 << 30) + 1, 3, PTR, c), (PTR, 4, 3, PTR, None)):
            assert squeeze(*args, None) == INVALID, args
            assert cur.value == start
    for bad in (5, 5 << 4, 1 | (2 << 4), 1 << 8, 0xFFFFFFFF):    # not a pair of positions a sponge can be in
        cur = ctypes.c_uint32(bad)
        assert absorb(PTR, 4, PTR, 3, ctypes.byref(cur), None) == INVALID and cur.value == bad
        assert squeeze(PTR, 4, 3, PTR, ctypes.byref(cur), None) == INVALID and cur.value == bad


class _NoDevice:
    """SafeSponge with the device taken out: the pattern bookkeeping alone (what a violation is never reaches a device)."""

    def __new__(cls, pattern):
        from hades252_amd import strategy as H
        sp = object.__new__(H.SafeSponge)
        H.safe_pattern(pattern)
        sp._todo = [list(c) for c in M.aggregate(pattern)]
        return sp


def test_safe_sponge_refuses_departures_from_its_pattern():
    from hades252_amd import strategy as H
    sp = _NoDevice([A(2), A(1), Q(2), A(2), Q(1)])
    with pytest.raises(ValueError, match="expects absorb"):
        sp._take("squeeze", 1)                                  # wrong kind
    with pytest.raises(ValueError, match="has 3 left"):
        sp._take("absorb", 4)                                   # too long
    with pytest.raises(ValueError, match="at least one word"):
        sp._take("absorb", 0)
    with pytest.raises(ValueError, match="still expects absorb"):
        sp.finish()                                             # early
    for kind, k in (("absorb", 1), ("absorb", 2), ("squeeze", 2), ("absorb", 2)):   # split calls are served
        sp._take(kind, k)
        sp._took(k)
    with pytest.raises(ValueError, match="still expects squeeze"):
        sp.finish()
    with pytest.raises(ValueError, match="expects squeeze"):
        sp._take("absorb", 1)
    sp._take("squeeze", 1)
    sp._took(1)
    sp.finish()
    with pytest.raises(ValueError, match="used up"):
        sp._take("squeeze", 1)
    with pytest.raises(ValueError):
        H.SafeSponge(3, [Q(1)], 1, device="cpu")                # an invalid pattern: refused before any allocation
    with pytest.raises(ValueError):
        H._safe_calls([("soak", 1)], "test")
    assert H.safe_tag_input([A(2), A(1), Q(1)], 7) == M.tag_input([A(2), A(1), Q(1)], 7) == \
        bytes.fromhex("80000003" "00000001" "0000000000000007")


def test_python_layer_checks_shapes():
    import numpy as np
    from hades252_amd import strategy as H
    with pytest.raises(ValueError):                              # 7 scalars are not sponges of 3
        H.safe_hash_host(np.zeros((7, 4), dtype=np.uint64), [A(3), Q(1)], 1)
    with pytest.raises(TypeError):
        H.safe_hash_host(np.zeros((6, 4), dtype=np.int64), [A(3), Q(1)], 1)
    assert H.safe_pattern([A(3), Q(2), A(2), Q(1)]) == (5, 3, 2)


def test_cpp_wrappers_compile_and_link(hades_lib, tmp_path):
    abi_common.compile_and_run(tmp_path, "safe", r'''
#include "hades252.hpp"
#include <cstdio>
#include <vector>
int main() {
    using dusk_hades::BlsScalar;
    const std::uint32_t calls[] = {dusk_hades::safe_absorb(3), dusk_hades::safe_squeeze(2)};
    try {
        const dusk_hades::SafePattern p = dusk_hades::safe_pattern(calls, 2);
        std::printf("%zu %zu %zu\n", p.n_in, p.n_out, p.n_perms);
        if (p.n_in != 3 || p.n_out != 2 || p.n_perms != 1) return 1;
        const std::size_t n = 3;
        std::vector<BlsScalar> in(n * p.n_in), out(n * p.n_out);
        const BlsScalar tag{};
        std::uint32_t cursor = 0;
        if (false) {
            dusk_hades::safe_hash_dev(nullptr, n, calls, 2, tag, nullptr);
            dusk_hades::safe_absorb_dev(nullptr, n, nullptr, 3, cursor);
            dusk_hades::safe_squeeze_dev(nullptr, n, 2, nullptr, cursor);
        }
        dusk_hades::safe_hash(in.data(), n, calls, 2, tag, out.data());
    } catch (const dusk_hades::HadesPanic &e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
''', run=False)       # it would touch a device: link only


def test_safe_kernels_have_no_scratch_and_fit_their_bounds(hades_lib):
    co = codeobj.load()
    lane, wave = co.kernels("k_safe"), co.kernels("k_safe_lanes")
    assert len(lane) == 1 and len(wave) == 2, sorted(co.meta)
    for name in lane + wave:
        r = co.meta[name]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] >= 256                # the aggregated calls travel by value in the arguments
    for name in lane:         # __launch_bounds__(256, 3): 3 waves per SIMD -> at most 168 VGPRs (+ AGPRs: one file)
        r = co.meta[name]
        assert r["vgpr_count"] + r["agpr_count"] <= 168, (name, r)
    for name in wave:         # __launch_bounds__(256): 1 wave per SIMD admits 512, the lanes arithmetic needs <= 128
        r = co.meta[name]
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, r)


def test_counter_record_of_the_secondary_kernels_stays_keyed():
    """The duplex sponge's sources stay out of build.device_source_hash (they define and launch none of the kernels of the
    committed `secondary_kernels` counter record), so adding them leaves that record valid for bench.py."""
    abi_common.assert_outside_counter_records(["kernels_safe.hpp", "abi_safe.hpp"],
                                              also_in_deps=["host_safe.hpp", "kernels_cipher.hpp"])
