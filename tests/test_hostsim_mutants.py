"""CPU tier: proof that the detectors of the host simulation tier are live.  Each case builds the host executable from
the temporary copy with ONE line of a shipped source changed (tests/hostsim_lib.py MUTANTS), runs a script that passes on
the unchanged build, and asserts that the detector named for the mutant reports it.  Nothing here touches a GPU or the
tree's sources."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import test_fast_model as M  # noqa: E402
from oracle_lib import limbs_of  # noqa: E402
from gpu_common import edge_scalars  # noqa: E402

FAST = 2


def perm_script(variant, mutant, n=300, launcher=False):
    s = HS.Script("perm", variant, mutant)
    s.buf("st", edge_scalars(5 * n, 700).tobytes())
    if launcher:
        s.call("launch_perm_fast", "st", "st", n, None)
    else:
        s.call("hades252_perm_batch_dev_ex", "st", n, None, FAST)
    s.dump("st")
    return s


def both(make, timeout):
    """(result on the unchanged build -- must pass --, result on the mutant)"""
    good = make(None).run(timeout=timeout)
    assert good.returncode == 0
    return good, make(True).run(timeout=timeout, check=False)


def test_store_one_chunk_past_the_end_is_an_asan_report():
    _, bad = both(lambda m: perm_script("asan", m and "store_off_by_one"), 120)        # measured: 0.5 s
    assert bad.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in bad.stderr
    assert "WRITE of size 16" in bad.stderr and "0 bytes after 48000-byte region" in bad.stderr.replace("to the right of", "after")


def test_halved_dynamic_lds_is_an_asan_report():
    _, bad = both(lambda m: perm_script("asan", m and "lds_halved", launcher=True), 120)
    assert bad.returncode != 0 and "AddressSanitizer: use-after-poison" in bad.stderr


def test_removed_barrier_is_a_tsan_report():
    _, bad = both(lambda m: perm_script("tsan", m and "load_barrier_removed"), 300)      # measured: 1 s
    assert bad.returncode != 0 and "ThreadSanitizer: data race" in bad.stderr
    assert "wave_load_scalars" in bad.stderr


def test_wrong_limb_of_minus_p_is_an_oracle_mismatch():
    with open(os.path.join(ROOT, "tests", "golden", "kat.json")) as f:
        kat = json.load(f)["single"]
    inp = np.array([l for s in kat for x in s["in_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)
    exp = np.array([l for s in kat for x in s["out_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)

    def make(m):
        s = HS.Script("perm", "asan", m and "negp_index")
        s.buf("st", inp.tobytes())
        s.call("hades252_perm_batch_dev_ex", "st", len(kat), None, FAST)
        s.dump("st")
        return s
    good, bad = both(make, 120)
    assert (np.frombuffer(good.out["st"], dtype=np.uint64) == exp).all()
    assert bad.returncode == 0, bad.stderr[-2000:]          # no sanitizer sees it: only the known answers do
    got = np.frombuffer(bad.out["st"], dtype=np.uint64).reshape(-1, 20)
    assert (got != exp.reshape(-1, 20)).any(axis=1).all()   # every known answer is missed


def test_doubled_cross_products_are_a_ubsan_report():
    """mont_fips<SQR> on the maximal-limb operands of tests/test_fast_model.py: the column bound 9 * 2.25 * 2^58 + 8 * 2^58
    < 2^63 holds on the shipped code and breaks when the doubled cross products are counted twice."""
    ops = np.array([l for x in M.PRODUCT_PATTERNS for l in x], dtype=np.int32)

    def make(m):
        s = HS.Script("perm", "asan", m and "double_doubled")
        s.buf("a", ops.tobytes())
        s.fill("o", ops.nbytes, 0xFF)
        s.call("units_mont_sqr", "a", "o", len(M.PRODUCT_PATTERNS), None)
        s.dump("o")
        return s
    good, bad = both(make, 120)
    got = np.frombuffer(good.out["o"], dtype=np.int32).reshape(-1, M.NL)
    assert [list(map(int, r)) for r in got] == [M.mont_fips(x, x, True) for x in M.PRODUCT_PATTERNS]
    assert bad.returncode != 0 and "runtime error: signed integer overflow" in bad.stderr
    assert "hades_fast.hpp" in bad.stderr


# ---- the DPP forms of hades_lanes.hpp (emulated DPP row moves and permlane swaps) ---------------------------------------
LANES = 4


def lanes_script(variant, mutant, n, seed=701):
    s = HS.Script("perm", variant, mutant)
    s.buf("st", edge_scalars(5 * n, seed).tobytes())
    s.call("hades252_perm_batch_dev_ex", "st", n, None, LANES)
    s.dump("st")
    return s


def test_single_exchange_buffer_of_the_helper_protocol_is_a_tsan_report():
    """The one cross-wave protocol argued in prose only (LanesLds::xw, "whatever the timing"): with both sides on ONE
    buffer a main wave's store of round r + 1 is no longer a barrier away from the helper's reads of round r.  TSan's
    happens-before analysis reports it whatever the schedule of this run was."""
    _, bad = both(lambda m: lanes_script("tsan", m and "xw_single_buffer", 4), 600)    # measured: 9 s, the mutant 0.6 s
    assert bad.returncode != 0 and "ThreadSanitizer: data race" in bad.stderr
    assert "lanes_perm" in bad.stderr and "hades_lanes.hpp" in bad.stderr


def test_wrong_carry_shift_in_a_dpp_routine_is_an_oracle_mismatch():
    with open(os.path.join(ROOT, "tests", "golden", "kat.json")) as f:
        kat = json.load(f)["single"]
    inp = np.array([l for s in kat for x in s["in_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)
    exp = np.array([l for s in kat for x in s["out_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)

    def make(m):
        s = HS.Script("perm", "asan", m and "carry_light_shift")
        s.buf("st", inp.tobytes())
        s.call("hades252_perm_batch_dev_ex", "st", len(kat), None, LANES)
        s.dump("st")
        return s
    good, bad = both(make, 900)                              # measured: 25 s each (11 known answers: four helped blocks)
    assert (np.frombuffer(good.out["st"], dtype=np.uint64) == exp).all()
    assert bad.returncode == 0, bad.stderr[-2000:]          # every value stays inside its word: only the known answers see it
    got = np.frombuffer(bad.out["st"], dtype=np.uint64).reshape(-1, 20)
    assert (got != exp.reshape(-1, 20)).any(axis=1).all()   # every known answer is missed


def test_lane_addressing_the_next_word_is_an_asan_report():
    _, bad = both(lambda m: lanes_script("asan", m and "lanes_word_off_by_one", 1), 300)      # measured: 2 s
    assert bad.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in bad.stderr
    # (the word is read four bytes at a time: whichever of its eight reads is reported lies 0 .. 28 bytes behind the state)
    assert re.search(r"READ of size 4 .*\n(.*\n)*.* is located (0|4|8|12|16|20|24|28) bytes (after|to the right of) 160-byte region",
                     bad.stderr)
