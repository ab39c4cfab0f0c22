"""CPU tier: the shipped permutation kernels -- k_perm_fast, k_perm_coop, k_perm_lanes (helped and not), k_perm_rows,
k_states_literal, both traces, the scaled trace and the witness -- compiled for the host from the unchanged sources and run through the shipped launch policy under
ASan+UBSan (tests/hostsim_lib.py), byte for byte against the oracle.  Buffers are heap blocks of exactly their size, so a
read or write past byte n is a sanitizer report; the dynamic LDS behind a launch's request is poisoned.

Sizes stand on ~50 us per permutation per thread under the sanitizers (k_perm_fast; the literal kernel about 13 x that).
Every subprocess timeout is the measured time of its case on an 8-core box times 20 or more: a deadlocked emulation
fails the test, a slow machine does not."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hades_spec as S  # noqa: E402
import hostsim_lib as HS  # noqa: E402
import oracle_lib  # noqa: E402
from oracle_lib import limbs_of, int_of  # noqa: E402
from gpu_common import EDGE_VALUES, edge_scalars, catalogue_states, placed_batches, WIRES, FORM_SIZES  # noqa: E402

LITERAL, FAST, COOP = 1, 2, 3
SELECTORS = {"fast": FAST, "coop": COOP, "literal": LITERAL}
RAGGED = [1, 63, 64, 65, 255, 256, 257, 300]


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(ROOT, "tests", "golden", "kat.json")) as f:
        return json.load(f)


def u64(b):
    return np.frombuffer(b, dtype=np.uint64)


def states_of(n, seed):
    return edge_scalars(5 * n, seed)


@pytest.mark.parametrize("name", list(SELECTORS))
def test_kat_singles(kat, name):
    inp = np.array([l for s in kat["single"] for x in s["in_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)
    exp = np.array([l for s in kat["single"] for x in s["out_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)
    s = HS.Script()
    for i in range(len(kat["single"])):                  # one permutation per call (the reference's call shape) ...
        s.buf("one%d" % i, inp[20 * i:20 * i + 20].tobytes())
        s.call("hades252_perm_batch_dev_ex", "one%d" % i, 1, None, SELECTORS[name])
        s.dump("one%d" % i)
    s.buf("all", inp.tobytes())                          # ... and all of them as one batch
    s.call("hades252_perm_batch_dev_ex", "all", len(kat["single"]), None, SELECTORS[name])
    s.dump("all")
    r = s.run(timeout=120)                               # measured: 0.4 s (fast) .. 1.1 s (literal)
    assert all(rc == 0 for _, rc in r.rc)
    assert (u64(r.out["all"]) == exp).all()
    for i in range(len(kat["single"])):
        assert (u64(r.out["one%d" % i]) == exp[20 * i:20 * i + 20]).all()


@pytest.mark.parametrize("name", list(SELECTORS))
def test_ragged_in_place_edge_values(oracle, name):
    s = HS.Script()
    inp = {}
    for n in RAGGED:
        inp[n] = states_of(n, 1000 + n)
        s.buf("st%d" % n, inp[n].tobytes())
        s.call("hades252_perm_batch_dev_ex", "st%d" % n, n, None, SELECTORS[name])
        s.dump("st%d" % n)
    r = s.run(timeout=300)                               # measured: 0.6 s (fast), 1.5 s (coop), 3.9 s (literal)
    assert [rc for _, rc in r.rc] == [0] * len(RAGGED)
    for n in RAGGED:
        assert (u64(r.out["st%d" % n]) == oracle.perm_batch(inp[n])).all(), n


def test_fast_out_of_place_leaves_input(oracle):
    """k_perm_fast with out != in (the shape the host-pointer path launches), through the shipped launcher."""
    s = HS.Script()
    inp = {}
    for n in RAGGED:
        inp[n] = states_of(n, 2000 + n)
        s.buf("in%d" % n, inp[n].tobytes())
        s.fill("out%d" % n, 160 * n, 0xFF)
        s.call("launch_perm_fast", "in%d" % n, "out%d" % n, n, None)
        s.dump("in%d" % n)
        s.dump("out%d" % n)
    r = s.run(timeout=120)                               # measured: 0.6 s
    assert [rc for _, rc in r.rc] == [0] * len(RAGGED)
    for n in RAGGED:
        assert (u64(r.out["in%d" % n]) == inp[n]).all(), n
        assert (u64(r.out["out%d" % n]) == oracle.perm_batch(inp[n])).all(), n


def test_default_dispatch_past_coop_threshold(oracle):
    """16 400 states through hades252_perm_batch_dev: the size rule picks k_perm_fast, 65 blocks with a ragged last wave."""
    n = 16400
    inp = states_of(n, 3)
    s = HS.Script()
    s.call("hades252_kernel_for", n)
    s.buf("st", inp.tobytes())
    s.call("hades252_perm_batch_dev", "st", n, None)
    s.dump("st")
    r = s.run(timeout=300)                               # measured: 2.5 s
    assert r.rc == [("hades252_kernel_for", FAST), ("hades252_perm_batch_dev", 0)]
    assert (u64(r.out["st"]) == oracle.perm_batch(inp)).all()


# ---- the latency forms of hades_lanes.hpp: DPP row moves and permlane swaps emulated by the stand-in header ---------------
# One emulated block of four waves costs seconds (two wave barriers per DPP move, ~13 000 moves per permutation), so the
# sizes are the smallest that reach every role of a block.  form: tests/hostsim/hostsim_main.cpp, namespace forms.
LANES, ROWS = 4, 5
HELPED, UNHELPED, PER_ROW = 0, 1, 2


def test_default_dispatch_single_permutation_runs_the_helped_lanes_form(kat):
    """The reference's real call shape, ONE permutation, through the default dispatch: k_perm_lanes<true>, a lone state
    wave and its helper.  Known answers, one call each."""
    assert FORM_SIZES["lanes_helped"][0] == 1
    inp = np.array([l for s in kat["single"] for x in s["in_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)
    exp = np.array([l for s in kat["single"] for x in s["out_mont"] for l in limbs_of(int(x, 16))], dtype=np.uint64)
    n = 3                                                # (all eleven, as one batch: tests/test_hostsim_mutants.py's unchanged run)
    s = HS.Script()
    s.call("hades252_kernel_for", 1)
    for i in range(n):
        s.buf("one%d" % i, inp[20 * i:20 * i + 20].tobytes())
        s.call("hades252_perm_batch_dev", "one%d" % i, 1, None)
        s.dump("one%d" % i)
    r = s.run(timeout=600)                               # measured: 2.2 s per known answer
    assert r.rc == [("hades252_kernel_for", LANES)] + [("hades252_perm_batch_dev", 0)] * n
    assert "not_emulated" not in r.stdout
    for i in range(n):
        assert (u64(r.out["one%d" % i]) == exp[20 * i:20 * i + 20]).all(), i


@pytest.mark.parametrize("form,n", [(HELPED, 3), (HELPED, 4), (UNHELPED, 5), (PER_ROW, 4), (PER_ROW, 5)],
                         ids=["helped-full_block", "helped-ragged_block_idle_waves", "unhelped-full_and_ragged_block",
                              "rows-one_full_wave", "rows-ragged_second_wave"])
def test_lanes_and_rows_forms_in_place_edge_values(oracle, form, n):
    """k_perm_lanes<true> (three state waves and the helper; then a second block with one state wave, two idle waves and
    the helper), k_perm_lanes<false> (four state waves; then a block whose other waves return at once) and k_perm_rows (one
    state per 16-lane row: a full wave, then a wave with one row in use) on exact-size buffers of edge values.  The helped
    form and the rows form go through the shipped selector; the unhelped form belongs to 769 .. 1 024 states, which the
    emulation cannot afford, and is launched with its call site's geometry by form_perm."""
    assert n < FORM_SIZES["lanes"][0] < FORM_SIZES["rows"][0]
    inp = states_of(n, 4000 + 10 * form + n)
    s = HS.Script()
    s.buf("st", inp.tobytes())
    if form == UNHELPED:
        s.call("form_perm", "st", n, UNHELPED)
    else:
        s.call("hades252_perm_batch_dev_ex", "st", n, None, LANES if form == HELPED else ROWS)
    s.dump("st")
    r = s.run(timeout=600)                               # measured: 5.5 / 7.1 s (helped), 8.2 s (unhelped), 3.0 / 5.0 s (rows)
    assert [rc for _, rc in r.rc] == [0] and "not_emulated" not in r.stdout
    assert (u64(r.out["st"]) == oracle.perm_batch(inp)).all()


@pytest.mark.parametrize("name", list(SELECTORS))
def test_catalogue_placed_at_wave_and_block_boundaries(oracle, name):
    """The round-inverse catalogue (edge values INSIDE the rounds) at lanes 0, 63, 64, 255, 256 and the last of 300.  The
    five-waves kernel (64 states per block, 67 block barriers of 320 threads each: 0.1 s per block here) and the literal
    kernel (13 x the arithmetic) get the first two placed batches and then the whole catalogue as one dense batch, so that
    every entry still runs through them and the lanes 0, 63, 64, 255, 256 and the ragged last wave hold catalogue entries."""
    states, _ = catalogue_states()
    n = 300
    fill = states_of(n, 5).reshape(n, 20)
    s = HS.Script()
    batches = [b for b, lanes, idx in placed_batches(states, n, fill)]
    if name != "fast":
        batches = batches[:2] + [states]
    for i, b in enumerate(batches):
        s.buf("b%d" % i, b.tobytes())
        s.call("hades252_perm_batch_dev_ex", "b%d" % i, len(b), None, SELECTORS[name])
        s.dump("b%d" % i)
    r = s.run(timeout=900)                               # measured: 10 s (fast), 3 s (coop), 4 s (literal)
    assert all(rc == 0 for _, rc in r.rc) and len(r.rc) == len(batches)
    for i, b in enumerate(batches):
        assert (u64(r.out["b%d" % i]) == oracle.perm_batch(b.reshape(-1))).all(), i


# ---- traces and witness -----------------------------------------------------------------------------------------------
def oracle_trace(oracle, inp):
    """[67, n, 5, 4]"""
    st = inp.reshape(-1, 20)
    return np.stack([oracle.perm_trace(row)[1] for row in st], axis=1)


def trace_inputs(n):
    """The whole round-inverse catalogue (258 states: two blocks with a ragged last wave), or its first n rows."""
    states, _ = catalogue_states()
    return (states if n is None else states[:n]).reshape(-1).copy()


TRACE_SIZES = [1, 65, None]                               # None: the whole catalogue as one dense batch


@pytest.mark.parametrize("size", TRACE_SIZES, ids=["1", "65", "catalogue"])
def test_traces_true_literal_scaled(oracle, size):
    inp = trace_inputs(size)
    n = inp.size // 20
    s = HS.Script()
    s.buf("st", inp.tobytes())
    for name in ("fast", "literal", "scaled"):
        s.fill("tr_" + name, 67 * 160 * n, 0xFF)
    s.call("hades252_perm_trace_dev_ex", "st", "tr_fast", n, None, FAST)
    s.call("hades252_perm_trace_dev_ex", "st", "tr_literal", n, None, LITERAL)
    s.call("hades252_perm_trace_scaled_dev", "st", "tr_scaled", n, None)
    s.zero("mul", 67 * 32)
    s.zero("add", 67 * 5 * 32)
    s.call("hades252_perm_trace_scale_table", "mul", "add")
    for b in ("st", "tr_fast", "tr_literal", "tr_scaled", "mul", "add"):
        s.dump(b)
    r = s.run(timeout=600)                               # measured: 0.5 s (n = 1) .. 5 s (the catalogue)
    assert [rc for _, rc in r.rc] == [0, 0, 0, 0]
    assert (u64(r.out["st"]) == inp).all()
    exp = oracle_trace(oracle, inp)
    assert (u64(r.out["tr_fast"]).reshape(67, n, 5, 4) == exp).all()
    assert (u64(r.out["tr_literal"]).reshape(67, n, 5, 4) == exp).all()
    # scaled trace times the table equals the oracle trace: true = scaled * mul + add on in-memory (Montgomery) values,
    # every word of every round of every record
    scaled = u64(r.out["tr_scaled"]).reshape(67, n, 5, 4)
    mul, add = u64(r.out["mul"]).reshape(67, 4), u64(r.out["add"]).reshape(67, 5, 4)
    rinv = pow(oracle_lib.R, -1, oracle_lib.P)
    for rnd in range(67):
        m = int_of(mul[rnd])
        for w in range(5):
            a = int_of(add[rnd, w])
            for i in range(n):
                sc = int_of(scaled[rnd, i, w])
                assert sc < oracle_lib.P
                assert (sc * m * rinv + a) % oracle_lib.P == int_of(exp[rnd, i, w]), (rnd, i, w)


@pytest.mark.parametrize("size", TRACE_SIZES, ids=["1", "65", "catalogue"])
def test_witness_all_wires(oracle, size):
    """All 972 wires of EVERY record against the spec's GadgetStrategy, byte for byte (the unique in-memory form of the
    spec's value: canonical by construction)."""
    inp = trace_inputs(size)
    n = inp.size // 20
    s = HS.Script()
    s.buf("st", inp.tobytes())
    s.fill("wires", WIRES * 32 * n, 0xFF)
    s.call("hades252_witness_wires")
    s.call("hades252_perm_witness_dev", "st", "wires", n, None)
    s.dump("st")
    s.dump("wires")
    r = s.run(timeout=600)                               # measured: 0.5 s .. 3 s
    assert r.rc == [("hades252_witness_wires", WIRES), ("hades252_perm_witness_dev", 0)]
    assert (u64(r.out["st"]) == inp).all()
    wires = u64(r.out["wires"]).reshape(WIRES, n, 4)
    for i in range(n):
        st = [S.from_mont(int_of(inp.reshape(n, 5, 4)[i, w])) for w in range(5)]
        spec = []
        S.perm_gadget(st, spec)
        exp = np.array([limbs_of(S.to_mont(v)) for v in spec], dtype=np.uint64)
        bad = np.flatnonzero((wires[:, i, :] != exp).any(axis=1))
        assert bad.size == 0, (i, bad[:8])
    out = oracle.perm_batch(inp).reshape(n, 5, 4)           # r2 of the last round is the permutation
    for j in range(5):
        assert (wires[WIRES - 10 + 2 * j + 1] == out[:, j, :]).all()
