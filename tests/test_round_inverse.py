"""CPU tier: tests/round_inverse.py (Hades252 run backwards) and its edge catalogue -- inputs that put edge values INSIDE
the rounds -- against the spec (hades_spec.perm's trace, perm_gadget's wires), the C oracle's trace, and every limb-exact
model of tests/test_fast_model.py with all of their bound and window assertions.

Which catalogue entries reach which exit or reduction routine (shown by the models below; the GPU tier runs the same
entries through the kernels: test_gpu_a01_perm.py, test_gpu_a02_perop.py, test_gpu_f4_witness.py):
  * finalize (hades_fast.hpp), the exit of the fast, coop, lanes and rows kernels: round 66 "out" = 0 in any word (kinds
    "edge" and "zero") and "sbox_in" = 0 in every word of round 66 hand it x >= 0, so BOTH conditional subtractions run;
    lanes and rows also on the in-memory output 1.  Every output 0 sends exactly p through one fr_cond_sub_p (fr32.hpp).
  * finalize_window (kernels_perm.hpp, the scaled trace's exit): its rare x >= 0 side is taken where the held value is
    exactly 0: the all-zero output and round 0's all-zero S-box input, and the held zeros r5/out/w1, r33/out/w1, w3.
  * the held zero of the scale-tracked schedule ("held_zero" at "out": the held word is 0 mod p, the scaled trace stores 0;
    at "mds_in": words 0..3 enter the linear layer as 0 mod p).
  * finalize32 (kernels_perm.hpp, every witness wire and the true-form trace): every zero wire -- "zero" at "out" (the
    trace word), "sbox_edge" = 0 (the key wire and v2, v4, v5), "r1_zero" (an r1 row) -- sends exactly p through its
    fr_cond_sub_p."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hades_spec as S  # noqa: E402
import round_inverse as RI  # noqa: E402
import test_fast_model as F  # noqa: E402
from hades252_amd import _derive as D  # noqa: E402
from oracle_lib import limbs_of, int_of  # noqa: E402

P = S.P
LB, NL, MASK = F.LB, F.NL, F.MASK


def mont(vals):
    return [S.to_mont(v) for v in vals]


def signed_limbs(v):
    """the normalised limbs (0..7 in [0, 2^29), signed top limb) of a value the linear layer leaves"""
    return [(v >> (LB * k)) & MASK for k in range(NL - 1)] + [v >> (LB * (NL - 1))]


def catalogue_subset():
    """The entries the slower lane models run (a fixed subset keeps the CPU tier inside its time): every round-66 entry
    and the held zeros of a first, a middle and the last partial round."""
    return [(inp, lab) for inp, lab in RI.edge_catalogue()
            if lab.r == RI.ROUNDS - 1 or (lab.kind == "held_zero" and lab.r in (5, 33, 62))]


def zero_entries():
    """The entries with a zero among their targets (every "zero" and "r1_zero", the zero S-box inputs and outputs): the
    ones that reach finalize32's exact-p subtraction in the witness model."""
    return [(inp, lab) for inp, lab in RI.edge_catalogue() if 0 in lab.values or lab.kind == "r1_zero"]


def test_inverse_maps():
    m, minv = S.mds_matrix(), RI.mds_inverse()
    for i in range(5):
        for j in range(5):
            assert sum(minv[i][k] * m[k][j] for k in range(5)) % P == int(i == j)
    assert 5 * RI.SBOX_INV % (P - 1) == 1
    rng = random.Random(3)
    for v in [0, 1, 2, P - 1, RI.M1, RI.MP1] + [rng.randrange(P) for _ in range(20)]:
        assert pow(S.quintic_s_box(v), RI.SBOX_INV, P) == v and S.quintic_s_box(pow(v, RI.SBOX_INV, P)) == v


def test_unround_inverts_every_round():
    rng = random.Random(5)
    for r in range(RI.ROUNDS):
        for _ in range(3):
            x = [rng.randrange(P) for _ in range(5)]
            assert RI.unround(RI.round_fwd(x, r), r) == x, r
            assert RI.round_fwd(RI.unround(x, r), r) == x, r
    x = [rng.randrange(P) for _ in range(5)]
    tr = []
    S.perm(x, tr)
    assert [s["out"] for s in RI.stages_of(x)] == tr


def test_input_for_every_stage():
    rng = random.Random(7)
    for r in (0, 2, 4, 30, 62, 63, 66):
        for stage in RI.STAGES:
            tgt = [rng.randrange(P) for _ in range(5)]
            assert RI.stages_of(RI.input_for(r, stage, tgt))[r][stage] == tgt, (r, stage)
    assert S.perm(RI.input_for(66, "out", [0] * 5)) == [0] * 5


def test_catalogue_holds_what_it_promises():
    cat = RI.edge_catalogue()
    assert cat == RI.edge_catalogue() and len(cat) == len({lab for _, lab in cat})
    keys = {tuple(lab[:4]) for _, lab in cat}
    trace_d, pre_d = RI.held_offsets()
    for v in RI.OUTPUT_EDGES:
        assert (66, "out", tuple(range(5)), (v,) * 5) in keys
    for w in range(5):
        assert (66, "out", (w,), (0,)) in keys
    r1 = {}
    for _, lab in cat:
        if lab.kind == "r1_zero":
            r1.setdefault(lab.r, set()).update(RI.r1_rows(lab))
    for r in RI.CATALOGUE_ROUNDS:
        for v in RI.SBOX_EDGES:
            assert (r, "sbox_in", (4,), (v,)) in keys
            assert not RI.is_full(r) or (r, "sbox_in", tuple(range(5)), (v,) * 5) in keys
        for w in range(5):
            assert (r, "out", (w,), (0,)) in keys and (r, "out", (w,), (trace_d[r][w],)) in keys
        for w in range(4):
            assert (r, "mds_in", (w,), (pre_d[r][w],)) in keys
        assert {0, 4} <= r1[r], r
    # the held zeros differ from the true zeros exactly where constants are deferred: in and after the partial rounds
    assert all(any(trace_d[r]) == any(pre_d[r]) == (not RI.is_full(r)) for r in RI.CATALOGUE_ROUNDS)


def test_every_entry_reaches_its_label_in_the_spec(oracle):
    """For every entry: the labelled words hold the labelled values at the labelled round and stage -- read from the spec's
    trace and from perm_gadget's wires (the key wires / r2 rows for "sbox_in", the S-box outputs for "mds_in"), which must
    agree with the forward restatement stages_of; a zero r1 wire for "r1_zero"; and the C oracle's trace is the spec's."""
    lay = RI.gadget_layout()
    trace_d, pre_d = RI.held_offsets()
    for inp, lab in RI.edge_catalogue():
        assert len(inp) == 5 and all(0 <= v < P for v in inp)
        tr, wires = [], []
        out = S.perm(inp, tr)
        assert S.perm_gadget(inp, wires) == out and len(wires) == 972
        st = RI.stages_of(inp)
        for r in range(RI.ROUNDS) if lab.r == 66 else (lab.r,):
            sbox_in = [wires[i] for i in lay[r]["sbox_in"]]
            mds_in = list(sbox_in)
            for w, (_, _, v5) in lay[r]["sbox"].items():
                mds_in[w] = wires[v5]
            assert st[r] == {"sbox_in": sbox_in, "mds_in": mds_in, "out": tr[r]}, (str(lab), r)
        got = st[lab.r][lab.stage]
        assert [got[w] for w in lab.words] == list(lab.values), str(lab)
        if lab.kind == "held_zero":
            offs = trace_d[lab.r] if lab.stage == "out" else pre_d[lab.r]
            assert all(v == offs[w] and v for w, v in zip(lab.words, lab.values)), str(lab)
        if lab.kind == "r1_zero":
            rows = RI.r1_rows(lab)
            assert rows and all(wires[lay[lab.r]["r1"][j]] == 0 for j in rows), str(lab)
        if lab.stage == "sbox_in" and lab.values[0] == 0:              # the S-box wires of a zero input are zero
            assert all(wires[g] == 0 for w in lab.words for g in lay[lab.r]["sbox"][w]), str(lab)
        _, otr = oracle.perm_trace(np.array([l for v in mont(inp) for l in limbs_of(v)], dtype=np.uint64))
        assert [[int_of(otr[r][w]) for w in range(5)] for r in range(RI.ROUNDS)] == [mont(row) for row in tr], str(lab)


def test_fast_model_and_scaled_trace_on_the_catalogue():
    """fast_perm_model (k_perm_fast, k_perm_rows' schedule) on every entry, with the state it holds after every round; that
    state through finalize_window_model (the scaled trace's exit) and the host's tables back to the spec's trace, every
    round and word; the held zeros held as 0 mod p; and which entries take the rare sides named in the module docstring."""
    sch = D.fast_schedule()
    mul, add = D.trace_scaled_tables()
    r_inv = pow(S.R, -1, P)
    trace_d, _ = RI.held_offsets()
    exit_both, window_pos = set(), set()
    for inp, lab in RI.edge_catalogue():
        held, tr = [], []
        assert F.fast_perm_model(mont(inp), held) == mont(S.perm(inp, tr)), str(lab)
        for r in range(RI.ROUNDS):
            for w in range(5):
                scaled, rare = F.finalize_window_model(signed_limbs(held[r][w]))
                assert (scaled * mul[r] % P * r_inv + add[r][w]) % P == S.to_mont(tr[r][w]), (str(lab), r, w)
                if rare and held[r][w] >= 0:
                    window_pos.add(str(lab))
        if lab.stage == "out":
            for w, v in zip(lab.words, lab.values):
                if v == trace_d[lab.r][w]:
                    assert held[lab.r][w] % P == 0, str(lab)
        for w in range(5):                                              # finalize(mont_lin(., FINAL_F)): x + 2p >= 2p?
            if F.val(F.mont_lin(signed_limbs(held[66][w]), sch["final_f"])) >= 0:
                exit_both.add(str(lab))
    zero_out = {str(lab) for _, lab in RI.edge_catalogue() if lab.r == 66 and lab.stage == "out" and 0 in lab.values}
    assert zero_out and zero_out <= exit_both, sorted(zero_out - exit_both)
    assert {"r66/out/w01234=0,0,0,0,0/edge", "r0/sbox_in/w01234=0,0,0,0,0/sbox_edge"} <= window_pos
    assert any(s.endswith("/held_zero") for s in window_pos), sorted(window_pos)


@pytest.mark.parametrize("model", ["coop", "lanes", "rows"])
def test_latency_models_on_the_catalogue(model, monkeypatch):
    """coop_perm_model, lanes_perm_model, rows_perm_model (k_perm_coop, k_perm_lanes, k_perm_rows) on the round-66 entries
    and the held zeros: spec-equal outputs with every bound asserted; the output zeros reach finalize with x >= 0."""
    fn = {"coop": F.coop_perm_model, "lanes": F.lanes_perm_model, "rows": F.rows_perm_model}[model]
    seen = []
    real = F.finalize_model

    def recording(x, factor):
        seen.append(F.val(F.mont_fips(x, D.to_limbs29(factor))))
        return real(x, factor)

    monkeypatch.setattr(F, "finalize_model", recording)
    for inp, lab in catalogue_subset():
        seen.clear()
        assert fn(mont(inp)) == mont(S.perm(inp)), str(lab)
        if lab.r == 66 and lab.stage == "out" and lab.values == (0,) * 5:
            assert len(seen) == 5 and all(x >= 0 for x in seen), (model, str(lab))


def test_witness_model_on_the_catalogue():
    """witness_model (k_perm_witness, and k_perm_trace_fast with `trace`) on the entries with a zero target: all 972
    wires against perm_gadget, every round of the trace against the spec, finalize32's window asserted on every wire."""
    for inp, lab in zero_entries():
        spec, tr, spec_tr = [], [], []
        S.perm_gadget(inp, spec)
        S.perm(inp, spec_tr)
        assert F.witness_model(mont(inp), tr) == mont(spec), str(lab)
        assert tr == [mont(row) for row in spec_tr], str(lab)


def test_per_op_models_on_the_catalogue():
    """The per-operation kernels (k_states_fast, k_sbox) on the state each entry's round hands them: the S-box on the
    "sbox_in" words, the matrix on "mds_in", the full / partial round body after the key."""
    op = D.per_op_constants()
    for inp, lab in RI.edge_catalogue():
        st = RI.stages_of(inp)[lab.r]
        a, b = st["sbox_in"], st["mds_in"]
        x = [D.to_limbs29(v) for v in mont(a)]
        assert [F.finalize_model(F.sbox(w), op["k"]) for w in x] == mont(S.quintic_s_box(v) for v in a), str(lab)
        assert [F.finalize_model(y, op["w"]) for y in F.small_mds([D.to_limbs29(v) for v in mont(b)])] == \
            mont(RI._matvec(S.mds_matrix(), b)), str(lab)
        if RI.is_full(lab.r):
            body = F.small_mds([F.sbox(w) for w in x])
            assert [F.finalize_model(y, op["w_full"]) for y in body] == mont(st["out"]), str(lab)
        else:
            body = F.small_mds(x[:4] + [F.mont_fips(F.sbox(x[4]), D.to_limbs29(op["k"]))])
            assert [F.finalize_model(y, op["w"]) for y in body] == mont(st["out"]), str(lab)
