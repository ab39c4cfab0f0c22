"""CPU tier: the per-operation kernels (k_states_literal<OP_ARK>, k_states_fast, k_sbox), the bulk field operations
(k_fr_op, both implementations, with `out` aliasing either input), the wire format (k_wire, in place too) and the
generators / digest, from the unchanged sources in the host build under ASan+UBSan, byte for byte against the oracle.
Buffers are heap blocks of exactly their size."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import oracle_lib  # noqa: E402
import round_inverse as RI  # noqa: E402
from oracle_lib import P, R, limbs_of, int_of, digest_ref  # noqa: E402
from gpu_common import EDGE_VALUES, edge_scalars, catalogue_states, word_boundary_values  # noqa: E402

FR_ADD, FR_MUL, FR_SQUARE, FR_FROM_RAW, FR_REDUCE_SIGNED = range(5)
RINV = pow(R, -1, P)


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def u64(b):
    return np.frombuffer(b, dtype=np.uint64)


def words(vals):
    return np.array([l for v in vals for l in limbs_of(v)], dtype=np.uint64)


def _partial_sbox(oracle, ark):
    st = ark.reshape(-1, 5, 4).copy()
    st[:, 4, :] = oracle.quintic_s_box(st[:, 4, :].copy()).reshape(-1, 4)
    return st.reshape(-1)


def test_per_op_kernels_on_catalogue_rounds(oracle):
    """As tests/test_gpu_a02_perop.py: for the catalogue entries of each round r, from the oracle's trace[r - 1]:
    add_round_key (round and cursor forms), the S-box on the keyed words, mul_matrix on the "mds_in" states,
    apply_full_round and apply_partial_round (round and cursor forms)."""
    states, labels = catalogue_states()
    by_round = {}
    for i, lab in enumerate(labels):
        by_round.setdefault(lab.r, []).append(i)
    s = HS.Script()
    want = {}
    for r, idx in sorted(by_round.items()):
        prev = np.array([states[i] if r == 0 else oracle.perm_trace(states[i])[1][r - 1].reshape(-1) for i in idx],
                        dtype=np.uint64).reshape(-1)
        n = len(idx)
        ark = oracle.add_round_key(prev, r)
        sboxed = oracle.quintic_s_box(ark)
        mds_in = sboxed if RI.is_full(r) else _partial_sbox(oracle, ark)
        cases = [("ark", prev, "hades252_add_round_key_dev", (n, r), ark),
                 ("arkc", prev, "hades252_add_round_key_at_dev", (n, 5 * r), ark),
                 ("sbox", ark, "hades252_quintic_s_box_dev", (5 * n,), sboxed),
                 ("mds", mds_in, "hades252_mul_matrix_dev", (n,), oracle.mul_matrix(mds_in)),
                 ("full", prev, "hades252_apply_full_round_dev", (n, r), oracle.full_round(prev, r)),
                 ("fullc", prev, "hades252_apply_full_round_at_dev", (n, 5 * r), oracle.full_round(prev, r)),
                 ("part", prev, "hades252_apply_partial_round_dev", (n, r), oracle.partial_round(prev, r)),
                 ("partc", prev, "hades252_apply_partial_round_at_dev", (n, 5 * r), oracle.partial_round(prev, r))]
        for tag, inp, fn, args, exp in cases:
            name = "%s%d" % (tag, r)
            s.buf(name, inp.tobytes())
            s.call(fn, name, *args, None)
            s.dump(name)
            want[name] = exp
    r = s.run(timeout=900)                               # measured: 8 s (the catalogue's 12 rounds x 8 launches of one ragged block)
    assert all(rc == 0 for _, rc in r.rc) and len(r.rc) == len(want)
    for name, exp in want.items():
        assert (u64(r.out[name]) == exp).all(), name


def test_per_op_cursor_limits():
    s = HS.Script()
    s.zero("st", 160)
    s.call("hades252_add_round_key_at_dev", "st", 1, 955, None)
    s.call("hades252_add_round_key_at_dev", "st", 1, 956, None)
    s.call("hades252_add_round_key_at_dev", "st", 1, -1, None)
    r = s.run(timeout=60)                                # measured: 0.3 s
    assert [rc for _, rc in r.rc] == [0, -6, -1]         # ok, HADES252_ERR_OUT_OF_CONSTANTS, HADES252_ERR_INVALID_ARG


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("alias", ["none", "a", "b"])
def test_fr_op_both_implementations_and_aliases(impl, alias):
    """out[i] = a[i] op b[i]; the header promises that out may alias a or b."""
    rng = random.Random(11 + impl)
    n = 300                                              # two blocks, ragged last wave
    av = [EDGE_VALUES[i % len(EDGE_VALUES)] if i % 3 else rng.randrange(P) for i in range(n)]
    bv = [EDGE_VALUES[(i * 5 + 1) % len(EDGE_VALUES)] if i % 2 else rng.randrange(P) for i in range(n)]
    truth = {FR_ADD: [(x + y) % P for x, y in zip(av, bv)], FR_MUL: [x * y * RINV % P for x, y in zip(av, bv)],
             FR_SQUARE: [x * x * RINV % P for x in av], FR_FROM_RAW: [x * R % P for x in av]}
    s = HS.Script()
    for op in truth:
        s.buf("a%d" % op, words(av).tobytes())
        s.buf("b%d" % op, words(bv).tobytes())
        s.fill("o%d" % op, 32 * n, 0xFF)
        out = {"none": "o%d", "a": "a%d", "b": "b%d"}[alias] % op
        s.call("hades252_fr_op_dev", op, impl, "a%d" % op, "b%d" % op, out, n, None)
        for b in ("a%d" % op, "b%d" % op, "o%d" % op):
            s.dump(b)
    r = s.run(timeout=120)                               # measured: 0.8 s
    assert [rc for _, rc in r.rc] == [0] * 4
    for op, exp in truth.items():
        out = {"none": "o%d", "a": "a%d", "b": "b%d"}[alias] % op
        assert (u64(r.out[out]) == words(exp)).all(), (op, alias)
        if alias != "a":
            assert (u64(r.out["a%d" % op]) == words(av)).all()
        if alias != "b":
            assert (u64(r.out["b%d" % op]) == words(bv)).all()


def test_fr_op_reduce_signed_window():
    """op 4 (impl 1 only): the exit routine of the scaled trace on the edges of its window (-p - 2^250, 2^250]."""
    rng = random.Random(13)
    xs = [0, 1, -1, 1 << 250, (1 << 250) - 1, -P, -P + 1, -P - 1, -P - (1 << 250) + 1, -(1 << 250), P >> 1, -(P >> 1)]
    xs += [rng.randrange(-P - (1 << 250) + 1, (1 << 250) + 1) for _ in range(300 - len(xs))]
    s = HS.Script()
    s.buf("a", words([x % (1 << 256) for x in xs]).tobytes())
    s.fill("o", 32 * len(xs), 0xFF)
    s.call("hades252_fr_op_dev", FR_REDUCE_SIGNED, 1, "a", None, "o", len(xs), None)
    s.call("hades252_fr_op_dev", FR_REDUCE_SIGNED, 0, "a", None, "o", len(xs), None)
    s.dump("o")
    r = s.run(timeout=60)                                # measured: 0.4 s
    assert [rc for _, rc in r.rc] == [0, -1]
    assert (u64(r.out["o"]) == words([x % P for x in xs])).all()


def test_wire_format_ragged_in_place_and_bad_count(oracle):
    rng = random.Random(3)
    vals = [0, 1, P - 1, R] + [rng.randrange(P) for _ in range(596)]
    raw = b"".join(v.to_bytes(32, "little") for v in vals)
    bnd = word_boundary_values()
    mixed = [bnd[i // 2] if i % 2 == 0 else (vals[i], True) for i in range(2 * len(bnd))] + [(v, True) for v in vals[:300]]
    mraw = b"".join(v.to_bytes(32, "little") for v, _ in mixed)
    n_bad = sum(1 for _, ok in mixed if not ok)
    s = HS.Script()
    s.buf("mix", mraw)
    s.fill("mix_out", len(mraw), 0xFF)
    s.zero("bad", 4)
    s.call("hades252_from_bytes_dev", "mix", "mix_out", len(mixed), "bad", None)
    s.zero("bad2", 4)
    s.call("hades252_from_bytes_dev", "mix", "mix", len(mixed), "bad2", None)          # in place
    for b in ("mix", "mix_out", "bad", "bad2"):
        s.dump(b)
    sizes = (1, 2, 255, 256, 257, 511, 513, 600)
    for n in sizes:
        s.buf("raw%d" % n, raw[:32 * n])
        s.fill("limbs%d" % n, 32 * n, 0xFF)
        s.fill("back%d" % n, 32 * n, 0xFF)
        s.call("hades252_from_bytes_dev", "raw%d" % n, "limbs%d" % n, n, None, None)
        s.call("hades252_to_bytes_dev", "limbs%d" % n, "back%d" % n, n, None)
        s.dump("limbs%d" % n)
        s.dump("back%d" % n)
        s.call("hades252_to_bytes_dev", "limbs%d" % n, "limbs%d" % n, n, None)         # in place; dumped again below
    r = s.run(timeout=120)                               # measured: 1.2 s
    assert all(rc == 0 for _, rc in r.rc)
    assert int(np.frombuffer(r.out["bad"], dtype=np.int32)[0]) == n_bad
    assert int(np.frombuffer(r.out["bad2"], dtype=np.int32)[0]) == n_bad
    got = u64(r.out["mix_out"]).reshape(-1, 4)
    for (v, ok), row in zip(mixed, got):
        assert int_of(row) == (v * R % P if ok else 0), (hex(v), ok)
    assert r.out["mix"] == r.out["mix_out"]
    for n in sizes:
        assert [int_of(x) for x in u64(r.out["limbs%d" % n]).reshape(-1, 4)] == [v * R % P for v in vals[:n]], n
        assert r.out["back%d" % n] == raw[:32 * n], n
    rc, one = oracle.from_bytes(list((P - 1).to_bytes(32, "little")))
    assert rc == 0 and int_of(one) == (P - 1) * R % P


def test_to_bytes_in_place():
    rng = random.Random(4)
    vals = [rng.randrange(P) for _ in range(300)]
    s = HS.Script()
    s.buf("x", words([v * R % P for v in vals]).tobytes())
    s.call("hades252_to_bytes_dev", "x", "x", len(vals), None)
    s.dump("x")
    r = s.run(timeout=60)                                # measured: 0.4 s
    assert r.rc == [("hades252_to_bytes_dev", 0)]
    assert r.out["x"] == b"".join(v.to_bytes(32, "little") for v in vals)


def test_generators_and_digest(oracle):
    n = 1000                                             # scalars: ragged for both generators
    s = HS.Script("sponge")
    s.fill("a", 32 * n, 0xFF)
    s.fill("b", 32 * n, 0xFF)
    s.call("hades252_gen_a_dev", "a", 7, n, None)
    s.call("hades252_gen_b_dev", "b", 7, n, oracle_lib.GEN_SEED, None)
    s.zero("d", 32)
    s.call("hades252_digest_dev", "b", 5, 4 * n - 3, "d", None)       # a word count that is no multiple of 4 or 256
    for b in "abd":
        s.dump(b)
    r = s.run(timeout=60)                                # measured: 0.5 s
    assert [rc for _, rc in r.rc] == [0, 0, 0]
    assert (u64(r.out["a"]) == oracle.gen_a(7, n)).all()
    assert (u64(r.out["b"]) == oracle.gen_b(7, n)).all()
    assert list(map(int, u64(r.out["d"]))) == digest_ref(oracle.gen_b(7, n)[:4 * n - 3], 5)
