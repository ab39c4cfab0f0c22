"""CPU tier: the big-integer model of the inverse permutation (tests/perm_inverse_model.py) against oracle/hades_spec.py, its
golden file, and the generated constant tables of the kernels (hades252_amd/csrc/hades_inverse_constants.inc)."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_inverse_model as M  # noqa: E402
import round_inverse as RI  # noqa: E402
from hades252_amd import _derive as D  # noqa: E402

S, P = M.S, M.P
EDGES = (0, 1, 2, P - 1, P - 2, S.from_mont(1), S.from_mont(P - 1), S.R, (1 << 255) % P)


def test_exponent_inverts_the_s_box():
    assert 5 * M.D % (P - 1) == 1 and 0 < M.D < P - 1
    assert M.D == D.INV_D == 0x2e5f0fbadd72321ce14a56699d73f002217f0e679998f19933333332cccccccd
    for v in EDGES:
        assert pow(M.fifth_root(v), 5, P) == v
        assert M.fifth_root(S.quintic_s_box(v)) == v
    assert M.fifth_root(0) == 0 and M.fifth_root(1) == 1 and M.fifth_root(P - 1) == P - 1


def test_model_inverts_the_permutation_both_ways(kat):
    rng = random.Random(0xF11)
    inputs = [[int(v, 16) for v in case["in"]] for case in kat["single"]]
    assert len(inputs) >= 5
    inputs += [[rng.randrange(P) for _ in range(5)] for _ in range(32)]
    for x in inputs:
        y = S.perm(x)
        assert M.perm_inverse(y) == x
        assert S.perm(M.perm_inverse(x)) == x


def test_round_ranges_walk_the_trace_backwards():
    x = [7, 0, P - 1, 1 << 100, 3]
    trace = []
    S.perm(x, trace)
    for hi, lo in M.ROUND_RANGES:
        assert M.inverse_rounds(trace[hi - 1], hi, lo) == (trace[lo - 1] if lo else x), (hi, lo)
    assert M.inverse_rounds(trace[30], 31, 31) == trace[30]


def test_golden_file_is_what_the_model_gives():
    with open(os.path.join(ROOT, "tests", "golden", "perm_inverse_kat.json")) as f:
        committed = json.load(f)
    assert committed == M.golden()
    assert int(committed["D"], 16) == M.D and len(committed["inverse_rounds"]) == len(M.ROUND_RANGES)
    # and the file's cases are what they say: the forward permutation of every preimage is the case's state
    for case in committed["perm_inverse"]:
        assert [hex(v) for v in S.perm([int(v, 16) for v in case["x"]])] == case["y"]


def test_committed_inverse_tables_are_current():
    with open(os.path.join(ROOT, "hades252_amd", "csrc", "hades_inverse_constants.inc")) as f:
        assert f.read() == D.inverse_inc_text()


def test_generated_tables_are_the_models_constants():
    """The product side derives M^-1, the keys and the chain on its own (hades252_amd/_derive.py, independent of oracle/):
    they are the model's."""
    assert [list(row) for row in RI.mds_inverse()] == D.mds_inverse()
    t = D.inverse_tables()
    rp = D.RP % P
    ark = S.round_constants()
    for r in range(RI.ROUNDS):
        for w in range(5):
            assert (t["negkey"][r][w] + ark[5 * r + w] * rp) % P == 0
    assert t["to_rp"] * S.R % P == rp * rp % P and t["from_rp"] == S.R
    # the chain replays to D and costs what the header says
    steps = D.inverse_chain()
    e = D.INV_CHAIN_TABLE[steps[0][1]]
    products = D.INV_TABLE_PRODUCTS
    for nsq, k in steps[1:]:
        e = (e << nsq) + D.INV_CHAIN_TABLE[k]
        products += nsq + 1
    assert e == M.D and products == D.inverse_chain_products() == 311
    assert all(0 < nsq < 32 and 0 <= k < 5 for nsq, k in steps)
    text = D.inverse_inc_text()
    assert "#define HADES_INV_CHAIN_PRODUCTS 311\n" in text and "#define HADES_INV_CHAIN_STEPS %d\n" % len(steps) in text
