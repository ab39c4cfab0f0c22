"""CPU tier: the duplex sponge model (tests/safe_model.py) -- the zero-fill sponge and the arity-4 Merkle node as instances,
aggregation of split calls, the closed-form permutation count, the batch form against the integer form, the cipher composed
over the sponge, and the committed known answers (tests/golden/safe_kat.json), which lock the (UNPINNED) convention against
drift."""
import json
import os
import random

import numpy as np
import pytest

import cipher_model as C
import safe_model as M
from safe_model import A, Q, P, S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "safe_kat.json")


def _random_pattern(rng, max_calls=6, max_len=9):
    pat = [A(rng.randrange(1, max_len + 1))]
    for _ in range(rng.randrange(0, max_calls - 1)):
        pat.append((rng.choice(["absorb", "squeeze"]), rng.randrange(1, max_len + 1)))
    pat.append(Q(rng.randrange(1, max_len + 1)))
    return pat


@pytest.mark.parametrize("length", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17])
def test_absorb_then_one_word_is_the_zero_fill_sponge(length):
    rng = random.Random(300 + length)
    msg, cap = [rng.randrange(P) for _ in range(length)], rng.randrange(P)
    out, perms = M.run([A(length), Q(1)], msg, cap)
    assert out == [S.sponge_hash(msg, cap, pad_mode=0)]
    assert perms == (length + 3) // 4


def test_four_words_with_tag_15_is_the_merkle_node():
    rng = random.Random(11)
    children = [rng.randrange(P) for _ in range(4)]
    assert M.run([A(4), Q(1)], children, 15) == ([S.merkle4_node(children)], 1)


def test_squeeze_draws_more_than_one_block():
    """nine words out of one absorbed word: three permutations, words 1..4 of each state in turn"""
    st = S.perm([7, 5, 0, 0, 0])
    want = st[1:5]
    st = S.perm(st)
    want += st[1:5]
    st = S.perm(st)
    want += st[1:2]
    assert M.run([A(1), Q(9)], [5], 7) == (want, 3)


def test_absorb_after_squeeze_adds_from_position_0_of_the_squeezed_state():
    st = S.perm([3, 10, 20, 30, 0])
    out = st[1:3]
    st[1] = (st[1] + 40) % P
    st[2] = (st[2] + 50) % P
    st = S.perm(st)
    assert M.run([A(3), Q(2), A(2), Q(1)], [10, 20, 30, 40, 50], 3) == (out + [st[1]], 2)


def test_any_split_of_a_call_changes_nothing():
    rng = random.Random(21)
    toy = lambda st: [(3 * st[(i + 1) % 5] + st[i] * st[i] + i + 1) % P for i in range(5)]      # noqa: E731
    for it in range(200):
        pat = _random_pattern(rng)
        split = []
        for kind, n in pat:
            while n:
                c = rng.randrange(1, n + 1)
                split.append((kind, c))
                n -= c
        inputs, tag = [rng.randrange(P) for _ in range(M.words_in(pat))], rng.randrange(P)
        perm = S.perm if it < 8 else toy                       # the real permutation for a few, a toy one for the many
        assert M.run(split, inputs, tag, perm) == M.run(pat, inputs, tag, perm)      # (at most 6 x 9 = 54 calls)
        assert M.aggregate(split) == M.aggregate(pat)
        assert M.tag_input(split, 5) == M.tag_input(pat, 5)


def test_permutation_count_has_a_closed_form():
    rng = random.Random(22)
    ident = lambda st: list(st)                                 # noqa: E731
    for _ in range(300):
        pat = _random_pattern(rng, max_calls=8, max_len=23)
        _, perms = M.run(pat, [0] * M.words_in(pat), 1, ident)
        assert perms == M.perms_closed_form(pat), pat
    assert M.perms_closed_form([A(4), Q(1)]) == 1 and M.perms_closed_form([A(5), Q(6)]) == 3
    assert M.perms_closed_form([A(1), Q(64)]) == 16 and M.perms_closed_form(M.cipher_pattern(2)) == 2


def test_validity():
    assert M.valid([A(1), Q(1)]) and M.valid([A(1)] * 63 + [Q(1)]) and M.valid([A(1 << 20), Q(1 << 20)])
    for bad in ([], [Q(1)], [A(1)], [Q(1), A(1), Q(1)], [A(0), Q(1)], [A(1), Q(0)], [A(1)] * 64 + [Q(1)],
                [A((1 << 20) + 1), Q(1)], [A(1), Q((1 << 20) + 1)], [A(1 << 20), A(1), Q(1)]):
        assert not M.valid(bad), bad[:3]


def test_tag_input_bytes():
    assert M.tag_input([A(2), A(1), Q(1)], 7) == bytes.fromhex("80000003" "00000001" "0000000000000007")
    assert M.encode([A(3), Q(2)]) == [0x80000003, 2]


def test_batch_model_equals_integer_model():
    rng = random.Random(23)
    for pat in ([A(4), Q(1)], [A(3), Q(2), A(2), Q(1)], [A(5), Q(6)], [A(2), A(1), Q(1), Q(2)]):
        cases = [[rng.randrange(P) for _ in range(M.words_in(pat))] for _ in range(3)]
        tag = rng.randrange(P)
        inputs = np.array([[C.mont_limbs(v) for v in case] for case in cases], dtype=np.uint64)
        got = M.run_batch(pat, inputs, S.to_mont(tag), C.spec_perm_batch)
        for i, case in enumerate(cases):
            assert [S.from_mont(C.int_of(w)) for w in got[i]] == M.run(pat, case, tag)[0]


@pytest.mark.parametrize("m", [1, 2, 4, 5, 9])
def test_cipher_over_the_sponge_round_trips_and_follows_its_pattern(m):
    rng = random.Random(400 + m)
    msg, key, nonce, tag = [rng.randrange(P) for _ in range(m)], [rng.randrange(P), rng.randrange(P)], rng.randrange(P), \
        rng.randrange(P)
    c = M.cipher_encrypt(msg, key, nonce, tag)
    assert len(c) == m + 1
    assert M.cipher_decrypt(c, key, nonce, tag) == (msg, True)
    bad = list(c)
    bad[0] = (bad[0] + 1) % P
    assert not M.cipher_decrypt(bad, key, nonce, tag)[1]
    # the same words through the one-shot pattern: the squeezed words are cipher - message, then the tag word
    out, _ = M.run(M.cipher_pattern(m), key + [nonce] + msg, tag)
    assert [(x + k) % P for x, k in zip(msg, out[:m])] + out[m:] == c


def kat_cases():
    """The inputs of tests/golden/safe_kat.json: seeded patterns and canonical integers (not Montgomery form)."""
    pats = [[A(4), Q(1)], [A(1), Q(9)], [A(5), Q(6)], [A(3), Q(2), A(2), Q(1)], [A(2), A(1), Q(1), Q(2)], M.cipher_pattern(2),
            M.cipher_pattern(5)]
    out = []
    for seed, pat in enumerate(pats, 1):
        rng = random.Random(0x5AFE + seed)
        out.append({"seed": seed, "pattern": pat, "tag": rng.randrange(P),
                    "inputs": [rng.randrange(P) for _ in range(M.words_in(pat))]})
    return out


def render_kat():
    cases = []
    for c in kat_cases():
        outputs, perms = M.run(c["pattern"], c["inputs"], c["tag"])
        case = {"seed": c["seed"], "pattern": [[k, n] for k, n in c["pattern"]], "tag": hex(c["tag"]),
                "inputs": [hex(v) for v in c["inputs"]], "outputs": [hex(v) for v in outputs], "perms": perms}
        if c["pattern"][:2] == [A(2), A(1)] and len(c["pattern"]) == 5:      # the cipher shape: inputs = key, nonce, message
            case["cipher"] = [hex(v) for v in M.cipher_encrypt(c["inputs"][3:], c["inputs"][:2], c["inputs"][2], c["tag"])]
        cases.append(case)
    return {"about": "duplex sponge known answers (CONVENTION UNPINNED, include/hades252.h), generated by tests/safe_model.py; "
                     "values are canonical integers, not Montgomery form; `cipher` = message + squeezed words, then the "
                     "last squeezed word, for the cases of the cipher shape (inputs = key x 2, nonce, message)",
            "cases": cases}


def test_known_answers_are_rederived_exactly():
    with open(KAT) as f:
        committed = json.load(f)
    assert committed == render_kat()
    assert len(committed["cases"]) == 7
    for case in committed["cases"]:
        if "cipher" in case:
            ints = lambda xs: [int(x, 16) for x in xs]            # noqa: E731
            inp, tag = ints(case["inputs"]), int(case["tag"], 16)
            assert M.cipher_decrypt(ints(case["cipher"]), inp[:2], inp[2], tag) == (inp[3:], True)


if __name__ == "__main__":          # regenerate the golden file (only when the convention changes on purpose)
    with open(KAT, "w") as f:
        json.dump(render_kat(), f, indent=1)
        f.write("\n")
