"""CPU tier: the model of the cipher witnesses' input states (tests/cipher_witness_model.py) against the cipher's own model
(tests/cipher_model.py) and its committed known answers -- the final state's word 1 is the tag, encrypt's cipher words are
the absorbed input words, decrypting an encryption rebuilds the same states, non-canonical cipher words (p, 2p, 2^256 - 1)
enter the states reduced and reject the message."""
import json
import os
import random

import pytest

import cipher_model as C
import cipher_witness_model as CW
from cipher_witness_model import P, S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(rng, n, m):
    msgs = [[rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(m)] for _ in range(n)]
    keys = [[rng.randrange(P), rng.randrange(P)] for _ in range(n)]
    nonces = [rng.randrange(P) for _ in range(n)]
    return msgs, keys, nonces


def test_cipher_perms():
    assert [CW.cipher_perms(m) for m in range(0, 10)] == [0, 2, 2, 2, 2, 3, 3, 3, 3, 4]
    assert CW.cipher_perms(CW.MAX_LEN) == CW.MAX_LEN // 4 + 1 and CW.cipher_perms(CW.MAX_LEN + 1) == 0


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 9])
def test_chains_match_the_cipher_model(m):
    rng = random.Random(0xC1 + m)
    msgs, keys, nonces = _batch(rng, 2, m)
    dom = rng.choice([C.DOMAIN, rng.randrange(P)])
    inputs, ciphers = CW.encrypt_inputs(msgs, keys, nonces, dom)
    assert len(inputs) == CW.cipher_perms(m) and all(len(step) == 2 for step in inputs)
    for i in range(2):
        assert inputs[0][i] == [dom, m, keys[i][0], keys[i][1], nonces[i]]
        assert ciphers[i] == C.encrypt(msgs[i], keys[i], nonces[i], dom)
        # the tag is word 1 of the final permutation's output
        assert S.perm(list(inputs[-1][i]))[1] == ciphers[i][m]
        for s in range(1, len(inputs)):                # word 0 passes through; words 1 + j absorb (or keep) their word
            prev = S.perm(list(inputs[s - 1][i]))
            assert inputs[s][i][0] == prev[0]
            for j in range(4):
                k = 4 * (s - 1) + j
                want = (prev[1 + j] + msgs[i][k]) % P if k < m else prev[1 + j]
                assert inputs[s][i][1 + j] == want
                if k < m:
                    assert inputs[s][i][1 + j] == ciphers[i][k]       # the cipher words ARE the absorbed words
    # decrypt of the encryption: the same states, the messages back, accepted
    d_inputs, d_msgs, oks = CW.decrypt_inputs(ciphers, keys, nonces, dom)
    assert d_inputs == inputs and d_msgs == msgs and oks == [True, True]
    for i in range(2):
        assert (d_msgs[i], oks[i]) == C.decrypt(ciphers[i], keys[i], nonces[i], dom)


def test_known_answers():
    with open(os.path.join(ROOT, "tests", "golden", "cipher_kat.json")) as f:
        kat = json.load(f)
    dom = int(kat["domain"], 16)
    for case in kat["cases"]:
        msg = [int(v, 16) for v in case["msg"]]
        key = [int(v, 16) for v in case["key"]]
        nonce = int(case["nonce"], 16)
        cipher = [int(v, 16) for v in case["cipher"]]
        inputs, ciphers = CW.encrypt_inputs([msg], [key], [nonce], dom)
        assert ciphers == [cipher], case["seed"]
        assert S.perm(list(inputs[-1][0]))[1] == cipher[-1]
        d_inputs, d_msgs, oks = CW.decrypt_inputs([cipher], [key], [nonce], dom)
        assert d_inputs == inputs and d_msgs == [msg] and oks == [True]
        bad = list(cipher)
        bad[-1] = (bad[-1] + 1) % P                    # a wrong tag: the same states, the message zeroed
        d_inputs, d_msgs, oks = CW.decrypt_inputs([bad], [key], [nonce], dom)
        assert d_inputs == inputs and d_msgs == [[0] * len(msg)] and oks == [False]


@pytest.mark.parametrize("m", [2, 5])
def test_non_canonical_words_enter_reduced(m):
    rng = random.Random(77 + m)
    msgs, keys, nonces = _batch(rng, 1, m)
    _, ciphers = CW.encrypt_inputs(msgs, keys, nonces)
    ref_inputs, _, _ = CW.decrypt_inputs(ciphers, keys, nonces)
    for k in range(m + 1):
        for big in (P, 2 * P, (1 << 256) - 1):
            c = list(ciphers[0])
            c[k] = big if big == (1 << 256) - 1 else c[k] + big
            if c[k] >= 1 << 256:
                continue
            inputs, out, oks = CW.decrypt_inputs([c], keys, nonces)
            assert oks == [False] and out == [[0] * m], (k, big)
            assert all(0 <= v < P for step in inputs for st in step for v in st)
            # the states change only where a reduced message word differs (the tag enters no state)
            assert (k == m or c[k] % P == ciphers[0][k]) == (inputs == ref_inputs), (k, big)
            msg, ok = C.decrypt(c, keys[0], nonces[0])
            assert (msg, ok) == (out[0], False)
            if k < m:                                   # the reduced word sits in its state
                assert inputs[1 + k // 4][0][1 + k % 4] == c[k] % P
