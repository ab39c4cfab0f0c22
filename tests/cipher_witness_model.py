"""Big-integer model of the input states of the cipher witnesses (include/hades252.h, "gadget witnesses of the cipher"),
from the definition of tests/cipher_model.py on the spec oracle (oracle/hades_spec.py).  CONVENTION UNPINNED, as there.
Values are canonical integers (not Montgomery form); a cipher word may be any 256-bit integer.

A batch of n messages of M words is S * n permutations, S = ceil(M / 4) + 1; inputs[s][i] enters permutation (s, i).
  inputs[0][i] = [D, M, kx, ky, nonce]
  encrypt: inputs[s][i] = perm(inputs[s - 1][i]) with message word 4 (s - 1) + j added to word 1 + j (the words that
           exist); those sums are the cipher words, and word 1 of perm(inputs[S - 1][i]) is the tag
  decrypt: inputs[s][i] = perm(inputs[s - 1][i]) with word 1 + j replaced by cipher word 4 (s - 1) + j mod p

`perm_many` (a list of states -> the list of their permutations) defaults to the spec's `perm`, one state at a time; a
caller with many states may hand in a batched one (the C oracle)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402

import cipher_model as C  # noqa: E402

P = S.P
MAX_LEN = 1024                  # HADES252_CIPHER_MAX_LEN


def _spec_perm_many(states):
    return [S.perm(list(s)) for s in states]


def cipher_perms(msg_len: int) -> int:
    """Permutations per message: ceil(M / 4) + 1 for 1 <= M <= MAX_LEN, else 0 (hades252_cipher_perms)."""
    if not 1 <= msg_len <= MAX_LEN:
        return 0
    return C.blocks(msg_len) + 1


def _chain(words, keys, nonces, m, domain, absorb, perm_many):
    """(inputs [S][n][5], outputs [S][n][5]): outputs[s] = the permutations of inputs[s]; absorb(state word, word) -> the
    new state word."""
    n_steps = cipher_perms(m)
    assert n_steps, m
    inputs = [[[domain % P, m % P, k[0], k[1], nc] for k, nc in zip(keys, nonces)]]
    outputs = [perm_many(inputs[0])]
    for s in range(1, n_steps):
        step = []
        for i, st in enumerate(outputs[-1]):
            st = list(st)
            for j in range(4):
                idx = 4 * (s - 1) + j
                if idx < m:
                    st[1 + j] = absorb(st[1 + j], words[i][idx])
            step.append(st)
        inputs.append(step)
        outputs.append(perm_many(step))
    return inputs, outputs


def encrypt_inputs(msgs, keys, nonces, domain=C.DOMAIN, perm_many=None):
    """-> (inputs [S][n][5], ciphers [n][M + 1]).  Every message has the same length M >= 1."""
    m = len(msgs[0])
    inputs, outputs = _chain(msgs, keys, nonces, m, domain, lambda a, b: (a + b) % P, perm_many or _spec_perm_many)
    ciphers = [[inputs[1 + k // 4][i][1 + k % 4] for k in range(m)] + [outputs[-1][i][1]] for i in range(len(msgs))]
    return inputs, ciphers


def decrypt_inputs(ciphers, keys, nonces, domain=C.DOMAIN, perm_many=None):
    """-> (inputs [S][n][5], msgs [n][M], ok [n]).  Cipher words are 256-bit integers; the states hold them mod p.  A
    rejected message (a word >= p, or a wrong tag) comes out as M zeros, as from cipher_model.decrypt."""
    m = len(ciphers[0]) - 1
    inputs, outputs = _chain(ciphers, keys, nonces, m, domain, lambda a, b: b % P, perm_many or _spec_perm_many)
    msgs, oks = [], []
    for i, c in enumerate(ciphers):
        ok = all(0 <= w < P for w in c) and c[m] == outputs[-1][i][1]
        # message word = the reduced cipher word - the permutation output word it replaces
        msg = [(c[k] % P - outputs[k // 4][i][1 + k % 4]) % P for k in range(m)]
        oks.append(ok)
        msgs.append(msg if ok else [0] * m)
    return inputs, msgs, oks
