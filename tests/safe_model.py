"""Model of the batched duplex sponge (hades252_safe_*; CONVENTION UNPINNED: dusk-safe / dusk-poseidon are outside the
reference tree, the construction is recalled from those crates and pinned only to this model -- include/hades252.h).

Two forms of the same construction:
  * `Sponge` / `run` on canonical integers, one sponge, over oracle/hades_spec.py::perm (the definition);
  * `run_batch` on Montgomery limb arrays (the ABI's memory format), a whole batch at once, with the permutation passed in
    (the C oracle's perm_batch), for the GPU tier's large batches.

    state = [tag, 0, 0, 0, 0]; pos_absorb = 0; pos_squeeze = 0
    absorb(x ..):  for each x: if pos_absorb == 4: state = perm(state); pos_absorb = 0
                               state[1 + pos_absorb] += x; pos_absorb += 1
                   afterwards: pos_squeeze = 4
    squeeze(n):    n times:    if pos_squeeze == 4: state = perm(state); pos_squeeze = 0; pos_absorb = 0
                               output state[1 + pos_squeeze]; pos_squeeze += 1

A pattern is a list like [("absorb", 3), ("squeeze", 2)]: not empty, starts with an absorb, ends with a squeeze, no call of
length 0, at most MAX_CALLS calls and MAX_WORDS words in and out.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402

from cipher_model import fr_add, limbs, _permute  # noqa: E402  (limb arithmetic of the memory format)

P = S.P
RATE = 4
MAX_CALLS = 64
MAX_WORDS = 1 << 20
ABSORB_BIT = 1 << 31


def A(n):
    return ("absorb", n)


def Q(n):
    return ("squeeze", n)


def valid(pattern) -> bool:
    if not pattern or len(pattern) > MAX_CALLS or pattern[0][0] != "absorb" or pattern[-1][0] != "squeeze":
        return False
    if any(kind not in ("absorb", "squeeze") or n <= 0 for kind, n in pattern):
        return False
    return words_in(pattern) <= MAX_WORDS and words_out(pattern) <= MAX_WORDS


def aggregate(pattern):
    out = []
    for kind, n in pattern:
        if out and out[-1][0] == kind:
            out[-1] = (kind, out[-1][1] + n)
        else:
            out.append((kind, n))
    return out


def words_in(pattern) -> int:
    return sum(n for kind, n in pattern if kind == "absorb")


def words_out(pattern) -> int:
    return sum(n for kind, n in pattern if kind == "squeeze")


def perms_closed_form(pattern) -> int:
    """Permutations of a valid pattern: per aggregated call, ceil(L / 4) - 1 for an absorb (its words fill blocks that the
    NEXT call's first permutation closes) and ceil(L / 4) for a squeeze."""
    return sum((n + 3) // 4 - (1 if kind == "absorb" else 0) for kind, n in aggregate(pattern))


def encode(pattern):
    """the calls as SAFE's 32-bit words: bit 31 = absorb, low 31 bits = length"""
    return [(ABSORB_BIT if kind == "absorb" else 0) | n for kind, n in pattern]


def tag_input(pattern, domain_sep: int) -> bytes:
    """the bytes SAFE hashes into a tag: the aggregated calls as big-endian 32-bit words, then the 64-bit domain separator"""
    return b"".join(w.to_bytes(4, "big") for w in encode(aggregate(pattern))) + domain_sep.to_bytes(8, "big")


# ---- one sponge, canonical integers -----------------------------------------------------------------------------------
class Sponge:
    def __init__(self, tag: int, perm=S.perm):
        self.state = [tag % P, 0, 0, 0, 0]
        self.pos_absorb = 0
        self.pos_squeeze = 0
        self.perm = perm
        self.n_perms = 0

    def _permute(self):
        self.state = self.perm(self.state)
        self.n_perms += 1

    def absorb(self, xs):
        for x in xs:
            if self.pos_absorb == RATE:
                self._permute()
                self.pos_absorb = 0
            self.state[1 + self.pos_absorb] = (self.state[1 + self.pos_absorb] + x) % P
            self.pos_absorb += 1
        if len(xs):
            self.pos_squeeze = RATE

    def squeeze(self, n: int):
        out = []
        for _ in range(n):
            if self.pos_squeeze == RATE:
                self._permute()
                self.pos_squeeze = 0
                self.pos_absorb = 0
            out.append(self.state[1 + self.pos_squeeze])
            self.pos_squeeze += 1
        return out


def run(pattern, inputs, tag: int, perm=S.perm):
    """-> (outputs in call order, permutations used)"""
    assert valid(pattern) and len(inputs) == words_in(pattern)
    sp, out, at = Sponge(tag, perm), [], 0
    for kind, n in pattern:
        if kind == "absorb":
            sp.absorb(inputs[at:at + n])
            at += n
        else:
            out += sp.squeeze(n)
    return out, sp.n_perms


# ---- the new cipher, composed as a caller composes it -----------------------------------------------------------------
def cipher_pattern(m: int):
    return [A(2), A(1), Q(m), A(m), Q(1)]


def cipher_encrypt(msg, key, nonce, tag: int, perm=S.perm):
    """[A(2) key, A(1) nonce, S(M), A(M) message, S(1)]: cipher = message + squeezed words, then the last squeezed word"""
    sp = Sponge(tag, perm)
    sp.absorb(list(key))
    sp.absorb([nonce])
    ks = sp.squeeze(len(msg))
    sp.absorb(list(msg))
    return [(m + k) % P for m, k in zip(msg, ks)] + sp.squeeze(1)


def cipher_decrypt(cipher, key, nonce, tag: int, perm=S.perm):
    """-> (message, ok)"""
    m = len(cipher) - 1
    sp = Sponge(tag, perm)
    sp.absorb(list(key))
    sp.absorb([nonce])
    ks = sp.squeeze(m)
    msg = [(c - k) % P for c, k in zip(cipher[:m], ks)]
    sp.absorb(msg)
    return msg, sp.squeeze(1)[0] == cipher[m]


# ---- batches in the memory format (Montgomery limbs, uint64 [..., 4]) --------------------------------------------------
class SpongeBatch:
    """n sponges that follow the same calls; `state` is the 160-byte AoS state array of the ABI."""

    def __init__(self, n: int, tag_mont: int, perm_batch):
        self.state = np.zeros((n, 5, 4), dtype=np.uint64)
        self.state[:, 0] = limbs(tag_mont)
        self.pos_absorb = self.pos_squeeze = 0
        self.perm_batch = perm_batch

    def absorb(self, xs):
        """xs [n, len, 4]"""
        for i in range(xs.shape[1]):
            if self.pos_absorb == RATE:
                self.state = _permute(self.state, self.perm_batch)
                self.pos_absorb = 0
            self.state[:, 1 + self.pos_absorb] = fr_add(self.state[:, 1 + self.pos_absorb], xs[:, i])
            self.pos_absorb += 1
        if xs.shape[1]:
            self.pos_squeeze = RATE

    def squeeze(self, k: int):
        out = np.empty((self.state.shape[0], k, 4), dtype=np.uint64)
        for i in range(k):
            if self.pos_squeeze == RATE:
                self.state = _permute(self.state, self.perm_batch)
                self.pos_squeeze = 0
                self.pos_absorb = 0
            out[:, i] = self.state[:, 1 + self.pos_squeeze]
            self.pos_squeeze += 1
        return out


def run_batch(pattern, inputs, tag_mont: int, perm_batch):
    """inputs [n, words_in, 4] (uint64 Montgomery limbs) -> outputs [n, words_out, 4]"""
    assert valid(pattern)
    inputs = np.asarray(inputs, dtype=np.uint64).reshape(-1, words_in(pattern), 4)
    sp, outs, at = SpongeBatch(inputs.shape[0], tag_mont, perm_batch), [], 0
    for kind, k in pattern:
        if kind == "absorb":
            sp.absorb(inputs[:, at:at + k])
            at += k
        else:
            outs.append(sp.squeeze(k))
    return np.concatenate(outs, axis=1)
