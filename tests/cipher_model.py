"""Model of the batched Poseidon cipher (hades252_cipher_*; CONVENTION UNPINNED: dusk-poseidon is outside the reference
tree, the construction is recalled from that crate and pinned only to this model -- include/hades252.h).

Two forms of the same construction:
  * `encrypt` / `decrypt` on canonical integers, one message, over oracle/hades_spec.py::perm (the definition);
  * `encrypt_batch` / `decrypt_batch` on Montgomery limb arrays (the ABI's memory format), a whole batch at once, with the
    permutation passed in (the C oracle's perm_batch), for the GPU tier's large batches.

    state = [D, M, kx, ky, nonce]                     (M as the field element M)
    encrypt: for each block b of 4 words: state = perm(state); for idx = 4b + j < M: state[1+j] += m[idx]; c[idx] = state[1+j]
             state = perm(state); c[M] = state[1]
    decrypt: same start; per block: state = perm(state); m[idx] = c[idx] - state[1+j]; state[1+j] = c[idx]
             state = perm(state); ok = c[M] == state[1] and every c word canonical; if not ok: m = 0
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402

P = S.P
DOMAIN = 1 << 32                     # dusk-poseidon's instance: BlsScalar::from_raw([0x1_0000_0000, 0, 0, 0])
DOMAIN_MONT = S.to_mont(DOMAIN)


def blocks(m: int) -> int:
    return (m + 3) // 4


# ---- one message, canonical integers ----------------------------------------------------------------------------------
def encrypt(msg, key, nonce, domain=DOMAIN, perm=S.perm):
    m = len(msg)
    st = [domain % P, m % P, key[0], key[1], nonce]
    c = []
    for b in range(blocks(m)):
        st = perm(st)
        for j in range(4):
            idx = 4 * b + j
            if idx < m:
                st[1 + j] = (st[1 + j] + msg[idx]) % P
                c.append(st[1 + j])
    st = perm(st)
    c.append(st[1])
    return c


def decrypt(cipher, key, nonce, domain=DOMAIN, perm=S.perm):
    """-> (msg, ok).  Cipher words are integers; one >= P stands for a non-canonical word (rejected)."""
    m = len(cipher) - 1
    canonical = all(0 <= w < P for w in cipher)
    st = [domain % P, m % P, key[0], key[1], nonce]
    msg = []
    for b in range(blocks(m)):
        st = perm(st)
        for j in range(4):
            idx = 4 * b + j
            if idx < m:
                w = cipher[idx] % P
                msg.append((w - st[1 + j]) % P)
                st[1 + j] = w
    st = perm(st)
    ok = canonical and cipher[m] == st[1]
    return (msg if ok else [0] * m), ok


# ---- batches in the memory format (Montgomery limbs, uint64 [..., 4]) --------------------------------------------------
_PL = np.array([(P >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def _add_limbs(a, b):
    """256-bit a + b -> (sum mod 2^256, carry out), limb arrays [..., 4]."""
    s = np.empty_like(a)
    carry = np.zeros(a.shape[:-1], dtype=np.uint64)
    for k in range(4):
        t = a[..., k] + b[..., k]
        c1 = (t < a[..., k]).astype(np.uint64)
        t2 = t + carry
        c2 = (t2 < t).astype(np.uint64)
        s[..., k] = t2
        carry = c1 | c2
    return s, carry


def _sub_limbs(a, b):
    """256-bit a - b -> (difference mod 2^256, borrow out)."""
    d = np.empty_like(a)
    borrow = np.zeros(a.shape[:-1], dtype=np.uint64)
    for k in range(4):
        t = a[..., k] - b[..., k]
        b1 = (a[..., k] < b[..., k]).astype(np.uint64)
        t2 = t - borrow
        b2 = (t < borrow).astype(np.uint64)
        d[..., k] = t2
        borrow = b1 | b2
    return d, borrow


def canonical(a):
    """a < p, per scalar (limb array [..., 4] -> bool [...])."""
    _, borrow = _sub_limbs(a, np.broadcast_to(_PL, a.shape))
    return borrow.astype(bool)


def fr_add(a, b):
    s, carry = _add_limbs(a, b)
    d, borrow = _sub_limbs(s, np.broadcast_to(_PL, s.shape))
    use_d = (carry == 1) | (borrow == 0)
    return np.where(use_d[..., None], d, s)


def fr_sub(a, b):
    d, borrow = _sub_limbs(a, b)
    s, _ = _add_limbs(d, np.broadcast_to(_PL, d.shape))
    return np.where((borrow == 1)[..., None], s, d)


def limbs(x: int):
    """the 256-bit integer x as 4 u64 limbs (no conversion)"""
    return np.array([(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def int_of(w) -> int:
    return sum(int(x) << (64 * k) for k, x in enumerate(w))


def mont_limbs(v: int):
    """the field element v in the memory format (Montgomery limbs)"""
    return limbs(S.to_mont(v % P))


def _start(keys, nonces, m, domain_mont):
    n = nonces.shape[0]
    st = np.empty((n, 5, 4), dtype=np.uint64)
    st[:, 0] = limbs(domain_mont)
    st[:, 1] = mont_limbs(m)
    st[:, 2:4] = keys.reshape(n, 2, 4)
    st[:, 4] = nonces.reshape(n, 4)
    return st


def _permute(st, perm_batch):
    return np.ascontiguousarray(perm_batch(np.ascontiguousarray(st).reshape(-1))).view(np.uint64).reshape(st.shape)


def encrypt_batch(msgs, keys, nonces, m, perm_batch, domain_mont=DOMAIN_MONT):
    """msgs [n, m, 4], keys [n, 2, 4], nonces [n, 4] (uint64 Montgomery limbs) -> ciphers [n, m + 1, 4]."""
    n = nonces.reshape(-1, 4).shape[0]
    msgs = np.asarray(msgs, dtype=np.uint64).reshape(n, m, 4)
    st = _start(keys, nonces, m, domain_mont)
    c = np.empty((n, m + 1, 4), dtype=np.uint64)
    for b in range(blocks(m)):
        st = _permute(st, perm_batch)
        for j in range(min(4, m - 4 * b)):
            idx = 4 * b + j
            st[:, 1 + j] = fr_add(st[:, 1 + j], msgs[:, idx])
            c[:, idx] = st[:, 1 + j]
    st = _permute(st, perm_batch)
    c[:, m] = st[:, 1]
    return c


def decrypt_batch(ciphers, keys, nonces, m, perm_batch, domain_mont=DOMAIN_MONT):
    """ciphers [n, m + 1, 4] -> (msgs [n, m, 4], ok [n] uint8); rejected messages are zeros."""
    n = nonces.reshape(-1, 4).shape[0]
    ciphers = np.asarray(ciphers, dtype=np.uint64).reshape(n, m + 1, 4)
    good = canonical(ciphers).all(axis=1)
    st = _start(keys, nonces, m, domain_mont)
    out = np.empty((n, m, 4), dtype=np.uint64)
    for b in range(blocks(m)):
        st = _permute(st, perm_batch)
        for j in range(min(4, m - 4 * b)):
            idx = 4 * b + j
            out[:, idx] = fr_sub(ciphers[:, idx], st[:, 1 + j])
            st[:, 1 + j] = ciphers[:, idx]
    st = _permute(st, perm_batch)
    good &= (ciphers[:, m] == st[:, 1]).all(axis=1)
    out[~good] = 0
    return out, good.astype(np.uint8)


def spec_perm_batch(flat):
    """hades_spec.perm over a flat limb array of whole states (slow: for small CPU-tier batches)."""
    a = np.asarray(flat, dtype=np.uint64).reshape(-1, 20)
    return np.array([S.perm_mont_limbs([int(x) for x in row]) for row in a], dtype=np.uint64).reshape(-1)
