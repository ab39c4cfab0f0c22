"""Model of the batched proof-of-work grinding (hades252_grind; CONVENTION UNPINNED: nothing in the reference tree defines a
proof of work, the definition is this repository's own and pinned only to this model -- include/hades252.h).

    candidate(x) = the seed (five field elements) with seed[word] + x (mod p) in place of seed[word],  0 <= x < 2^64
    digest(x)    = word out_idx of perm(candidate(x)) as a canonical integer (the to_bytes value, not the Montgomery limbs)
    x is a hit  <=>  digest(x) < target    (strictly; target any integer in [0, 2^256): 0 never hits, >= p always does)
    answer       = the smallest hit in [first, first + max_n), or None

Two forms of the same definition:
  * `digest` / `first_hit` / `hits` on canonical integers, one job, over oracle/hades_spec.py::perm (the definition);
  * `first_hit_batch` / `hits_batch` on Montgomery limb arrays (the ABI's memory format), many jobs at once, with the
    permutation passed in (the C oracle's perm_batch).  Candidates are evaluated in chunks of CHUNK per unfinished job, so a
    batch costs little more than the candidates up to each job's hit.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402

from cipher_model import int_of, limbs, mont_limbs  # noqa: E402  (the memory format)

P = S.P
CHUNK = 256
MAX_NONCE = 1 << 64


def target_bits(bits: int) -> int:
    return P >> bits


def _check(word, out_idx, target, first, max_n):
    assert 0 <= word < 5 and 0 <= out_idx < 5 and 0 <= target < 1 << 256
    assert first >= 0 and max_n >= 0 and first + max_n <= MAX_NONCE


# ---- one job, canonical integers --------------------------------------------------------------------------------------
def digest(seed_values, word: int, out_idx: int, x: int, perm=S.perm) -> int:
    st = [v % P for v in seed_values]
    st[word] = (st[word] + x) % P
    return perm(st)[out_idx]


def first_hit(seed_values, word: int, out_idx: int, target: int, first: int = 0, max_n: int = 1 << 32, perm=S.perm):
    """-> the smallest hit in [first, first + max_n), or None"""
    _check(word, out_idx, target, first, max_n)
    if target == 0:
        return None
    for x in range(first, first + max_n):
        if digest(seed_values, word, out_idx, x, perm) < target:
            return x
    return None


def hits(seed_values, word: int, out_idx: int, target: int, count: int, first: int = 0, perm=S.perm):
    """the first `count` hits from `first` on (the range must hold them)"""
    out = []
    while len(out) < count:
        out.append(first_hit(seed_values, word, out_idx, target, first, MAX_NONCE - first, perm))
        first = out[-1] + 1
    return out


# ---- batches in the memory format (Montgomery limbs, uint64 [n, 5, 4]) -------------------------------------------------
def seeds_of(values):
    """[[v0 .. v4], ...] canonical integers -> uint64 [n, 5, 4] Montgomery limbs"""
    return np.array([[mont_limbs(v) for v in job] for job in values], dtype=np.uint64).reshape(-1, 5, 4)


def digests_batch(seeds, word: int, out_idx: int, nonces, perm_batch):
    """seeds [n, 5, 4], nonces: one list of integers per job (all of one length m) -> canonical digests, n lists of m"""
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1, 5, 4)
    n, m = seeds.shape[0], len(nonces[0]) if len(nonces) else 0
    if n == 0 or m == 0:
        return [[] for _ in range(n)]
    st = np.repeat(seeds[:, None], m, axis=1)                                  # [n, m, 5, 4]
    for j in range(n):
        base = S.from_mont(int_of(seeds[j, word]))
        st[j, :, word] = [mont_limbs(base + x) for x in nonces[j]]
    out = np.asarray(perm_batch(np.ascontiguousarray(st).reshape(-1))).view(np.uint64).reshape(n, m, 5, 4)
    return [[S.from_mont(int_of(out[j, i, out_idx])) for i in range(m)] for j in range(n)]


def first_hit_batch(seeds, word: int, out_idx: int, target: int, first: int, max_n: int, perm_batch):
    """-> (nonces: list of int or None per job)"""
    _check(word, out_idx, target, first, max_n)
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1, 5, 4)
    answer = [None] * seeds.shape[0]
    if target == 0:
        return answer
    open_jobs, at = list(range(seeds.shape[0])), first
    while open_jobs and at < first + max_n:
        xs = list(range(at, min(at + CHUNK, first + max_n)))
        ds = digests_batch(seeds[open_jobs], word, out_idx, [xs] * len(open_jobs), perm_batch)
        still = []
        for j, row in zip(open_jobs, ds):
            hit = next((x for x, d in zip(xs, row) if d < target), None)
            if hit is None:
                still.append(j)
            else:
                answer[j] = hit
        open_jobs, at = still, at + CHUNK
    return answer


def hits_batch(seed, word: int, out_idx: int, target: int, count: int, perm_batch, first: int = 0):
    """the first `count` hits of ONE job (seed [5, 4]) from `first` on"""
    out = []
    while len(out) < count:
        out.append(first_hit_batch(seed, word, out_idx, target, first, MAX_NONCE - first, perm_batch)[0])
        first = out[-1] + 1
    return out
