"""CPU tier: the model of the proof-of-work grinding (tests/grind_model.py, the definition of hades252_grind: CONVENTION
UNPINNED).  Its two forms -- canonical integers over the Python specification, Montgomery limb batches over the C oracle --
agree; the anchor values below (the first four hits of two seeds at a ladder of targets) are recomputed and asserted
literally; the edges of the definition (strict compare, target 0, targets >= p, range ends, the field wrap of the nonce
word) hold in the model itself."""
import random

import numpy as np
import pytest

import grind_model as M
from cipher_model import int_of, spec_perm_batch
from grind_model import P, S

SEED_A, SEED_B = [1 << 64, 1, 2, 3, 4], [15, 0, 0, 0, 0]
# (seed values, word, out_idx) -> {bits: the first four hits from nonce 0 at target p >> bits}
ANCHORS = {
    "a": (SEED_A, 4, 1, {4: [6, 18, 20, 48], 6: [93, 105, 124, 178], 8: [105, 178, 189, 571], 10: [571, 594, 1620, 1808],
                         12: [5003, 5032, 5134, 5215], 14: [5003, 5032, 21011, 26327], 16: [5003, 26327, 85670, 121255]}),
    "b": (SEED_B, 1, 1, {4: [19, 67, 114, 159], 8: [228, 280, 421, 541], 10: [228, 834, 860, 2005]}),
}


@pytest.mark.parametrize("which,bits", [(w, b) for w in sorted(ANCHORS) for b in sorted(ANCHORS[w][3])])
def test_anchors_recomputed_with_the_c_oracle(oracle, which, bits):
    values, word, out_idx, table = ANCHORS[which]
    got = M.hits_batch(M.seeds_of([values])[0], word, out_idx, P >> bits, 4, oracle.perm_batch)
    assert got == table[bits]


def test_small_anchors_recomputed_with_the_python_specification():
    """the definition itself (hades_spec.perm on canonical integers), where it is quick enough: about 400 permutations"""
    assert M.hits(SEED_A, 4, 1, P >> 4, 4) == [6, 18, 20, 48]
    assert M.hits(SEED_B, 1, 1, P >> 4, 4) == [19, 67, 114, 159]
    assert M.first_hit(SEED_A, 4, 1, P >> 6, 0, 200) == 93
    # every hit of the ladder is a hit, and its predecessor is not unless the table says so
    for values, word, out_idx, table in ANCHORS.values():
        for bits, xs in table.items():
            for x in xs[:2]:
                assert M.digest(values, word, out_idx, x) < P >> bits
                assert x - 1 in xs or x == 0 or M.digest(values, word, out_idx, x - 1) >= P >> bits


@pytest.mark.parametrize("bits", [4, 6])
def test_the_two_forms_agree_on_random_seeds(oracle, bits):
    rng = random.Random(100 + bits)
    jobs = [[rng.randrange(P) for _ in range(5)] for _ in range(4)]
    word, out_idx, first = rng.randrange(5), rng.randrange(5), rng.randrange(1 << 40)
    want = [M.first_hit(v, word, out_idx, P >> bits, first, 400) for v in jobs]
    assert any(w is not None for w in want)
    assert M.first_hit_batch(M.seeds_of(jobs), word, out_idx, P >> bits, first, 400, oracle.perm_batch) == want
    # ... and over the Python specification as the batch's permutation (no C code at all), on the first two jobs
    assert M.first_hit_batch(M.seeds_of(jobs[:2]), word, out_idx, P >> bits, first, 400, spec_perm_batch) == want[:2]


def test_edges_of_the_definition(oracle):
    seeds = M.seeds_of([SEED_A])
    pb = oracle.perm_batch
    one = lambda target, first, max_n: M.first_hit_batch(seeds, 4, 1, target, first, max_n, pb)[0]  # noqa: E731
    assert one(0, 0, 1000) is None                                   # target 0 never hits
    assert one(P, 7, 1) == 7 and one((1 << 256) - 1, 9, 5) == 9      # anything >= p hits at once
    assert one(P >> 10, 0, 571) is None and one(P >> 10, 0, 572) == 571
    assert one(P >> 4, 7, 100) == 18 and one(P >> 4, 18, 1) == 18 and one(P >> 4, 19, 1) is None
    assert one(P >> 10, 572, 2000) == 594
    assert one(P >> 4, 5, 0) is None                                 # an empty range
    v = M.digests_batch(seeds, 4, 1, [[571]], pb)[0][0]
    assert v == M.digest(SEED_A, 4, 1, 571) and v < P >> 10
    assert one(v + 1, 0, 572) == 571 and one(v, 0, 572) is None      # strictly below
    # the nonce is added in the field: seed[word] = p - 3 wraps to 0 at nonce 3
    wrap = [5, 6, 7, P - 3, 9]
    assert M.digest(wrap, 3, 2, 3) == S.perm([5, 6, 7, 0, 9])[2]
    d = M.digests_batch(M.seeds_of([wrap]), 3, 2, [[2, 3, 4]], pb)[0]
    assert d == [S.perm([5, 6, 7, x, 9])[2] for x in (P - 1, 0, 1)]
    # wide nonces: the last 300 of the 64-bit range
    first = (1 << 64) - 300
    want = M.first_hit(SEED_A, 4, 1, P >> 4, first, 300)
    assert want is not None and one(P >> 4, first, 300) == want
    with pytest.raises(AssertionError):
        M.first_hit(SEED_A, 4, 1, P >> 4, first, 301)                # the range may not leave [0, 2^64)


def test_seeds_of_is_the_memory_format():
    s = M.seeds_of([SEED_A, SEED_B])
    assert s.shape == (2, 5, 4) and s.dtype == np.uint64
    assert [S.from_mont(int_of(w)) for w in s[0]] == SEED_A and [S.from_mont(int_of(w)) for w in s[1]] == SEED_B
    assert M.target_bits(8) == P >> 8
