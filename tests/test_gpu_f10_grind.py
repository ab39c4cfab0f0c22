"""GPU tier, row f10 (beyond SURVEY section 8): batched proof-of-work grinding (hades252_grind) against its model
(tests/grind_model.py, over the C oracle's perm_batch): hits inside the first wave, in a later wave, in a later 256-nonce
stride and twenty strides in (later iterations and later blocks); several hits in one wave; both ends of the nonce
range; the strict 256-bit compare limb by limb; the field wrap of the nonce word and the top of the 64-bit nonce range; every word / out_idx; batches; the launch loop's later
rounds (lowered window, child process); and the composition with the streaming sponge, which verifies a found nonce with
calls the library already had.  Exact everywhere.  Convention: this repository's own, UNPINNED (include/hades252.h)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grind_model as M  # noqa: E402
from cipher_model import int_of, mont_limbs  # noqa: E402
from gpu_common import CAP, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

P, S = M.P, M.S
SEED_A = [1 << 64, 1, 2, 3, 4]
SENTINEL = 0xABCDEF0123456789
TOP = 1 << 64


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def grind_raw(lib, seeds, word, out_idx, target, first, max_n):
    """The C entry point itself, the outputs prefilled: -> list of the nonce, or None where found[j] == 0 (and then the
    sentinel must still stand in nonces[j])."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1, 5, 4)
    n = seeds.shape[0]
    nonces, found = np.full(n, SENTINEL, dtype=np.uint64), np.full(n, 7, dtype=np.uint8)
    tgt = (ctypes.c_uint64 * 4)(*[(target >> (64 * k)) & (TOP - 1) for k in range(4)])
    assert lib.hades252_grind(_p(seeds), n, word, out_idx, tgt, first, max_n, _p(nonces), _p(found)) == 0
    assert set(found.tolist()) <= {0, 1}
    assert all(int(x) == SENTINEL for x, f in zip(nonces, found) if not f), "nonces[j] was written where found[j] == 0"
    return [int(x) if f else None for x, f in zip(nonces, found)]


@pytest.fixture(scope="module")
def seed_a():
    return M.seeds_of([SEED_A])


@pytest.fixture(scope="module")
def digests_a(oracle, seed_a):
    """the model's digests of SEED_A (word 4, out_idx 1) at nonces 0 .. 571: the last one is the first below p >> 10"""
    d = M.digests_batch(seed_a, 4, 1, [list(range(572))], oracle.perm_batch)[0]
    assert d[571] < P >> 10 and min(d[:571]) >= P >> 10
    return d


def _first_below(digests, target, first=0):
    return next((x for x in range(first, len(digests)) if digests[x] < target), None)


@pytest.mark.parametrize("bits,want", [(4, 6), (8, 105), (10, 571), (12, 5003)])
def test_wave_and_block_boundaries(hades_lib, H, oracle, seed_a, bits, want):
    """Nonce 6 lies inside wave 0 (with three more hits in the same wave: the minimum of several), 105 in wave 1, 571 in the
    third 256-nonce stride and 5003 in the twentieth: a stride is one iteration of a block, and a block covers
    kGrindIters of them (host_grind.hpp; 1 as shipped: block 2 and block 19).  With the window lowered to 256
    (test_later_rounds_with_lowered_window) every stride is a launch of its own."""
    assert M.first_hit_batch(seed_a, 4, 1, P >> bits, 0, 1 << 16, oracle.perm_batch) == [want]
    assert grind_raw(hades_lib, seed_a, 4, 1, P >> bits, 0, 1 << 16) == [want]
    nonces, found = H.grind(seed_a, 4, 1, H.grind_target(bits), max_nonces=1 << 16)
    assert found.tolist() == [True] and nonces.tolist() == [want] and nonces.dtype == np.uint64


@pytest.mark.parametrize("bits,first,max_n,want", [(10, 0, 571, None), (10, 0, 572, 571), (4, 7, 100, 18), (4, 18, 1, 18),
                                                   (4, 19, 1, None), (10, 572, 2000, 594)])
def test_range_ends(hades_lib, oracle, seed_a, bits, first, max_n, want):
    assert M.first_hit_batch(seed_a, 4, 1, P >> bits, first, max_n, oracle.perm_batch) == [want]
    assert grind_raw(hades_lib, seed_a, 4, 1, P >> bits, first, max_n) == [want]


def test_strict_compare_limb_by_limb(hades_lib, seed_a, digests_a):
    v = digests_a[571]
    assert grind_raw(hades_lib, seed_a, 4, 1, v + 1, 0, 572) == [571]
    assert grind_raw(hades_lib, seed_a, 4, 1, v, 0, 572) == [_first_below(digests_a, v)] == [None]
    seen = set()
    for k in range(8):
        for t in (v + (1 << (32 * k)), v - (1 << (32 * k))):
            if 0 <= t < 1 << 256:
                want = _first_below(digests_a, t)
                seen.add(want)
                assert grind_raw(hades_lib, seed_a, 4, 1, t, 0, 572) == [want], (k, t > v)
    assert {571, None} <= seen                                   # the targets just above and just below v were both there
    assert grind_raw(hades_lib, seed_a, 4, 1, 0, 0, 4096) == [None]
    for first in (0, 5, TOP - 1):
        assert grind_raw(hades_lib, seed_a, 4, 1, P, first, 1) == [first]
        assert grind_raw(hades_lib, seed_a, 4, 1, (1 << 256) - 1, first, 1) == [first]
    assert grind_raw(hades_lib, seed_a, 4, 1, P, 1000, 1 << 20) == [1000]


def test_field_wrap_and_wide_nonces(hades_lib, oracle):
    pb = oracle.perm_batch
    wrap = M.seeds_of([[5, 6, 7, P - 3, 9]])                      # nonce 3 makes word 3 zero
    d = M.digests_batch(wrap, 3, 2, [list(range(8))], pb)[0]
    assert d[3] == S.perm([5, 6, 7, 0, 9])[2]
    for x in range(8):                                            # each nonce around the wrap is the first hit of some target
        t = d[x] + 1
        assert grind_raw(hades_lib, wrap, 3, 2, t, 0, 8) == [_first_below(d, t)]
        assert grind_raw(hades_lib, wrap, 3, 2, t, x, 1) == [x] and grind_raw(hades_lib, wrap, 3, 2, d[x], x, 1) == [None]
    assert grind_raw(hades_lib, wrap, 3, 2, P >> 4, 0, 1024) == M.first_hit_batch(wrap, 3, 2, P >> 4, 0, 1024, pb)
    # the last 300 nonces of the 64-bit range: the nonce's upper word reaches the Montgomery product, the range does not wrap
    seeds = M.seeds_of([[1 << 64, j, 2, 3, 4] for j in range(3)])
    first = TOP - 300
    want = M.first_hit_batch(seeds, 4, 1, P >> 4, first, 300, pb)
    assert all(w is not None and w >= first for w in want)
    assert grind_raw(hades_lib, seeds, 4, 1, P >> 4, first, 300) == want
    last = M.digests_batch(seeds[:1], 4, 1, [[TOP - 1]], pb)[0][0]                # ... and its very last nonce, alone
    assert grind_raw(hades_lib, seeds[:1], 4, 1, last + 1, TOP - 1, 1) == [TOP - 1]
    assert grind_raw(hades_lib, seeds[:1], 4, 1, last, TOP - 1, 1) == [None]
    # a nonce with both halves set, far from either end
    mid = 0x123456789ABCDEF0
    assert grind_raw(hades_lib, seeds, 4, 1, P >> 4, mid, 300) == M.first_hit_batch(seeds, 4, 1, P >> 4, mid, 300, pb)


def test_every_word_and_out_idx(hades_lib, oracle):
    seeds = M.seeds_of([[11, 22, 33, 44, 55], [P - 1, 0, 1 << 200, 7, P - 2]])
    answers = set()
    for word in range(5):
        for out_idx in range(5):
            want = M.first_hit_batch(seeds, word, out_idx, P >> 4, 0, 1024, oracle.perm_batch)
            assert grind_raw(hades_lib, seeds, word, out_idx, P >> 4, 0, 1024) == want, (word, out_idx)
            answers.add(tuple(want))
    assert len(answers) > 20                                      # the 25 searches are different searches


@pytest.mark.parametrize("n_jobs", [1, 2, 300])
def test_batches(hades_lib, H, oracle, n_jobs):
    seeds = M.seeds_of([[1 << 64, j, 2, 3, 4] for j in range(n_jobs)])
    want = M.first_hit_batch(seeds, 4, 1, P >> 6, 0, 1024, oracle.perm_batch)
    assert grind_raw(hades_lib, seeds, 4, 1, P >> 6, 0, 1024) == want
    nonces, found = H.grind(seeds, 4, 1, P >> 6, max_nonces=1024)
    assert found.tolist() == [w is not None for w in want]
    assert [int(x) for x, f in zip(nonces, found) if f] == [w for w in want if w is not None]
    if n_jobs == 300:
        assert len(set(want)) > 50                                # the jobs are different searches
        # a range so short that many jobs have no hit in it: found and not found side by side in one launch
        short = M.first_hit_batch(seeds, 4, 1, P >> 6, 0, 40, oracle.perm_batch)
        assert 50 < sum(w is None for w in short) < 250
        assert grind_raw(hades_lib, seeds, 4, 1, P >> 6, 0, 40) == short


_LATER_ROUNDS_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
from hades252_amd import build, strategy as H
import grind_model as M
build.build(verbose=False)
assert os.environ["HADES252_TEST_GRIND_WINDOW"] == "256"
out = {}
one = M.seeds_of([[1 << 64, 1, 2, 3, 4]])
nonces, found = H.grind(one, 4, 1, M.P >> 12, max_nonces=1 << 16)
out["one"] = [int(x) if f else None for x, f in zip(nonces, found)]
nonces, found = H.grind(one, 4, 1, M.P >> 12, first_nonce=100, max_nonces=4903)      # exhausted in its twentieth round
out["exhausted"] = [int(x) if f else None for x, f in zip(nonces, found)]
many = M.seeds_of([[1 << 64, j, 2, 3, 4] for j in range(300)])
nonces, found = H.grind(many, 4, 1, M.P >> 8, max_nonces=2048)
out["many"] = [int(x) if f else None for x, f in zip(nonces, found)]
print("LATER_ROUNDS " + json.dumps(out))
"""


def test_later_rounds_with_lowered_window(torch_cuda, hades_lib, oracle, seed_a):
    """HADES252_TEST_GRIND_WINDOW = 256 (read once by the library, hence a child process): one launch covers 256 nonces of
    every job, so the hit at 5003 lies in round 20, a range that ends just before it runs 20 rounds to exhaustion, and the
    300 jobs at p >> 8 finish in different rounds while the finished ones' blocks return at once."""
    env = dict(os.environ, HADES252_TEST_GRIND_WINDOW="256")
    r = subprocess.run([sys.executable, "-c", _LATER_ROUNDS_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LATER_ROUNDS ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-1500:] + r.stderr[-3000:]
    got = json.loads(lines[0].split(" ", 1)[1])
    pb = oracle.perm_batch
    assert got["one"] == M.first_hit_batch(seed_a, 4, 1, P >> 12, 0, 1 << 16, pb) == [5003] and 5003 // 256 == 19
    assert got["exhausted"] == M.first_hit_batch(seed_a, 4, 1, P >> 12, 100, 4903, pb) == [None]
    many = M.seeds_of([[1 << 64, j, 2, 3, 4] for j in range(300)])
    want = M.first_hit_batch(many, 4, 1, P >> 8, 0, 2048, pb)
    assert got["many"] == want
    assert len({w // 256 for w in want if w is not None}) >= 4    # they did finish in different rounds


def test_composition_with_the_streaming_sponge(torch_cuda, hades_lib, H, oracle):
    """The seed is a resident sponge state; a found nonce is verified by absorbing it into rate word 4 and squeezing word 1."""
    torch = torch_cuda
    n, target = 3, P >> 8
    sp = H.SpongeStates(n, CAP)
    sp.absorb(to_dev(torch, oracle.gen_b(4242, n * 4).reshape(n, 1, 4, 4)))
    seeds = sp.states.cpu().numpy().view(np.uint64).reshape(n, 5, 4).copy()
    want = M.first_hit_batch(seeds, 4, 1, target, 0, 4096, oracle.perm_batch)
    assert all(w is not None for w in want)
    nonces, found = H.grind(seeds, 4, 1, target, max_nonces=4096)
    assert found.all() and nonces.tolist() == want

    def squeezed_after(xs):
        again = H.SpongeStates(n, CAP)
        again.states.copy_(sp.states)
        block = np.zeros((n, 1, 4, 4), dtype=np.uint64)
        for j, x in enumerate(xs):
            block[j, 0, 3] = mont_limbs(x)
        again.absorb(to_dev(torch, block))
        out = again.squeeze(1).cpu().numpy().view(np.uint64).reshape(n, 4)
        return [S.from_mont(int_of(w)) for w in out]

    assert all(d < target for d in squeezed_after(want))
    before = squeezed_after([max(w - 1, 0) for w in want])
    assert all(d >= target for d, w in zip(before, want) if w > 0)
