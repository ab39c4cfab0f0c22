"""GPU tier, the device half of tests/test_fast_model.py: every field routine of the shipped headers, driven on its own
(tests/units/arith_units.hip: one kernel per routine, built from the unchanged headers with the product's flags) and
compared with its Python model limb for limb, with the big-integer truth mod p, and with the output contract its header
comment states.

The inputs are the model tests' own adversarial operands (imported from test_fast_model, so the two cannot drift apart),
a few thousand random in-contract operands from fixed seeds, and waves that mix them: waves where every lane is an
extreme, and waves of random lanes with extremes in lanes 0, 31, 32 and 63 (rows 0 and 3 for the lane routines), so that
both uniform and divergent selects run.  For every conditional subtraction the model's count of inputs on each side is
asserted non-zero: a rare side cannot silently go unrun.

Caveat: a wrapper compiles a routine in another inlining context than the kernels do; this checks the source's semantics
on the hardware, the end-to-end tests check the kernels' own instruction streams."""
import functools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import units_lib  # noqa: E402
from gpu_common import _record, word_boundary_values  # noqa: E402
from hades252_amd import _derive as D  # noqa: E402
import test_fast_model as M  # noqa: E402
from test_fast_model import (mont_fips, mont_lin, small_mds, mds_row_cols, add_lazy, finalize32_model,  # noqa: E402
                             finalize1_model, lane_mont_mul, lane_lin, lane_sbox, lane_mds_row, carry_split, sbox, val,
                             normalised, far_limbs, steered_rows, mont_lin_factors, lane_lin_factors)

pytestmark = pytest.mark.gpu

P, RP, R = D.P, D.RP, D.R
LB, NL, MASK, LAZY = M.LB, M.NL, M.MASK, M.LAZY
M256 = (1 << 256) - 1
N_RANDOM = 2048
GUARD = 64                     # guard words behind every output buffer
SENTINEL = 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def units(torch_cuda):
    return units_lib.load()


class Out:
    """A device output of `n` elements of `words` 32-bit words, followed by GUARD sentinel words."""

    def __init__(self, torch, n, words):
        self.torch, self.size = torch, n * words
        self.t = torch.full((self.size + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self):
        h = self.t.cpu().numpy()
        assert (h[self.size:] == SENTINEL).all(), "a wrapper wrote behind its output"
        return h[:self.size]


def put(torch, words, dtype=np.int32):
    a = np.ascontiguousarray(words, dtype=dtype)
    return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).cuda()


def call(torch, fn, *args):
    """fn(args..., stream): tensors and Out buffers are passed by device pointer and stay referenced until the launch has
    completed (a pointer taken from a temporary tensor would let the caching allocator hand its block to the next one)."""
    ptrs = [a.data_ptr() if isinstance(a, (torch.Tensor, Out)) else a for a in args]
    rc = fn(*ptrs, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, "launch failed (%d)" % rc
    torch.cuda.synchronize()


def f29_words(xs):
    return [l for x in xs for l in x]


def fr_words(vals):
    return [(v >> (32 * k)) & 0xFFFFFFFF for v in vals for k in range(8)]


def f29_of(h):
    return [list(map(int, r)) for r in h.reshape(-1, NL)]


def fr_of(h):
    h = h.astype(np.int64) & 0xFFFFFFFF
    return [sum(int(w) << (32 * k) for k, w in enumerate(r)) for r in h.reshape(-1, 8)]


def unary29(torch, fn, xs, out_words):
    """xs: list of F29 limb lists -> device output (F29 rows or Fr integers)."""
    o = Out(torch, len(xs), out_words)
    a = put(torch, f29_words(xs))
    call(torch, fn, a, o, len(xs))
    return o.get()


def waves(extremes, randoms, per_wave=64, slots=(0, 31, 32, 63)):
    """Uniform waves (every element an extreme, cycled to whole waves), mixed waves (random elements with extremes in
    `slots`, every extreme placed at least once) and then the random elements."""
    assert extremes and len(randoms) >= per_wave
    n_uni = -(-len(extremes) // per_wave) * per_wave
    out = [extremes[i % len(extremes)] for i in range(n_uni)]
    n_mix = -(-len(extremes) // len(slots))
    for w in range(n_mix):
        wave = [randoms[(w * per_wave + i) % len(randoms)] for i in range(per_wave)]
        for s, slot in enumerate(slots):
            wave[slot] = extremes[(w * len(slots) + s) % len(extremes)]
        out += wave
    return out + list(randoms)


def row_waves(extremes, randoms):
    return waves(extremes, randoms, per_wave=4, slots=(0, 3))


def both_sides(name, counts):
    """Every side of a select was taken by at least one input (the counts come from the model / the big-integer truth)."""
    assert all(c > 0 for c in counts.values()), "%s: a side was never taken: %s" % (name, counts)
    _record("units_coverage.txt", "%s: %s" % (name, counts))


def driven(name, n):
    _record("units_coverage.txt", "%s: %d inputs" % (name, n))


# ---------------------------------------------------------------------------------------------------------------------
# operand generators (in-contract, fixed seeds)
# ---------------------------------------------------------------------------------------------------------------------
def signed_limbs(v):
    """normalised limbs 0..7, signed top limb"""
    return [(v >> (LB * k)) & MASK for k in range(NL - 1)] + [v >> (LB * (NL - 1))]


def lazy_operand(rng):
    """What an S-box receives: a normalised value of a product's range plus a balanced round constant."""
    x = signed_limbs(rng.randrange(-P - (1 << 253) + 1, 1 << 253))
    return [a + b for a, b in zip(x, D.to_balanced29(rng.randrange(P)))]


def product_operand(rng):
    k = rng.randrange(3)
    if k == 0:
        return lazy_operand(rng)
    if k == 1:
        return signed_limbs(rng.randrange(-P - (1 << 253) + 1, 1 << 253))
    return [rng.randrange(-LAZY + 1, LAZY) for _ in range(NL - 1)] + [rng.randrange(-(1 << 24), 1 << 24)]


def normalised_operand(rng):
    """mont_lin's contract: limbs 0..7 in [0, 2^29), |top limb| < 2^25."""
    if rng.random() < 0.5:
        return [rng.randrange(1 << LB) for _ in range(NL - 1)] + [rng.randrange(-(1 << 25) + 1, 1 << 25)]
    return signed_limbs(rng.randrange(-P - (1 << 253) + 1, 1 << 253))


def lane_row(limbs):
    return list(limbs) + [0] * 7


def lane_operand(rng):
    if rng.random() < 0.5:
        return lane_row([rng.randrange(M.LANE_IN_MAX + 1) for _ in range(NL - 1)] + [rng.randrange(M.LANE_TOP)])
    return lane_row(D.to_limbs29(rng.randrange(P)))


def lin_table(factor, steps):
    e = D.lin_table(factor, steps)
    return e + [0] * (D.LIN_ROW - len(e))


# ---------------------------------------------------------------------------------------------------------------------
# hades_fast.hpp
# ---------------------------------------------------------------------------------------------------------------------
def test_to_from_f29_round_trip(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(101)
    ext = [0, 1, P - 1, P, P + 1, M256, 1 << 255, (1 << 232) - 1, 1 << 232, (1 << 29) - 1] + \
          [((1 << (32 * k)) - 1) for k in range(1, 8)] + [1 << (29 * k) for k in range(9)]
    vals = waves(ext, [rng.getrandbits(256) for _ in range(N_RANDOM)])
    limbs = f29_of(_to_f29(torch, units, vals))
    for v, l in zip(vals, limbs):
        assert l == [(v >> (LB * k)) & MASK for k in range(NL)]
    back = fr_of(unary29(torch, units.units_from_f29, limbs, 8))
    assert back == vals
    driven("to_f29 / from_f29", len(vals))


def _to_f29(torch, units, vals):
    o = Out(torch, len(vals), NL)
    call(torch, units.units_to_f29, put(torch, fr_words(vals), np.uint32), o, len(vals))
    return o.get()


def check_product(a, b, r):
    """The header's contract of mont_fips: normalised, in (ab/Rp - p, ab/Rp], (-p - 2^253, 2^253), == ab/Rp mod p."""
    v, ab = val(r), val(a) * val(b)
    assert all(0 <= x < (1 << LB) for x in r[:-1])
    assert ab - P * RP < v * RP <= ab and -P - (1 << 253) < v < (1 << 253)
    assert (v - ab * pow(RP, -1, P)) % P == 0


@pytest.mark.parametrize("sqr", [False, True], ids=["mul", "sqr"])
def test_mont_fips_vs_model(torch_cuda, units, sqr):
    torch = torch_cuda
    rng = random.Random(103 + sqr)
    ext = M.PRODUCT_PATTERNS + [[LAZY - 1] * (NL - 1) + [-(1 << 24)],
                                [-(LAZY - 1)] * (NL - 1) + [(1 << 24) - 1], [0] * NL, [1] + [0] * (NL - 1),
                                signed_limbs(-P - (1 << 253) + 1), signed_limbs((1 << 253) - 1)]
    a = waves(ext, [product_operand(rng) for _ in range(N_RANDOM)])
    if sqr:
        b = a
        got = f29_of(unary29(torch, units.units_mont_sqr, a, NL))
    else:
        b = waves(list(reversed(ext)), [product_operand(rng) for _ in range(N_RANDOM)])
        o = Out(torch, len(a), NL)
        call(torch, units.units_mont_mul, put(torch, f29_words(a)), put(torch, f29_words(b)),
             o, len(a))
        got = f29_of(o.get())
    for x, y, r in zip(a, b, got):
        assert r == mont_fips(x, y, sqr), (x, y)
        check_product(x, y, r)
    driven("mont_fips<%s>" % ("true" if sqr else "false"), len(a))


def test_mont_mul_const_and_small_vs_model(torch_cuda, units):
    """mont_fips<false, true> with a wave-uniform constant; mont_mul_small(a, c) == mont_fips(a, (c, 0, ..., 0)) limb for
    limb (the product columns of the two are the same sums)."""
    torch = torch_cuda
    rng = random.Random(107)
    ext = M.PRODUCT_PATTERNS + [[0] * NL, signed_limbs(-P - (1 << 253) + 1), signed_limbs((1 << 253) - 1)]
    a = waves(ext, [product_operand(rng) for _ in range(N_RANDOM)])
    for c in (D.to_limbs29(D.RP * D.R % P), D.to_limbs29(P - 1), M.PRODUCT_PATTERNS[1]):
        o = Out(torch, len(a), NL)
        call(torch, units.units_mont_mul_const, put(torch, f29_words(a)), put(torch, c), o,
             len(a))
        for x, r in zip(a, f29_of(o.get())):
            assert r == mont_fips(x, c)
            check_product(x, c, r)
    cs = [0, 1, 32, MASK, MASK - 1] * 2
    cs = (cs * (len(a) // len(cs) + 1))[:len(a) - N_RANDOM] + [rng.randrange(1 << LB) for _ in range(N_RANDOM)]
    o = Out(torch, len(a), NL)
    call(torch, units.units_mont_mul_small, put(torch, f29_words(a)), put(torch, cs), o, len(a))
    for x, c, r in zip(a, cs, f29_of(o.get())):
        b = [c] + [0] * (NL - 1)
        assert r == mont_fips(x, b), "mont_mul_small differs from mont_fips(a, (c, 0, ..., 0))"
        check_product(x, b, r)
    driven("mont_fips<false, true>", 3 * len(a))
    driven("mont_mul_small", len(a))


@pytest.mark.parametrize("steps", [2, 1], ids=["mont_lin", "mont_lin1"])
def test_mont_lin_vs_model(torch_cuda, units, steps, monkeypatch):
    torch = torch_cuda
    # the model rebuilds its table on every call (milliseconds of modular powers): the same table, built once per factor
    monkeypatch.setattr(D, "lin_table", functools.lru_cache(maxsize=None)(D.lin_table))
    rng = random.Random(109 + steps)
    ext = M.MONT_LIN_OPERANDS + [[0] * NL, [MASK] * (NL - 1) + [-1], [0] * (NL - 1) + [-((1 << 25) - 1)],
                                 D.to_limbs29(P - 1), signed_limbs(-P - (1 << 253) + 1)]
    a = waves(ext, [normalised_operand(rng) for _ in range(N_RANDOM)])
    fn = units.units_mont_lin if steps == 2 else units.units_mont_lin1
    n = 0
    for factor in mont_lin_factors():
        o = Out(torch, len(a), NL)
        call(torch, fn, put(torch, f29_words(a)), put(torch, lin_table(factor, steps)), o,
             len(a))
        for x, r in zip(a, f29_of(o.get())):
            assert r == mont_lin(x, factor, steps), (x, factor)
            v = val(r)
            assert all(0 <= l < (1 << LB) for l in r[:-1])
            assert (v - val(x) * factor * pow(RP, -1, P)) % P == 0
            if steps == 2:
                assert -P - (1 << 227) < v < (1 << 230)                 # the header's window
            else:
                assert abs(r[-1]) < (1 << 26) and -P - (1 << 251) < v < 9 * P
        n += len(a)
    driven("mont_lin" if steps == 2 else "mont_lin1", n)


def test_sbox29_and_add_lazy_vs_model(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(113)
    ext = M.PRODUCT_PATTERNS + [[0] * NL, [1] + [0] * (NL - 1)]
    a = waves(ext, [lazy_operand(rng) for _ in range(N_RANDOM)])
    got = f29_of(unary29(torch, units.units_sbox29, a, NL))
    for x, r in zip(a, got):
        assert r == sbox(x)
        assert normalised(r) and -P - (1 << 253) < val(r) < (1 << 253)
        assert (val(r) - pow(val(x), 5, P) * pow(RP, -4, P)) % P == 0
    driven("sbox29", len(a))
    # add_lazy: a normalised word (a product's or the linear layer's output) + balanced round-constant limbs
    xs = waves([M.MONT_LIN1_NEIGHBOUR, [0] * NL, signed_limbs(-P - (1 << 253) + 1), [MASK] * (NL - 1) + [(1 << 24) - 1]],
               [signed_limbs(rng.randrange(-P - (1 << 253) + 1, 1 << 253)) for _ in range(N_RANDOM)])
    cs = [D.to_balanced29(v) for v in ([P - 1, 0, (1 << 254) + 12345, P >> 1] * len(xs))[:len(xs) - N_RANDOM]] + \
         [D.to_balanced29(rng.randrange(P)) for _ in range(N_RANDOM)]
    cs = [[-(1 << 28)] * (NL - 1) + [0] if i % 97 == 5 else c for i, c in enumerate(cs)]    # the balanced limbs' floor
    o = Out(torch, len(xs), NL)
    call(torch, units.units_add_lazy, put(torch, f29_words(xs)), put(torch, f29_words(cs)), o,
         len(xs))
    for x, c, r in zip(xs, cs, f29_of(o.get())):
        assert r == add_lazy(x, c) and val(r) == val(x) + val(c)
    driven("add_lazy", len(xs))


def test_small_mds_vs_model(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(127)
    big = M.MONT_LIN1_NEIGHBOUR
    r1 = mont_lin(M.MONT_LIN_OPERANDS[0], mont_lin_factors()[3], 1)          # a mont_lin1 result as word 4
    ext = M.LINEAR_LAYER_STATES + [[big, big, big, big, r1], [[0] * NL] * 5]
    sts = waves(ext, [[product_operand(rng) for _ in range(5)] for _ in range(N_RANDOM)])
    o = Out(torch, len(sts), 5 * NL)
    call(torch, units.units_small_mds, put(torch, [l for st in sts for l in f29_words(st)]), o, len(sts))
    got = o.get().reshape(-1, 5, NL)
    for st, g in zip(sts, got):
        rows = [list(map(int, r)) for r in g]
        assert rows == small_mds(st)
        for i in range(5):
            y = sum(D.MDS_SMALL[i][j] * val(st[j]) for j in range(5))
            assert normalised(rows[i]) and (val(rows[i]) - y * pow(1 << LB, -1, P)) % P == 0
    driven("small_mds", len(sts))


def finalize_sides(v):
    """finalize: + 2p, then two conditional subtractions; returns how many were taken"""
    t = v + 2 * P
    return (t >= P) + (t >= 2 * P)


def test_finalize_both_ends_and_every_number_of_subtractions(torch_cuda, units):
    """finalize: x in (-p - 2^250, 2^250] with normalised limbs -> x mod p; finalize1: x in (-p, p) -> x mod p.  Both
    ends of each window, and every number of conditional subtractions (0, 1, 2 / 0, 1) taken."""
    torch = torch_cuda
    rng = random.Random(131)
    lo = -P - (1 << 250) + 1
    ext = [lo, lo + 1, -P - 1, -P, -P + 1, -1, 0, 1, P - 1 if P - 1 <= (1 << 250) else (1 << 250), (1 << 250) - 1,
           1 << 250, -2, -(P >> 1)]
    rnd = [rng.randrange(lo, (1 << 250) + 1) if i % 4 else rng.randrange(-P, 0) for i in range(N_RANDOM)]
    vals = waves(ext, rnd)
    got = fr_of(unary29(torch, units.units_finalize, [signed_limbs(v) for v in vals], 8))
    sides = {0: 0, 1: 0, 2: 0}
    for v, g in zip(vals, got):
        assert g == v % P, v
        sides[finalize_sides(v)] += 1
    both_sides("finalize (subtractions taken)", sides)
    driven("finalize", len(vals))
    # finalize1
    ext1 = [-P + 1, -P + 2, -1, 0, 1, P - 1, P - 2, -(P >> 1), P >> 1]
    vals = waves(ext1, [rng.randrange(-P + 1, P) for _ in range(N_RANDOM)])
    got = fr_of(unary29(torch, units.units_finalize1, [signed_limbs(v) for v in vals], 8))
    sides = {"kept": 0, "subtracted": 0}
    for v, g in zip(vals, got):
        assert g == finalize1_model(v) == v % P, v
        sides["subtracted" if v >= 0 else "kept"] += 1
    both_sides("finalize1", sides)
    driven("finalize1", len(vals))


# ---------------------------------------------------------------------------------------------------------------------
# kernels_perm.hpp
# ---------------------------------------------------------------------------------------------------------------------
def finalize32_side(x):
    m = ((-x[0]) & 31) + 32
    return ((val(x) + m * P) >> 5) >= P


def test_finalize32_vs_model(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(137)
    ext = [D.to_balanced29_signed(v) for v in M.FINALIZE32_EDGES]
    ext += [D.to_limbs29(v) for v in M.FINALIZE32_EDGES if 0 <= v < (P >> 3)]
    ext += [far_limbs(v) for v in M.FINALIZE32_FAR]
    for j, vals, u in steered_rows(trials=8):                        # the row path at its worst, constant appended
        row = mds_row_cols(u, j, 5)
        ext += [add_lazy(row, D.to_balanced29_signed(c)) if c else row for c in M.ROW_CONSTANTS]
    rnd = []
    for i in range(N_RANDOM):
        if i % 2:
            rnd.append(D.to_balanced29_signed(rng.randrange(-2 * P, P >> 3)))
        else:                                                        # lazy: a normalised value + a balanced addend
            a, b = rng.randrange(P >> 4), rng.randrange(P)
            rnd.append([p + q for p, q in zip(D.to_limbs29(a), D.to_balanced29_signed(b - P))])
    xs = waves(ext, rnd)
    got = fr_of(unary29(torch, units.units_finalize32, xs, 8))
    sides = {"kept": 0, "subtracted": 0}
    inv32 = pow(32, -1, P)
    for x, g in zip(xs, got):
        assert g == finalize32_model(x) == val(x) * inv32 % P, x
        sides["subtracted" if finalize32_side(x) else "kept"] += 1
    both_sides("finalize32", sides)
    driven("finalize32", len(xs))


@pytest.mark.parametrize("ncol", [3, 5])
def test_mds_row_cols_vs_model(torch_cuda, units, ncol):
    torch = torch_cuda
    rng = random.Random(139 + ncol)
    by_row = {j: [] for j in range(5)}
    for j, vals, u in steered_rows():
        by_row[j].append(u)
    n = 0
    for j in range(5):
        us = waves(by_row[j], [[product_operand(rng) for _ in range(5)] for _ in range(N_RANDOM // 4)])
        o = Out(torch, len(us), NL)
        call(torch, units.units_mds_row_cols, ncol, put(torch, [l for u in us for l in f29_words(u)]), j,
             o, len(us))
        for u, r in zip(us, f29_of(o.get())):
            assert r == mds_row_cols(u, j, ncol)
            y = sum(D.MDS_SMALL[j][c] * val(u[c]) for c in range(ncol))
            assert val(r) * (1 << LB) == y - (y & MASK) * P
        n += len(us)
    driven("mds_row_cols<%d>" % ncol, n)


# ---------------------------------------------------------------------------------------------------------------------
# fr32.hpp
# ---------------------------------------------------------------------------------------------------------------------
def cios_reduced(a, b):
    """t of fr_mul before its conditional subtraction: (a b + M p) / 2^256, M = -a b / p mod 2^256 (word by word the
    CIOS digits compose to exactly this M)"""
    ab = a * b
    m = (-ab * pow(P, -1, 1 << 256)) % (1 << 256)
    t = (ab + m * P) >> 256
    assert (ab + m * P) % (1 << 256) == 0 and t < 2 * P
    return t


def test_fr_is_canonical_word_boundaries(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(149)
    bnd = word_boundary_values()
    ext = [v for v, _ in bnd]
    vals = waves(ext, [rng.getrandbits(256) if i % 2 else rng.randrange(P) for i in range(N_RANDOM)])
    o = Out(torch, len(vals), 1)
    call(torch, units.units_fr_is_canonical, put(torch, fr_words(vals), np.uint32), o, len(vals))
    got = o.get()
    for v, ok in bnd:
        assert (v < P) == ok
    sides = {"canonical": 0, "not canonical": 0}
    for v, g in zip(vals, got):
        assert int(g) == (1 if v < P else 0), hex(v)
        sides["canonical" if v < P else "not canonical"] += 1
    both_sides("fr_is_canonical", sides)
    driven("fr_is_canonical", len(vals))


def test_fr_cond_sub_p_both_tops(torch_cuda, units):
    """r = A - p if A >= p else A for A = a + top 2^256 < 2^256 + p (the header's bound): top = 0 on both sides of p (the
    word boundaries included), top = 1 (the borrow paid by the 257th bit) with a < p."""
    torch = torch_cuda
    rng = random.Random(151)
    ext = [(v, 0) for v, _ in word_boundary_values() if v < 2 * P] + [(P, 0), (2 * P - 1, 0), (0, 0)]
    ext += [(v, 1) for v in (0, 1, P - 1, P - (1 << 224), (1 << 32) - 1)]
    rnd = [(rng.randrange(2 * P), 0) if i % 3 else (rng.randrange(P), 1) for i in range(N_RANDOM)]
    cases = waves(ext, rnd)
    o = Out(torch, len(cases), 8)
    call(torch, units.units_fr_cond_sub_p, put(torch, fr_words([a for a, _ in cases]), np.uint32),
         put(torch, [t for _, t in cases], np.uint32), o, len(cases))
    sides = {"kept": 0, "subtracted": 0, "subtracted (top)": 0}
    for (a, top), g in zip(cases, fr_of(o.get())):
        full = a + (top << 256)
        assert full < (1 << 256) + P
        assert g == (full - P if full >= P else full), (hex(a), top)
        sides["subtracted (top)" if top else ("subtracted" if a >= P else "kept")] += 1
    both_sides("fr_cond_sub_p", sides)
    driven("fr_cond_sub_p", len(cases))


def add_pairs():
    """a + b at p - 1, p, p + 1 and 2p - 2, and 0 + 0"""
    out = [(0, 0), (P - 1, P - 1)]
    for s in (P - 1, P, P + 1):
        for a in (0, 1, s // 2, P - 1, (1 << 32) - 1, s - (P - 1)):
            if 0 <= a < P and 0 <= s - a < P:
                out.append((a, s - a))
    return out


def mul_pairs():
    """a b / R = 0, one (R) and p - 1: a a^-1 and its negation, in Montgomery form"""
    rng = random.Random(157)
    out = [(0, 0), (0, P - 1), (P - 1, 0), (R, R), (R, P - R)]
    for _ in range(6):
        x = rng.randrange(1, P)
        xm, xinv = x * R % P, pow(x, -1, P) * R % P
        out += [(xm, xinv), (xm, P - xinv), (P - xm, xinv)]
    return out


def test_fr_add_and_mul_vs_truth(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(163)
    pairs = waves(add_pairs(), [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)])
    o = Out(torch, len(pairs), 8)
    call(torch, units.units_fr_add, put(torch, fr_words([a for a, _ in pairs]), np.uint32),
         put(torch, fr_words([b for _, b in pairs]), np.uint32), o, len(pairs))
    sides = {"kept": 0, "subtracted": 0}
    for (a, b), g in zip(pairs, fr_of(o.get())):
        assert g == (a + b) % P, (a, b)
        sides["subtracted" if a + b >= P else "kept"] += 1
    both_sides("fr_add", sides)
    driven("fr_add", len(pairs))
    pairs = waves(mul_pairs() + [(P - 1, P - 1), (1, 1), (P - 1, 1)],
                  [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)])
    o = Out(torch, len(pairs), 8)
    call(torch, units.units_fr_mul, put(torch, fr_words([a for a, _ in pairs]), np.uint32),
         put(torch, fr_words([b for _, b in pairs]), np.uint32), o, len(pairs))
    sides = {"kept": 0, "subtracted": 0}
    rinv = pow(R, -1, P)
    for (a, b), g in zip(pairs, fr_of(o.get())):
        assert g == a * b * rinv % P, (a, b)
        sides["subtracted" if cios_reduced(a, b) >= P else "kept"] += 1
    both_sides("fr_mul", sides)
    driven("fr_mul", len(pairs))


# ---------------------------------------------------------------------------------------------------------------------
# hades_lanes.hpp: one element per 16-lane row
# ---------------------------------------------------------------------------------------------------------------------
def lane_rows_of(h):
    return [list(map(int, r)) for r in (h.astype(np.int64) & 0xFFFFFFFF).reshape(-1, 16)]


def check_lane_result(r, ab_over_rp):
    assert all(x <= M.LANE_IN_MAX for x in r) and r[NL - 1] < (1 << 26) and all(x == 0 for x in r[NL:])
    assert M.lane_val(r) < ab_over_rp + 2 * P + (P >> 20)


def test_lane_mont_mul_and_sbox_vs_model(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(167)
    pats = [lane_row(p) for p in M.LANE_PATTERNS]
    a = row_waves(pats, [lane_operand(rng) for _ in range(N_RANDOM // 2)])
    b = row_waves(list(reversed(pats)) + pats[:3], [lane_operand(rng) for _ in range(N_RANDOM // 2)])
    b = (b * 2)[:len(a)]
    # every pair of the model test's patterns as well
    a += [x for x in pats for _ in pats]
    b += [y for _ in pats for y in pats]
    o = Out(torch, len(a), 16)
    call(torch, units.units_lane_mont_mul, put(torch, [l for r in a for l in r], np.uint32),
         put(torch, [l for r in b for l in r], np.uint32), o, len(a))
    for x, y, r in zip(a, b, lane_rows_of(o.get())):
        assert r == lane_mont_mul(x, y), (x, y)
        ab = M.lane_val(x) * M.lane_val(y)
        assert (M.lane_val(r) - ab * pow(RP, -1, P)) % P == 0
        check_lane_result(r, ab // RP)
    driven("lane_mont_mul", len(a))
    # the S-box: what a row holds after a round key (plain limbs: a reduced value + a reduced constant)
    xs = row_waves([lane_row(D.to_limbs29(v)) for v in (0, 1, P - 1)] +
                   [lane_row([x + y for x, y in zip(D.to_limbs29(P - 1), D.to_limbs29(P - 1))]), pats[1]],
                   [lane_row([x + y for x, y in zip(D.to_limbs29(rng.randrange(P)), D.to_limbs29(rng.randrange(P)))])
                    for _ in range(N_RANDOM // 4)])
    o = Out(torch, len(xs), 16)
    call(torch, units.units_lane_sbox, put(torch, [l for r in xs for l in r], np.uint32), o, len(xs))
    for x, r in zip(xs, lane_rows_of(o.get())):
        assert r == lane_sbox(x)
        assert (M.lane_val(r) - pow(M.lane_val(x), 5, P) * pow(RP, -4, P)) % P == 0
        assert all(v <= M.LANE_IN_MAX for v in r) and r[NL - 1] < (1 << 26)
    driven("lane_sbox", len(xs))


def test_lane_lin_vs_model(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(173)
    pats = [lane_row(p) for p in M.LANE_PATTERNS]
    a = row_waves(pats, [lane_operand(rng) for _ in range(N_RANDOM // 4)])
    n = 0
    for factor in lane_lin_factors():
        e = [D.to_limbs29(factor * pow(2, LB * (k + D.LIN_STEPS - NL), P) % P) + [0] * 7 for k in range(NL)]
        o = Out(torch, len(a), 16)
        call(torch, units.units_lane_lin, put(torch, [l for r in a for l in r], np.uint32),
             put(torch, [l for r in e for l in r], np.uint32), o, len(a))
        for x, r in zip(a, lane_rows_of(o.get())):
            assert r == lane_lin(x, factor), (x, factor)
            w = M.lane_val(x) * factor
            assert (M.lane_val(r) - w * pow(RP, -1, P)) % P == 0
            assert all(v <= M.LANE_IN_MAX for v in r) and r[NL - 1] < (1 << 26) and all(v == 0 for v in r[NL:])
        n += len(a)
    driven("lane_lin", n)


def test_lane_mds_row_vs_model(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(179)
    pats = [lane_row(p) for p in M.LANE_PATTERNS]
    ext = [[M.LANE_MDS_BIG] * 5, [pats[0]] * 5, [pats[2]] * 5, [M.LANE_MDS_BIG, pats[0], pats[2], M.LANE_MDS_BIG, pats[6]]]
    xs = row_waves(ext, [[lane_operand(rng) for _ in range(5)] for _ in range(N_RANDOM // 4)])
    n = 0
    for j in range(5):
        o = Out(torch, len(xs), 16)
        call(torch, units.units_lane_mds_row, put(torch, [l for x in xs for r in x for l in r], np.uint32), j,
             o, len(xs))
        for x, r in zip(xs, lane_rows_of(o.get())):
            assert r == lane_mds_row(D.MDS_SMALL[j], x)
            y = sum(D.MDS_SMALL[j][c] * M.lane_val(x[c]) for c in range(5))
            assert (M.lane_val(r) - y * pow(1 << LB, -1, P)) % P == 0
            assert all(v <= (1 << LB) + 2 for v in r) and r[NL - 1] < (1 << 24) and all(v == 0 for v in r[NL:])
        n += len(xs)
    driven("lane_mds_row", n)


def product_columns(a, b):
    """T = a b column by column (lane k: sum_i a_i b_{k-i}): what carry_split receives first in lane_mont_mul"""
    return [sum(a[i] * b[k - i] for i in range(NL) if 0 <= k - i < NL) for k in range(16)]


def test_carry_split_vs_model(torch_cuda, units):
    torch = torch_cuda
    rng = random.Random(181)
    pats = [lane_row(p) for p in M.LANE_PATTERNS]
    ext = [product_columns(x, y) for x in pats for y in pats] + [[(1 << 64) - 1] * 16, [0] * 16, [(1 << 58) - 1] * 16,
                                                                 [1 << 58] * 16]
    accs = row_waves(ext, [[rng.getrandbits(64) for _ in range(16)] if i % 2 else
                           product_columns(lane_operand(rng), lane_operand(rng)) for i in range(N_RANDOM // 4)])
    n = len(accs)
    outs = [Out(torch, n, 16) for _ in range(3)]
    call(torch, units.units_carry_split, put(torch, [v for r in accs for v in r], np.uint64),
         *outs, n)
    t, c16, c17 = (lane_rows_of(o.get()) for o in outs)
    for k, acc in enumerate(accs):
        mt, mu, mtp = carry_split(acc)
        assert (t[k], c16[k], c17[k]) == (mt, mu, mtp), acc
        assert sum(x << (LB * i) for i, x in enumerate(t[k])) + (mu[15] << (LB * 16)) + (mtp[15] << (LB * 17)) == \
            sum(x << (LB * i) for i, x in enumerate(acc))                   # the carry step keeps the row's value
    driven("carry_split", n)


def test_dpp_moves_vs_model(torch_cuda, units):
    """The data moves every lane routine is made of, on their own: row_shr / row_shl<1..15>, row_bcast<0..15>,
    wave_bcast_row<0 / 1> and the two raw half-exchanges with two different operands, on lane-distinct non-zero values
    (a zero can then only be a shift's fill), two waves.  tests/test_hostsim_units.py holds the host build's emulation of
    these builtins to the same model."""
    torch = torch_cuda
    n = 2
    a = [0x1000_0000 * (w + 1) + 0x0101 * (lane + 1) for w in range(n) for lane in range(64)]
    b = [0xB000_0000 + 0x0100_0000 * w + 0x0307 * (lane + 1) for w in range(n) for lane in range(64)]
    assert len(set(a + b)) == 2 * 64 * n and 0 not in a + b
    o = Out(torch, n, 64 * 52)
    call(torch, units.units_dpp_moves, put(torch, a, np.uint32), put(torch, b, np.uint32), o, n)
    got = (o.get().astype(np.int64) & 0xFFFFFFFF).reshape(n, 52, 64)
    for w in range(n):
        va, vb = a[64 * w:64 * w + 64], b[64 * w:64 * w + 64]
        rows = [va[16 * r:16 * r + 16] for r in range(4)]
        exp = [sum((M.row_shr(r, s) for r in rows), []) for s in range(1, 16)]
        exp += [sum((M.row_shl(r, s) for r in rows), []) for s in range(1, 16)]
        exp += [sum((M.row_bcast(r, s) for r in rows), []) for s in range(16)]
        exp += [M.wave_bcast_row(va, 0), M.wave_bcast_row(va, 1)]
        exp += list(M.permlane_swap(va, vb, 16)) + list(M.permlane_swap(va, vb, 32))
        assert len(exp) == 52
        for j, e in enumerate(exp):
            assert list(map(int, got[w, j])) == e, (w, j)
    driven("row_shr / row_shl / row_bcast / wave_bcast_row / permlane swaps", 52 * n)
