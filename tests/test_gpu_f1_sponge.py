"""GPU tier, SURVEY section 8 row f1: the sponge hash over the batched permutation (fixed and variable length, device-side
sort by block count, streaming absorb / squeeze, the one-message-per-wave forms).  Convention (capacity, padding) is a
parameter: dusk-poseidon is outside the reference tree -- UNPINNED."""
import ctypes
import hashlib
import json
import os
import random
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402,F401
from oracle_lib import P, R, limbs_of, int_of, digest_ref  # noqa: E402,F401
from gpu_common import *  # noqa: E402,F401,F403  (helpers shared by the GPU tier; fixtures torch_cuda / H: conftest.py)

pytestmark = pytest.mark.gpu


def test_sponge_hash(torch_cuda, H, oracle):
    """Batched fixed-length sponge over the permutation vs the oracle (convention parameters;
    dusk-poseidon itself is outside the reference tree)."""
    torch = torch_cuda
    cap = S.to_mont(1 << 64)
    for length in (1, 2, 3, 4, 5, 7, 8, 9, 16):
        for pad in (0, 1):
            n = 1000 if length < 9 else 130
            msgs = oracle.gen_b(length * 977 + pad, n * length)
            got = H.sponge_hash(to_dev(torch, msgs), length, cap, pad)
            assert (to_host(got) == oracle.sponge(msgs, length, cap, pad)).all(), (length, pad)
    with pytest.raises(ValueError):
        H.sponge_hash(to_dev(torch, oracle.gen_b(0, 10)), 3, cap, 1)


# ---------------------------------------------------------------------------------------------
# variable-length sponge
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1])
def test_sponge_var_ragged_lengths(torch_cuda, H, oracle, pad):
    """Ragged lengths 0..33 (every residue mod 4, zero-length messages, one long outlier in a wave of
    short ones), shuffled offsets, gaps and overlaps -- vs the oracle, both padding modes."""
    torch = torch_cuda
    rng = random.Random(11 + pad)
    cap = S.to_mont((1 << 64) + 7)
    n = 1000
    lengths = [rng.randrange(0, 34) for _ in range(n)]
    lengths[5] = 0
    lengths[64:128] = [1] * 63 + [33]          # a wave of short messages with one long one
    lengths[300:364] = [0] * 64                # a wave of empty messages
    pool = oracle.gen_b(4242, 40000)
    offsets = [rng.randrange(0, 40000 - 34) for _ in range(n)]      # arbitrary: overlaps and gaps
    got = H.sponge_hash_var(to_dev(torch, pool), to_dev(torch, np.array(offsets, dtype=np.uint64)),
                            to_dev(torch, np.array(lengths, dtype=np.uint64)), cap, pad)
    exp = oracle.sponge_var(pool, offsets, lengths, cap, pad)
    assert (to_host(got) == exp).all()


def test_sponge_var_equals_fixed_and_packed(torch_cuda, H, oracle):
    torch = torch_cuda
    cap = S.to_mont(1 << 64)
    n, length = 777, 6
    msgs = oracle.gen_b(99, n * length)
    fixed = H.sponge_hash(to_dev(torch, msgs), length, cap, 1)
    off = np.arange(n, dtype=np.uint64) * np.uint64(length)
    var = H.sponge_hash_var(to_dev(torch, msgs), to_dev(torch, off), to_dev(torch, np.full(n, length, dtype=np.uint64)),
                            cap, 1)
    assert torch.equal(fixed, var)
    assert (to_host(fixed) == oracle.sponge(msgs, length, cap, 1)).all()
    # packed ragged (CSR-style offsets)
    lens = np.array([(i * 7) % 13 for i in range(500)], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    pool = oracle.gen_b(5, int(lens.sum()) + 1)
    got = H.sponge_hash_var(to_dev(torch, pool), to_dev(torch, offs), to_dev(torch, lens), cap, 1)
    assert (to_host(got) == oracle.sponge_var(pool, offs, lens, cap, 1)).all()
    # a message reaching outside the pool is never read: counted, raised by the mirror
    lens_bad = lens.copy()
    lens_bad[7] = np.uint64(1 << 40)
    with pytest.raises(IndexError):
        H.sponge_hash_var(to_dev(torch, pool), to_dev(torch, offs), to_dev(torch, lens_bad), cap, 1)
    offs_bad = offs.copy()
    offs_bad[9] = np.uint64((1 << 64) - 3)                      # offset + length would wrap around
    with pytest.raises(IndexError):
        H.sponge_hash_var(to_dev(torch, pool), to_dev(torch, offs_bad), to_dev(torch, lens), cap, 1)


@pytest.mark.parametrize("pad", [0, 1])
def test_sponge_sorted_equals_unsorted_and_oracle(torch_cuda, hades_lib, H, oracle, pad):
    """Ragged lengths (0 .. 70 scalars, a few very long, one beyond the last sort bucket): the device-sorted run (above
    COOP_MAX messages, so that the sort runs; guarded digests, zero-filled scratch) gives the same digests in message
    order as the plain run and the oracle."""
    torch = torch_cuda
    rng = random.Random(77 + pad)
    n = 17000
    assert sponge_form(n, sorted=True)[0] == "k_sponge_count"
    lens = [rng.choice([0, 1, 3, 4, 5, 8, 9, 17, 33, 70]) if rng.random() < 0.8 else rng.randrange(0, 40) for _ in range(n)]
    lens[123] = 4 * 1030                                     # > 1023 blocks: clamps into the last bucket
    lens[4000] = 600
    offs = np.cumsum([0] + lens[:-1]).astype(np.uint64)
    pool = oracle.gen_b(8, int(sum(lens)) + 1)
    lens_a = np.array(lens, dtype=np.uint64)
    exp = oracle_sponge_var(oracle, pool, offs, lens_a, CAP, pad)
    dp, do, dl = to_dev(torch, pool).view(-1, 4), to_dev(torch, offs), to_dev(torch, lens_a)
    plain = to_host(H.sponge_hash_var(dp, do, dl, CAP, pad))
    srt, nb = _sponge_var_dev(torch, hades_lib, dp, pool.size // 4, offs, lens_a, CAP, pad, sort=True)
    assert (plain == exp).all() and (srt.reshape(-1) == exp).all() and nb == 0
    # tiny batches and n not a multiple of the block size
    for m in (1, 2, 63, 65, 257):
        e = oracle.sponge_var(pool, offs[:m], lens_a[:m], CAP, pad)
        assert (to_host(H.sponge_hash_var(dp, do[:m].contiguous(), dl[:m].contiguous(), CAP, pad, sort=True)) == e).all()


def test_sponge_sort_argument_errors(torch_cuda, hades_lib, H):
    torch = torch_cuda
    pool = H.gen_b(64, "cuda")
    off = torch.zeros(8, dtype=torch.int64, device="cuda")
    ln = torch.full((8,), 4, dtype=torch.int64, device="cuda")
    out = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    cap = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    small = torch.zeros(8, dtype=torch.int64, device="cuda")
    need = hades_lib.hades252_sponge_sort_scratch_bytes(8)
    assert need >= (1024 + 8) * 4
    assert hades_lib.hades252_sponge_hash_var_ex_dev(pool.data_ptr(), 64, off.data_ptr(), ln.data_ptr(), 8, cap, 1,
                                                     out.data_ptr(), None, small.data_ptr(), 64, None) == -5
    assert hades_lib.hades252_sponge_hash_var_ex_dev(pool.data_ptr(), 64, off.data_ptr(), ln.data_ptr(), 8, cap, 1,
                                                     out.data_ptr(), None, small.data_ptr() + 8, need, None) == -1


def test_streaming_sponge_absorb_squeeze(torch_cuda, H, oracle):
    """init + absorb (in one call, in two calls, block by block) + squeeze == the one-shot sponge without padding, and
    the full state after each absorb == the oracle's add-then-permute."""
    torch = torch_cuda
    n, t = 3000, 5
    msgs = oracle.gen_b(21, n * t * 4)                       # n messages of 4 t scalars
    exp = oracle.sponge(msgs, 4 * t, CAP, 0)
    dm = to_dev(torch, msgs).view(n, t, 4, 4)
    a = H.SpongeStates(n, CAP)
    a.absorb(dm)
    assert (to_host(a.squeeze()) == exp).all()
    b = H.SpongeStates(n, CAP)
    b.absorb(dm[:, :2].contiguous())
    b.absorb(dm[:, 2:].contiguous())
    assert torch.equal(a.states, b.states)
    c = H.SpongeStates(n, CAP)
    for i in range(t):
        c.absorb(dm[:, i].contiguous())
    assert torch.equal(a.states, c.states)
    # the whole state, not only the digest word: one absorb of one block vs oracle arithmetic
    d = H.SpongeStates(7, CAP)
    blk = oracle.gen_b(99, 7 * 4)
    d.absorb(to_dev(torch, blk).view(7, 1, 4, 4))
    st = np.zeros((7, 5, 4), dtype=np.uint64)
    st[:, 0] = np.array(limbs_of(CAP), dtype=np.uint64)
    st[:, 1:] = blk.reshape(7, 4, 4)                          # 0 + block
    assert (to_host(d.states) == oracle.perm_batch(st.reshape(-1))).all()
    for w in range(5):
        assert (to_host(d.squeeze(w)).reshape(7, 4) == to_host(d.states).reshape(7, 5, 4)[:, w]).all()
    # the C ABI equivalence promised in the header: pad_mode 0 one-shot == streaming
    assert (to_host(H.sponge_hash(to_dev(torch, msgs).view(-1, 4), 4 * t, CAP, 0)) == exp).all()


# ---------------------------------------------------------------------------------------------
# small batches: one message / state / query per wave (the low-latency forms of sponge, absorb and verification)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1])
def test_small_batch_sponge_one_message_per_wave(torch_cuda, hades_lib, H, oracle, pad):
    """Batches on both sides of the two dispatch thresholds (768: helper wave, 1024: one message per lane), ragged lengths
    inside a block of three / four waves (the helped form runs every wave to the block's maximum), empty messages,
    overlapping messages, one LONG message alone, a message outside the pool."""
    torch = torch_cuda
    rng = random.Random(5 + pad)
    pool = oracle.gen_b(1234, 3000)
    dp = to_dev(torch, pool).view(-1, 4)
    for n in (1, 2, 3, 4, 5, 100, 767, 768, 769, 1023, 1024, 1025, 1027, 1100, 4095, 4096, 4097, 5000, 16383, 16384, 16385):
        lens = [rng.choice([0, 1, 2, 3, 4, 5, 7, 8, 9, 13, 40]) for _ in range(n)]
        offs = [rng.randrange(0, 3000 - l + 1) for l in lens]              # anywhere in the pool: messages overlap
        la, oa = np.array(lens, dtype=np.uint64), np.array(offs, dtype=np.uint64)
        exp = oracle.sponge_var(pool, oa, la, CAP, pad)
        got = to_host(H.sponge_hash_var(dp, to_dev(torch, oa), to_dev(torch, la), CAP, pad))
        assert (got == exp).all(), n
        if n in (3, 768, 1024, 5000, 16385):
            srt, nb = _sponge_var_dev(torch, hades_lib, dp, 3000, oa, la, CAP, pad, sort=True)
            assert (srt.reshape(-1) == exp).all() and nb == 0, n
    # one long message (750 blocks): the chain of dependent permutations the low-latency form is for
    one = oracle.sponge_var(pool, np.array([0], dtype=np.uint64), np.array([2999], dtype=np.uint64), CAP, pad)
    assert (to_host(H.sponge_hash_var(dp, to_dev(torch, np.array([0], dtype=np.uint64)),
                                      to_dev(torch, np.array([2999], dtype=np.uint64)), CAP, pad)) == one).all()
    # fixed length, few messages
    for n, ln in ((1, 9), (7, 4), (770, 3), (1024, 1), (1025, 5), (4096, 3), (4097, 3), (16384, 2), (16385, 2)):
        msgs = oracle.gen_b(n + ln, n * ln)
        e = oracle.sponge(msgs, ln, CAP, pad)
        assert (to_host(H.sponge_hash(to_dev(torch, msgs).view(-1, 4), ln, CAP, pad)) == e).all(), (n, ln)
    # a message that does not lie inside the pool is hashed as the empty message and counted, never read
    la = np.array([4, 8, 4, 3000], dtype=np.uint64)
    oa = np.array([0, 2995, 3001, 1], dtype=np.uint64)                     # #1 runs past the end, #2 starts past it, #3 too long
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    cap = (ctypes.c_uint64 * 4)(*limbs_of(CAP))
    assert hades_lib.hades252_sponge_hash_var_dev(dp.data_ptr(), 3000, to_dev(torch, oa).data_ptr(),
                                                  to_dev(torch, la).data_ptr(), 4, cap, pad, out.data_ptr(),
                                                  bad.data_ptr(), None) == 0
    torch.cuda.synchronize()
    empty = oracle.sponge_var(pool, np.array([0], dtype=np.uint64), np.array([0], dtype=np.uint64), CAP, pad)
    good = oracle.sponge_var(pool, oa[:1], la[:1], CAP, pad)
    got = to_host(out).reshape(4, 4)
    assert int(bad.item()) == 3 and (got[0] == good).all() and all((got[i] == empty).all() for i in (1, 2, 3))


def test_small_batch_streaming_absorb(torch_cuda, H, oracle):
    torch = torch_cuda
    for n, t in ((1, 1), (1, 40), (3, 2), (4, 3), (767, 2), (769, 2), (1024, 1), (1025, 1), (1030, 3), (4095, 2), (4096, 1), (4097, 1),
                 (16384, 1), (16385, 1)):
        msgs = oracle.gen_b(31 * n + t, n * t * 4)
        exp = oracle.sponge(msgs, 4 * t, CAP, 0)
        st = H.SpongeStates(n, CAP)
        st.absorb(to_dev(torch, msgs).view(n, t, 4, 4))
        assert (to_host(st.squeeze()) == exp).all(), (n, t)
        # the whole state equals the per-lane kernel's (forced by a batch above the threshold sharing the first n states)
        if n <= 4:
            big = H.SpongeStates(20000, CAP)
            blocks = torch.zeros((20000, t, 4, 4), dtype=torch.int64, device="cuda")
            blocks[:n] = to_dev(torch, msgs).view(n, t, 4, 4)
            big.absorb(blocks)
            assert torch.equal(big.states[:n], st.states)


def test_sponge_golden_vectors_on_the_device(torch_cuda, H, oracle, kat):
    """The committed sponge vectors (tests/golden/kat.json `sponge`, the ones rust/tests/kat_scalar.rs hands to the real
    crate's `perm`) through the HIP path: one ragged batch per (capacity, padding rule)."""
    torch = torch_cuda
    vecs = kat["sponge"]["vectors"]
    groups = {}
    for v in vecs:
        groups.setdefault((v["capacity"], v["pad_mode"]), []).append(v)
    assert len(groups) == 4
    for (cap_hex, pad), vs in groups.items():
        pool = np.concatenate([oracle.gen_b(v["first_elem"], v["len"]) for v in vs] + [np.zeros(4, dtype=np.uint64)])
        lengths = [v["len"] for v in vs]
        offsets = [sum(lengths[:i]) for i in range(len(vs))]
        got = H.sponge_hash_var(to_dev(torch, pool), to_dev(torch, np.array(offsets, dtype=np.uint64)),
                                to_dev(torch, np.array(lengths, dtype=np.uint64)), S.to_mont(int(cap_hex, 16)), pad)
        host = to_host(got).reshape(-1, 4)
        for i, v in enumerate(vs):
            assert int_of(host[i]) == int(v["digest_mont"], 16), v


# ---------------------------------------------------------------------------------------------
# every kernel form, guarded outputs, edge values, bad messages, the device sort (tests/gpu_common.py: form table, sizes)
# ---------------------------------------------------------------------------------------------
FORM_KERNEL = {"lanes_helped": "k_sponge_lanes<true>", "lanes": "k_sponge_lanes<false>", "rows": "k_sponge_rows",
               "coop": "k_sponge_coop", "fast": "k_sponge"}
CAPS = [P - 1, 0, R]


def _cap(v):
    return (ctypes.c_uint64 * 4)(*limbs_of(v))


def _sponge_var_dev(torch, hades_lib, dpool, n_scalars, offs, lens, cap, pad, sort=False):
    """hades252_sponge_hash_var_ex_dev into a guarded digest buffer.  sort: scratch of exactly
    hades252_sponge_sort_scratch_bytes(n), zero-filled (a slot never written then names message 0, inside the batch), and
    a guard after it.  Returns (digests [n, 4] uint64, bad count)."""
    n = len(offs)
    do, dl = to_dev(torch, np.asarray(offs, dtype=np.uint64)), to_dev(torch, np.asarray(lens, dtype=np.uint64))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    sptr, sbytes, scr = None, 0, None
    if sort:
        sbytes = hades_lib.hades252_sponge_sort_scratch_bytes(n)
        scr = torch.full((sbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        scr[:sbytes].zero_()
        sptr = scr.data_ptr()
    got = guarded_call(torch, (n, 4), lambda ptr: hades_lib.hades252_sponge_hash_var_ex_dev(
        dpool.data_ptr(), n_scalars, do.data_ptr(), dl.data_ptr(), n, _cap(cap), pad, ptr, bad.data_ptr(), sptr, sbytes,
        None), "sponge n=%d sort=%s" % (n, sort))
    if sort:
        assert bool((scr[sbytes:] == 0xA5).all()), "write past the sort scratch"
    return to_host(got).reshape(n, 4), int(bad.item())


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("form", list(FORM_SIZES))
def test_sponge_var_every_form_edges_trips_and_bad_messages(torch_cuda, hades_lib, oracle, form, pad):
    """Every form at its first, ragged and last size: trip-count patterns on its group boundaries, edge-value pool and
    capacity (p-1, 0, R), out-of-pool messages counted exactly and hashed as the empty message, every other digest
    equal to the oracle; plain and with sort scratch (the sort runs only in the per-lane form)."""
    torch = torch_cuda
    rng = random.Random("%s/%d" % (form, pad))
    n_pool = 4000
    pool = edge_scalars(n_pool, 31 + pad)
    dp = to_dev(torch, pool).view(-1, 4)
    empty = {}
    for k, n in enumerate(FORM_SIZES[form]):
        assert sponge_form(n) == (FORM_KERNEL[form],)
        cap = CAPS[k % 3]
        lens = _trip_layout(n, GROUP[form], rng)
        offs = [rng.randrange(0, n_pool - l + 1) for l in lens]
        n_bad = 0
        if n >= 16:
            bads, good_end = _bad_messages(n, n_pool)
            for i, o, l in bads:
                offs[i], lens[i] = o, l
            offs[good_end[0]], lens[good_end[0]] = good_end[1], good_end[2]
            n_bad = len(bads)
        oa, la = np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64)
        bad_mask = (oa > n_pool) | (la > np.uint64(n_pool) - np.minimum(oa, np.uint64(n_pool)))
        assert int(bad_mask.sum()) == n_bad
        so, sl = oa.copy(), la.copy()
        so[bad_mask], sl[bad_mask] = 0, 0
        exp = oracle_sponge_var(oracle, pool, so, sl, cap, pad).reshape(n, 4)
        if cap not in empty:
            empty[cap] = oracle.sponge_var(pool, np.zeros(1, np.uint64), np.zeros(1, np.uint64), cap, pad).reshape(4)
        assert (exp[bad_mask] == empty[cap]).all()
        for sort in (False, True):
            got, nb = _sponge_var_dev(torch, hades_lib, dp, n_pool, oa, la, cap, pad, sort)
            assert nb == n_bad, (form, n, sort, nb)
            assert (got == exp).all(), (form, n, sort, np.flatnonzero((got != exp).any(axis=1))[:10])


@pytest.mark.parametrize("form", list(FORM_SIZES))
def test_sponge_fixed_length_every_form(torch_cuda, hades_lib, oracle, form):
    """hades252_sponge_hash_dev, lengths 1..16 (those = 0 mod 4 take an extra block with pad mode 1), edge-value messages
    and capacity, into guarded digests, vs the oracle."""
    torch = torch_cuda
    n = FORM_SIZES[form][0 if form in ("coop", "fast") else 1]
    assert sponge_form(n) == (FORM_KERNEL[form],)
    for length in (1, 2, 3, 4, 5, 7, 8, 9, 16):
        msgs = edge_scalars(n * length, 1000 * length + n)
        dm = to_dev(torch, msgs)
        for pad in (0, 1):
            cap = CAPS[(length + pad) % 3]
            exp = oracle_sponge_var(oracle, msgs, np.arange(n, dtype=np.uint64) * np.uint64(length),
                                    np.full(n, length, dtype=np.uint64), cap, pad).reshape(n, 4)
            got = guarded_call(torch, (n, 4), lambda ptr: hades_lib.hades252_sponge_hash_dev(
                dm.data_ptr(), n, length, _cap(cap), pad, ptr, None), (form, length, pad))
            assert (to_host(got).reshape(n, 4) == exp).all(), (form, length, pad)


def _occupied_buckets(lens, pad):
    b = (np.asarray(lens, dtype=np.uint64) + np.uint64(pad + 3)) // np.uint64(4)     # wraps like the kernel's
    b = np.maximum(b, np.uint64(1))
    return np.minimum(b, np.uint64(SPONGE_BUCKETS - 1)).astype(np.int64)


def _sort_case(case, pad, rng):
    """(lengths, pool size) of the four sorted-batch cases, each above COOP_MAX messages."""
    if case == "one_bucket":
        return [5] * 20000, 64
    if case == "every_bucket":                        # buckets 1 .. 1023, one long message each, the rest short
        lens = [rng.randrange(0, 13) for _ in range(20000)]
        pos = rng.sample(range(20000), SPONGE_BUCKETS - 1)
        for b, i in enumerate(pos, 1):
            lens[i] = 4 * b - pad
        return lens, 4 * SPONGE_BUCKETS
    if case == "clamp":                               # > 1022 blocks: the last bucket; 4088 moves bucket with the pad mode
        lens = [rng.randrange(0, 13) for _ in range(17000)]
        for i in rng.sample(range(17000), 27):
            lens[i] = rng.choice([4084, 4085, 4087, 4088, 4089, 4091, 4092, 4096, 4120])
        return lens, 4200
    n = COUNT_GRID_RECORDS + 1037                     # k_sponge_count takes a second grid-stride trip
    return np.random.default_rng(7 + pad).integers(0, 13, size=n), 64


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("case", ["one_bucket", "every_bucket", "clamp", "strided_count"])
def test_sponge_device_sort_cases(torch_cuda, hades_lib, oracle, case, pad):
    """The counting sort (k_sponge_count / _scan / _scatter) in front of k_sponge: sorted digests == unsorted k_sponge
    digests for the whole batch (each in its own guarded buffer, zero-filled scratch with a guard after it) == the oracle
    (whole batch up to ~20 000 messages, else the first and last message of every occupied bucket + 3 000 random)."""
    torch = torch_cuda
    rng = random.Random("%s/%d" % (case, pad))
    lens, n_pool = _sort_case(case, pad, rng)
    n = len(lens)
    assert sponge_form(n, sorted=True) == ("k_sponge_count", "k_sponge_scan", "k_sponge_scatter", "k_sponge")
    buckets = _occupied_buckets(lens, pad)
    occ = np.unique(buckets)
    if case == "one_bucket":
        assert occ.size == 1
    elif case == "every_bucket":
        assert occ.size == SPONGE_BUCKETS - 1 and occ.size > 64
    elif case == "clamp":
        assert (buckets == SPONGE_BUCKETS - 1).sum() >= 10 and max(lens) > 4 * (SPONGE_BUCKETS - 1)
    else:
        assert n > COUNT_GRID_RECORDS
    pool = edge_scalars(n_pool + 8, 77 + pad)
    la = np.array(lens, dtype=np.uint64)
    oa = np.array([rng.randrange(0, n_pool - int(l) + 1) for l in lens], dtype=np.uint64) if n <= 20000 else \
        np.random.default_rng(3).integers(0, n_pool - 12, size=n).astype(np.uint64)
    dp = to_dev(torch, pool).view(-1, 4)
    cap = CAPS[pad]
    plain, nb0 = _sponge_var_dev(torch, hades_lib, dp, n_pool + 8, oa, la, cap, pad, sort=False)
    srt, nb1 = _sponge_var_dev(torch, hades_lib, dp, n_pool + 8, oa, la, cap, pad, sort=True)
    assert nb0 == nb1 == 0
    diff = np.flatnonzero((plain != srt).any(axis=1))
    assert diff.size == 0, (case, diff.size, diff[:10])
    if n <= 20000:
        sample = np.arange(n)
    else:
        firsts = [int(np.flatnonzero(buckets == b)[0]) for b in occ] + [int(np.flatnonzero(buckets == b)[-1]) for b in occ]
        sample = np.unique(np.concatenate([np.array(firsts), np.random.default_rng(11).integers(0, n, size=3000), [0, n - 1]]))
    exp = oracle_sponge_var(oracle, pool, oa[sample], la[sample], cap, pad).reshape(-1, 4)
    assert (plain[sample] == exp).all(), case


@pytest.mark.parametrize("form", list(FORM_SIZES))
def test_streaming_every_form_guarded(torch_cuda, hades_lib, oracle, form):
    """init / absorb / squeeze in every absorb form (the per-lane k_sponge_absorb above COOP_MAX states), on guarded
    in-place state buffers: one call == two calls == block by block (whole states); one absorb of an edge-value block ==
    oracle perm([capacity, 0 + block]) on every word; squeeze(w), w = 0..4; blocks_each = 0 is a no-op."""
    torch = torch_cuda
    lib = hades_lib
    n, t = FORM_SIZES[form][1], 3
    kern = {"lanes_helped": "k_sponge_absorb_lanes<true>", "lanes": "k_sponge_absorb_lanes<false>",
            "rows": "k_sponge_absorb_rows", "coop": "k_sponge_absorb_coop", "fast": "k_sponge_absorb"}[form]
    assert absorb_form(n) == kern
    cap = CAPS[len(form) % 3]
    blocks = edge_scalars(n * t * 4, 500 + n)
    db = to_dev(torch, blocks).view(n, t, 4, 4)

    def fresh():
        g = Guarded(torch, (n, 5, 4))
        assert lib.hades252_sponge_init_dev(g.ptr, n, _cap(cap), None) == 0
        g.check("init")
        return g

    def absorb(g, blk, each):
        assert lib.hades252_sponge_absorb_dev(g.ptr, blk.data_ptr(), n, each, None) == 0
        g.check("absorb")

    a = fresh()
    absorb(a, db, t)
    b = fresh()
    absorb(b, db[:, :1].contiguous(), 1)
    absorb(b, db[:, 1:].contiguous(), t - 1)
    c = fresh()
    for i in range(t):
        absorb(c, db[:, i].contiguous(), 1)
    assert torch.equal(a.t, b.t) and torch.equal(a.t, c.t)
    before = a.t.clone()
    absorb(a, db, 0)
    assert torch.equal(a.t, before)
    # squeeze every word, into guarded digests
    for w in range(5):
        got = guarded_call(torch, (n, 4), lambda ptr: lib.hades252_sponge_squeeze_dev(a.ptr, ptr, n, w, None), ("squeeze", w))
        assert torch.equal(got, a.t[:, w]), w
    # the digest word == the one-shot sponge without padding over the same scalars
    exp = oracle_sponge_var(oracle, blocks, np.arange(n, dtype=np.uint64) * np.uint64(4 * t),
                            np.full(n, 4 * t, dtype=np.uint64), cap, 0).reshape(n, 4)
    assert (to_host(a.t[:, 1]).reshape(n, 4) == exp).all()
    # one absorb of one block: every word == perm([capacity, 0 + block])
    d = fresh()
    absorb(d, db[:, 0].contiguous(), 1)
    st = np.zeros((n, 5, 4), dtype=np.uint64)
    st[:, 0] = np.array(limbs_of(cap), dtype=np.uint64)
    st[:, 1:] = blocks.reshape(n, t, 4, 4)[:, 0]
    assert (to_host(d.t) == oracle.perm_batch(st.reshape(-1))).all()
