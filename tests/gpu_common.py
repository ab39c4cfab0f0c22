"""Helpers shared by the GPU-tier test files (tests/test_gpu_*.py, one file per SURVEY section 8 row).  The fixtures
`torch_cuda` and `H` live in conftest.py."""
import os
import random
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402
from oracle_lib import P, R, limbs_of, int_of  # noqa: E402
from test_blob_kat import ARK_SHA256, MDS_SHA256, blob_bytes  # noqa: E402,F401

__all__ = ["KERNELS", "TAG", "TAG4", "CAP", "SITES_PERM", "to_dev", "to_host", "hex_of", "scalars_dev", "rows",
           "kernel_available", "each_state_is_input_or_output", "_record", "word_boundary_values", "ARK_SHA256", "MDS_SHA256",
           "blob_bytes", "EDGE_VALUES", "edge_scalars", "SENTINEL", "Guarded", "guarded_call", "FORM_SIZES", "LEVEL_SIZES",
           "sponge_form", "absorb_form", "level_form", "verify_form", "update_form", "form_family", "oracle_sponge_var",
           "SPONGE_BUCKETS", "COUNT_GRID_RECORDS", "CATALOGUE_LANES", "catalogue_states", "placed_batches", "WIRES",
           "mont_rows", "perm_many_over", "gadget_check", "assert_wires_are_perm_witness", "M64", "GROUP", "_trip_layout",
           "_bad_messages"]

KERNELS = [1, 2, 3, 4, 5]   # HADES252_KERNEL_LITERAL, _FAST (one state per lane), _COOP (five waves per state), _LANES (one
                            # state per wave, elements spread over 16-lane rows), _ROWS (one state per row, four per wave)
TAG = {1: S.to_mont(1), 2: S.to_mont(3), 3: S.to_mont(7), 4: S.to_mont(15)}      # per-arity domain tags of the Merkle tests
TAG4 = S.to_mont(15)
CAP = S.to_mont(1 << 64)
SITES_PERM = ["malloc", "hostmalloc", "hostregister", "memcpy", "streamcreate", "eventcreate", "sync"]


def to_dev(torch, arr):
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy((a if a.flags.writeable else a.copy()).view(np.int64)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1)


def hex_of(t):
    return hex(int_of(to_host(t)))


def scalars_dev(torch, ints):
    return to_dev(torch, np.array([l for v in ints for l in limbs_of(v)], dtype=np.uint64)).view(-1, 4)


def rows(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def kernel_available(hades_lib, torch, k):
    t = torch.zeros(20, dtype=torch.int64, device="cuda")
    return hades_lib.hades252_perm_batch_dev_ex(t.data_ptr(), 1, None, k) == 0


def each_state_is_input_or_output(got, inp, exp):
    g, i, e = got.reshape(-1, 20), inp.reshape(-1, 20), exp.reshape(-1, 20)
    is_in, is_out = (g == i).all(axis=1), (g == e).all(axis=1)
    return bool((is_in | is_out).all()), int(is_out.sum())


def _record(name, text):
    """Append a line to gpurun_out/<name> (travels back from the GPU box: evidence of the full-size runs)."""
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, name), "a") as f:
        f.write(text + "\n")


def word_boundary_values():
    """The per-32-bit-word boundary around p: (value, canonical?) pairs, for each word k: p + 2^(32 k) (not canonical),
    p - 2^(32 k) (canonical), p's words above k with word k one lower and every word below it all ones (canonical), and p
    with one word below k one higher (not canonical); then 2^255, 2^256 - 1, p (not canonical), p - 1 and 0."""
    p = S.P
    words = [(p >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
    out = []
    for k in range(8):
        out.append((p + (1 << (32 * k)), False))
        out.append((p - (1 << (32 * k)), True))
        if words[k] > 0:
            out.append((p >> (32 * (k + 1)) << (32 * (k + 1)) | (words[k] - 1) << (32 * k) | ((1 << (32 * k)) - 1), True))
        for j in range(k):
            if words[j] < 0xFFFFFFFF:
                out.append((p + (1 << (32 * j)), False))
    out += [(1 << 255, False), ((1 << 256) - 1, False), (p, False), (p - 1, True), (0, True)]
    assert all((v < p) == ok for v, ok in out)
    return out


# ---------------------------------------------------------------------------------------------
# edge values: the field elements where a modular add / reduce goes wrong (shared by the perm, sponge and Merkle tiers)
# ---------------------------------------------------------------------------------------------
EDGE_VALUES = [0, 1, 2, P - 1, P - 2, R, P - R, (1 << 255) % P, (1 << 254) - 1, 0xFFFFFFFF, P - (1 << 32),
               0xFFFFFFFF00000000, (P - 1) // 2, (1 << 128) - 1]


def edge_scalars(n, seed, edge_ratio=0.5):
    """n canonical scalars (4 uint64 limbs each, flat): each one an EDGE_VALUES entry with probability edge_ratio, else
    uniform-ish below p (random low limbs, top limb below p's).  Used as Montgomery words directly (every canonical value
    is one)."""
    rng = np.random.default_rng(seed)
    tab = np.array([limbs_of(v) for v in EDGE_VALUES], dtype=np.uint64)
    out = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False)
    out[:, 3] %= np.uint64(P >> 192)
    edge = rng.random(n) < edge_ratio
    out[edge] = tab[rng.integers(0, len(EDGE_VALUES), size=int(edge.sum()))]
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------
# guarded outputs: the kernel writes into the interior of a buffer whose guard rows (before and after) and interior start
# out as the non-canonical sentinel 2^256 - 1 (every word above p: no result equals it)
# ---------------------------------------------------------------------------------------------
SENTINEL = -1          # int64 view of 0xFFFF_FFFF_FFFF_FFFF
GUARD_ROWS = 64        # 32-byte rows on each side (2 KiB)


class Guarded:
    """A device buffer [GUARD_ROWS | interior | GUARD_ROWS] of int64, all SENTINEL; `.t` is the interior in `shape`
    (the last dimension a multiple of 4 limbs).  `init` (optional) is copied into the interior (in-place kernels)."""

    def __init__(self, torch, shape, init=None):
        self.torch = torch
        n = int(np.prod(shape))
        assert n % 4 == 0
        g = GUARD_ROWS * 4
        self.buf = torch.full((g + n + g,), SENTINEL, dtype=torch.int64, device="cuda")
        self.g, self.n = g, n
        self.t = self.buf[g:g + n].view(*shape)
        if init is not None:
            self.t.copy_(init.reshape(shape))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what="", interior=True):
        """The guards are intact and (interior) no 32-byte word of the interior still holds the sentinel."""
        self.torch.cuda.synchronize()
        g = self.g
        assert bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[g + self.n:] == SENTINEL).all()), \
            "guard row overwritten %s" % (what,)
        if not interior:
            return self.t
        left = int((self.buf[g:g + self.n].view(-1, 4) == SENTINEL).all(dim=1).sum().item())
        assert left == 0, "%d interior word(s) never written %s" % (left, what)
        return self.t


def guarded_call(torch, shape, call, what=""):
    """Run `call(ptr)` (a C-ABI call through hades_lib returning its status) on the interior of a fresh Guarded buffer;
    assert the status is 0, the guards are intact and every interior word was written.  Returns the interior."""
    g = Guarded(torch, shape)
    rc = call(g.ptr)
    assert rc == 0, "status %d %s" % (rc, what)
    return g.check(what)


# ---------------------------------------------------------------------------------------------
# which kernel runs: a mirror of the size dispatch of abi_sponge.hpp, abi_merkle.hpp and launch.hpp (tests/test_chain_forms.py
# checks it against the library's exported size rule; the GPU tests assert that their sizes reach every form they claim)
# ---------------------------------------------------------------------------------------------
LANES_HELPED_MAX, LANES_MAX, ROWS_MAX, COOP_MAX = 768, 1 << 10, 1 << 12, 1 << 14
SPONGE_BUCKETS = 1024                # counting-sort buckets (the last one takes every longer message)
COUNT_GRID_RECORDS = 2048 * 256      # k_sponge_count's grid cap: larger batches take a second grid-stride trip


def _chain(n, lanes, rows, coop, lane):
    if n <= LANES_HELPED_MAX:
        return lanes % "true"
    if n <= LANES_MAX:
        return lanes % "false"
    if n <= ROWS_MAX:
        return rows
    if n <= COOP_MAX:
        return coop
    return lane


def sponge_form(n, sorted=False):
    """The kernels hades252_sponge_hash[_var_ex]_dev launches for n messages, in launch order (the chain kernel last).
    `sorted`: scratch was given -- the device sort runs only above COOP_MAX messages."""
    chain = _chain(n, "k_sponge_lanes<%s>", "k_sponge_rows", "k_sponge_coop", "k_sponge")
    if sorted and n > COOP_MAX:
        return ("k_sponge_count", "k_sponge_scan", "k_sponge_scatter", chain)
    return (chain,)


def absorb_form(n):
    """The kernel hades252_sponge_absorb_dev runs for n states."""
    return _chain(n, "k_sponge_absorb_lanes<%s>", "k_sponge_absorb_rows", "k_sponge_absorb_coop", "k_sponge_absorb")


def level_form(n_children, arity):
    """The kernel one level of n_children children runs (hades252_merkle_level_pad_dev, and every unfused level of a tree):
    a ragged level of COOP_MAX or fewer parents above ROWS_MAX runs one parent per lane, not five waves per parent."""
    n = -(-n_children // arity)
    if n <= LANES_MAX:
        return "k_merkle_lanes<%d, %s>" % (arity, "true" if n <= LANES_HELPED_MAX else "false")
    if n <= ROWS_MAX:
        return "k_merkle_rows<%d>" % arity
    if n <= COOP_MAX and n_children % arity == 0:
        return "k_merkle_coop<%d>" % arity
    return "k_merkle_level_fast<%d>" % arity


def verify_form(nq, arity):
    """The kernel hades252_merkle_verify_dev runs for nq queries."""
    return _chain(nq, "k_merkle_verify_lanes<%d, %%s>" % arity, "k_merkle_verify_rows<%d>" % arity,
                  "k_merkle_verify_coop<%d>" % arity, "k_merkle_verify<%d>" % arity)


def update_form(nu, arity):
    """The kernel hades252_merkle_update_dev runs for nu updates on a level of more than nu parents (a level with no more
    parents than updates is recomputed whole, by level_form)."""
    return _chain(nu, "k_merkle_update_lanes<%d, %%s>" % arity, "k_merkle_update_rows<%d>" % arity,
                  "k_merkle_update_coop<%d>" % arity, "k_merkle_update_fast<%d>" % arity)


def form_family(name):
    """"lanes" / "rows" / "coop" / "fast": the per-state arithmetic of a chain kernel (hades252_chain_form_for's answer)."""
    base = name.split("<")[0]
    for fam in ("lanes", "rows", "coop"):
        if base.endswith("_" + fam):
            return fam
    return "fast"


# One size list per form (chains, messages, states, queries, updates, or parents of a level): first size, a ragged size
# inside, last size.  The one-chain-per-lane form has no last size: its third entry is a second ragged size.
FORM_SIZES = {"lanes_helped": (1, 386, 768), "lanes": (769, 901, 1024), "rows": (1025, 2051, 4096),
              "coop": (4097, 9001, 16384), "fast": (16385, 17003, 20011)}
# Levels: the coop form takes full levels only; the per-lane one also every ragged level above ROWS_MAX parents
LEVEL_SIZES = dict(FORM_SIZES, fast_ragged=(4097, 9001, 16384))


def oracle_sponge_var(oracle, pool, offsets, lengths, cap, pad, threads=16):
    """oracle.sponge_var over chunks on host threads (the C oracle is single-threaded per call and releases the GIL)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    n = offsets.size
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    step = -(-n // threads)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda a: oracle.sponge_var(pool, offsets[a:a + step], lengths[a:a + step], cap, pad),
                            range(0, n, step)))
    return np.concatenate(parts)


# ---------------------------------------------------------------------------------------------
# ragged sponge batches: trip-count patterns on a form's group boundaries, messages outside the pool (device-free: the GPU
# tier and the host simulation tier drive the same layouts)
# ---------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
# messages that share one trip count in each form: the three of a helped block, one per wave (four waves a block)
# unhelped, the four of a wave in rows, the 64 of a block in coop, the 64 of a wave in the per-lane kernel
GROUP = {"lanes_helped": 3, "lanes": 4, "rows": 4, "coop": 64, "fast": 64}


def _trip_layout(n, group, rng, short=(0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 17)):
    """Ragged lengths with three patterns aligned to the form's group boundaries, at the start and in the middle of the
    batch: one long message among short ones, an all-empty group, a group of lengths 0..3 around the pad boundary."""
    lens = [rng.choice(short) for _ in range(n)]
    for base in (0, group * (n // group // 2)):
        if base + 3 * group > n:
            continue
        lens[base:base + group] = [1] * group
        lens[base + group // 2] = 33
        lens[base + group:base + 2 * group] = [0] * group
        lens[base + 2 * group:base + 3 * group] = [i % 4 for i in range(group)]
    return lens


def _bad_messages(n, n_pool):
    """(index, offset, length) of messages that do not lie inside a pool of n_pool scalars, and one that does (an empty
    message at the very end), for a batch of n >= 16."""
    return [(n // 7, n_pool - 2, 8),                 # runs past the end
            (n // 5, n_pool + 1, 4),                 # starts past the end
            (n // 3, n_pool + 1, 0),                 # starts past the end, empty
            (n // 2, M64 - 2, 8),                    # offset + length wraps past 2^64
            (n - 3, 5, M64),                         # length near 2^64 (len + 4 wraps in the sort's bucket)
            (n - 1, 0, M64 - 3)], (n - 2, n_pool, 0)


# ---------------------------------------------------------------------------------------------
# edge values inside the rounds: the catalogue of tests/round_inverse.py as device input, and batches that place it at the
# lanes where a kernel's wave, row and block boundaries fall
# ---------------------------------------------------------------------------------------------
CATALOGUE_LANES = (0, 63, 64, 255, 256)          # ... and the last lane of the batch


def catalogue_states():
    """(states, labels): the round_inverse catalogue as in-memory Montgomery limbs, uint64 [entries, 20]."""
    import round_inverse as RI
    cat = RI.edge_catalogue()
    states = np.array([[l for v in inp for l in limbs_of(S.to_mont(v))] for inp, _ in cat], dtype=np.uint64)
    return states, [lab for _, lab in cat]


def placed_batches(states, n, fill):
    """Batches of n states that together hold every row of `states` (uint64 [entries, 20]) once: the rows sit at lanes
    CATALOGUE_LANES and n - 1 (those below n), the rest of each batch is `fill` (uint64 [n, 20]).  Yields (batch
    [n, 20], lanes, row indices)."""
    lanes = sorted({l for l in CATALOGUE_LANES if l < n} | {n - 1})
    for first in range(0, len(states), len(lanes)):
        idx = list(range(first, min(first + len(lanes), len(states))))
        b = fill.copy()
        b[lanes[:len(idx)]] = states[idx]
        yield b, lanes[:len(idx)], idx


# ---------------------------------------------------------------------------------------------
# the gadget witness families (perm_witness and the chains recorded over it): what each of them checks on its wires
# ---------------------------------------------------------------------------------------------
WIRES = 972                                      # wires per permutation record


def mont_rows(vals):
    """Canonical integers as in-memory Montgomery limbs, uint64 [len(vals), 4]."""
    return np.array([limbs_of(S.to_mont(v)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def perm_many_over(oracle):
    """A big-integer model's perm_many over the C oracle (Montgomery limbs in between)."""
    def run(states):
        if not states:
            return []
        out = oracle.perm_batch(mont_rows([v for st in states for v in st]).reshape(-1)).reshape(-1, 5, 4)
        return [[S.from_mont(int_of(w)) for w in st] for st in out]
    return run


def gadget_check(wires_h, inputs_h, pairs):
    """Records (s, i) of `pairs` against the spec's GadgetStrategy, wire for wire: host arrays wires_h [WIRES, S, n, 4]
    and inputs_h [S, n, 5, 4]."""
    for (s, i) in pairs:
        st = [S.from_mont(int_of(inputs_h[s, i, w])) for w in range(5)]
        spec = []
        S.perm_gadget(st, spec)
        got = [int_of(wires_h[g, s, i]) for g in range(WIRES)]
        bad = [g for g in range(WIRES) if got[g] != S.to_mont(spec[g])]
        assert not bad, ((s, i), bad[:8])


def assert_wires_are_perm_witness(torch, H, inputs, wires):
    """The defining property of every chain witness: wires == perm_witness(inputs), byte for byte."""
    ref = H.perm_witness(inputs.reshape(-1, 20))
    assert torch.equal(wires.reshape(WIRES, -1, 4), ref)
