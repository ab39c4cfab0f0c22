"""CPU tier: the chain kernels over the permutation -- sponge (fixed, variable, sorted, streaming), cipher, duplex sponge
(one-shot and streaming) and the chain witnesses -- in their one-chain-per-lane form and, where they have one, their
five-waves-per-chain form, through the shipped size dispatch in the host build under ASan+UBSan, byte for byte against
the oracle and the Python models over it.  Sizes are the first of each form (tests/gpu_common.py FORM_SIZES); the
trip-count layout and the out-of-pool messages are those of the GPU tier (tests/gpu_common.py)."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hades_spec as S  # noqa: E402
import hostsim_lib as HS  # noqa: E402
import oracle_lib  # noqa: E402
import cipher_model as CM  # noqa: E402
import safe_model as SM  # noqa: E402
import safe_witness_model as SW  # noqa: E402
from safe_model import A, Q  # noqa: E402
from oracle_lib import P, R, limbs_of  # noqa: E402
from gpu_common import (CAP, TAG, WIRES, edge_scalars, sponge_form, absorb_form, FORM_SIZES, oracle_sponge_var,  # noqa: E402
                        COOP_MAX, LANES_MAX, _bad_messages, _trip_layout, GROUP)

N_COOP, N_FAST = FORM_SIZES["coop"][0], FORM_SIZES["fast"][0]
N_LANE_CIPHER = LANES_MAX + 1                             # cipher and duplex sponge: one per lane above 1 024


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def u64(b):
    return np.frombuffer(b, dtype=np.uint64)


def limbs(v):
    return np.array(limbs_of(v), dtype=np.uint64).tobytes()


# ---- sponge -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,msg_len,pad", [(N_COOP, 3, 1), (N_FAST, 5, 1)])    # (pad mode 0: test_sponge_streaming)
def test_sponge_fixed(oracle, n, msg_len, pad):
    assert sponge_form(n) == (("k_sponge_coop",) if n <= COOP_MAX else ("k_sponge",))
    msgs = edge_scalars(n * msg_len, 200 + msg_len)
    s = HS.Script("sponge")
    s.buf("msgs", msgs.tobytes())
    s.buf("cap", limbs(CAP))
    s.fill("dig", 32 * n, 0xFF)
    s.call("hades252_sponge_hash_dev", "msgs", n, msg_len, "cap", pad, "dig", None)
    s.dump("dig")
    r = s.run(timeout=900)                               # measured: 13 s (five waves, one block each) / 15 s (per lane, two blocks)
    assert r.rc == [("hades252_sponge_hash_dev", 0)]
    assert (u64(r.out["dig"]) == oracle.sponge(msgs, msg_len, CAP, pad)).all()


@pytest.mark.parametrize("form,sort", [("coop", False), ("fast", False), ("fast", True)])
def test_sponge_variable_with_out_of_pool_messages(oracle, form, sort):
    """Trip-count patterns on the form's group boundaries, out-of-pool messages counted and hashed as the empty message;
    with sort scratch the counting sort (k_sponge_count / _scan / _scatter) runs first."""
    n = FORM_SIZES[form][0]
    rng = random.Random("hostsim/%s" % form)
    n_pool, pad = 4000, 1
    pool = edge_scalars(n_pool, 31)
    lens = [min(l, 9) for l in _trip_layout(n, GROUP[form], rng)]       # at most three blocks per message
    offs = [rng.randrange(0, n_pool - l + 1) for l in lens]
    bads, good_end = _bad_messages(n, n_pool)
    for i, o, l in bads:
        offs[i], lens[i] = o, l
    offs[good_end[0]], lens[good_end[0]] = good_end[1], good_end[2]
    oa, la = np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64)
    bad_mask = (oa > n_pool) | (la > np.uint64(n_pool) - np.minimum(oa, np.uint64(n_pool)))
    assert int(bad_mask.sum()) == len(bads)
    so, sl = oa.copy(), la.copy()
    so[bad_mask], sl[bad_mask] = 0, 0
    exp = oracle_sponge_var(oracle, pool, so, sl, CAP, pad, threads=8)
    s = HS.Script("sponge")
    s.buf("pool", pool.tobytes())
    s.buf("offs", oa.tobytes())
    s.buf("lens", la.tobytes())
    s.buf("cap", limbs(CAP))
    s.fill("dig", 32 * n, 0xFF)
    s.zero("bad", 4)
    if sort:
        s.call("hades252_sponge_sort_scratch_bytes", n)
        scratch = 4 * n + 4 * 1024 + 64                   # upper bound; the call above prints the exact need
        s.fill("scratch", scratch + 4096, 0xFF)
        s.call("hades252_sponge_hash_var_ex_dev", "pool", n_pool, "offs", "lens", n, "cap", pad, "dig", "bad", "scratch",
               scratch + 4096, None)
    else:
        s.call("hades252_sponge_hash_var_dev", "pool", n_pool, "offs", "lens", n, "cap", pad, "dig", "bad", None)
    s.dump("dig")
    s.dump("bad")
    r = s.run(timeout=900)                               # measured: 15 s (five waves, three trips) / 11 s (per lane) / 18 s (sorted)
    assert r.rc[-1][1] == 0
    if sort:
        assert 0 < r.rc[0][1] <= scratch + 4096
    assert int(np.frombuffer(r.out["bad"], dtype=np.int32)[0]) == len(bads)
    assert (u64(r.out["dig"]) == exp).all()


@pytest.mark.parametrize("n", [N_COOP, N_FAST])
def test_sponge_streaming(oracle, n):
    """init, absorb of one block, squeeze of word 1 == the fixed-length sponge with zero fill (pad mode 0)."""
    assert absorb_form(n) == ("k_sponge_absorb_coop" if n <= COOP_MAX else "k_sponge_absorb")
    msg_len, blocks = 3, 1
    msgs = edge_scalars(n * msg_len, 210).reshape(n, msg_len, 4)
    blk = np.zeros((n, 4 * blocks, 4), dtype=np.uint64)
    blk[:, :msg_len] = msgs
    s = HS.Script("sponge")
    s.buf("cap", limbs(CAP))
    s.fill("st", 160 * n, 0xFF)
    s.buf("blk", blk.tobytes())
    s.fill("dig", 32 * n, 0xFF)
    s.call("hades252_sponge_init_dev", "st", n, "cap", None)
    s.call("hades252_sponge_absorb_dev", "st", "blk", n, blocks, None)
    s.call("hades252_sponge_squeeze_dev", "st", "dig", n, 1, None)
    s.dump("dig")
    r = s.run(timeout=900)                               # measured: 17 s (five waves) / 34 s (per lane)
    assert [rc for _, rc in r.rc] == [0, 0, 0]
    assert (u64(r.out["dig"]) == oracle.sponge(msgs.reshape(-1), msg_len, CAP, 0)).all()


# ---- cipher -----------------------------------------------------------------------------------------------------------
def cipher_inputs(n, m, seed):
    return (edge_scalars(n * m, seed).reshape(n, m, 4), edge_scalars(2 * n, seed + 1).reshape(n, 2, 4),
            edge_scalars(n, seed + 2).reshape(n, 4))


@pytest.mark.parametrize("m", [2, 5])
def test_cipher_encrypt_decrypt_tampered_and_non_canonical(oracle, m):
    n = N_LANE_CIPHER                                    # 1 025: the per-lane form, five blocks with one message in the last
    msgs, keys, nonces = cipher_inputs(n, m, 300 + m)
    exp_c = CM.encrypt_batch(msgs, keys, nonces, m, oracle.perm_batch)
    tampered = exp_c.copy()
    rng = np.random.default_rng(301)
    for i in range(0, n, 5):                              # every fifth message: one word changed (the tag every 15th)
        w = m if i % 15 == 0 else int(rng.integers(0, m))
        tampered[i, w, 0] ^= np.uint64(1)
    for i in range(2, n, 64):                             # a non-canonical word: + p where it still fits 256 bits, else 2^256 - 1
        v = oracle_lib.int_of(tampered[i, 0]) + P
        tampered[i, 0] = CM.limbs(v if v < (1 << 256) else (1 << 256) - 1)
    exp_m, exp_ok = CM.decrypt_batch(tampered, keys, nonces, m, oracle.perm_batch)
    assert 0 < int((exp_ok == 0).sum()) < n
    s = HS.Script("sponge")
    s.buf("msgs", msgs.tobytes())
    s.buf("keys", keys.tobytes())
    s.buf("nonces", nonces.tobytes())
    s.buf("dom", limbs(CM.DOMAIN_MONT))
    s.fill("c", 32 * n * (m + 1), 0xFF)
    s.call("hades252_cipher_encrypt_dev", "msgs", "keys", "nonces", n, m, "dom", "c", None)
    s.dump("c")
    s.buf("t", tampered.tobytes())
    s.fill("back", 32 * n * m, 0xFF)
    s.fill("ok", n, 0xFF)
    s.zero("rej", 4)
    s.call("hades252_cipher_decrypt_dev", "t", "keys", "nonces", n, m, "dom", "back", "ok", "rej", None)
    s.fill("back2", 32 * n * m, 0xFF)
    s.fill("ok2", n, 0xFF)
    s.call("hades252_cipher_decrypt_dev", "c", "keys", "nonces", n, m, "dom", "back2", "ok2", "rej", None)
    for b in ("back", "ok", "rej", "back2", "ok2"):
        s.dump(b)
    r = s.run(timeout=600)                               # measured: 3 s
    assert [rc for _, rc in r.rc] == [0, 0, 0]
    assert (u64(r.out["c"]).reshape(exp_c.shape) == exp_c).all()
    assert (u64(r.out["back"]).reshape(exp_m.shape) == exp_m).all()
    assert (np.frombuffer(r.out["ok"], dtype=np.uint8) == exp_ok).all()
    assert int(np.frombuffer(r.out["rej"], dtype=np.int32)[0]) == int((exp_ok == 0).sum())      # the round trip adds none
    assert (u64(r.out["back2"]).reshape(msgs.shape) == msgs).all()
    assert (np.frombuffer(r.out["ok2"], dtype=np.uint8) == 1).all()


# ---- duplex sponge ----------------------------------------------------------------------------------------------------
SAFE_PATTERNS = [[A(1), Q(1)], [A(5), Q(1)], [A(3), Q(2), A(2), Q(1)], [A(2), A(1), Q(5), A(5), Q(1)], [A(6), Q(7)]]


def calls_buf(pattern):
    return np.array(SM.encode(pattern), dtype=np.uint32).tobytes()


def test_duplex_sponge_one_shot_and_streaming(oracle):
    n = N_LANE_CIPHER
    tag = S.to_mont(0x1234)
    s = HS.Script("sponge")
    s.buf("tag", limbs(tag))
    want = {}
    for k, pat in enumerate(SAFE_PATTERNS):
        n_in, n_out = SM.words_in(pat), SM.words_out(pat)
        inp = edge_scalars(n * n_in, 400 + k).reshape(n, n_in, 4)
        want[k] = SM.run_batch(pat, inp, tag, oracle.perm_batch)
        s.buf("in%d" % k, inp.tobytes())
        s.buf("calls%d" % k, calls_buf(pat))
        s.fill("out%d" % k, 32 * n * n_out, 0xFF)
        s.call("hades252_safe_hash_dev", "in%d" % k, n, "calls%d" % k, len(pat), "tag", "out%d" % k, None)
        s.dump("out%d" % k)
        # the same pattern call by call over the streaming entry points
        s.fill("st%d" % k, 160 * n, 0xFF)
        s.zero("cur%d" % k, 4)
        s.call("hades252_sponge_init_dev", "st%d" % k, n, "tag", None)
        at, j = 0, 0
        for kind, ln in pat:
            if kind == "absorb":
                s.buf("si%d_%d" % (k, j), np.ascontiguousarray(inp[:, at:at + ln]).tobytes())
                s.call("hades252_safe_absorb_dev", "st%d" % k, n, "si%d_%d" % (k, j), ln, "cur%d" % k, None)
                at += ln
            else:
                s.fill("so%d_%d" % (k, j), 32 * n * ln, 0xFF)
                s.call("hades252_safe_squeeze_dev", "st%d" % k, n, ln, "so%d_%d" % (k, j), "cur%d" % k, None)
                s.dump("so%d_%d" % (k, j))
            j += 1
    r = s.run(timeout=900)                               # measured: 13 s
    assert all(rc == 0 for _, rc in r.rc)
    for k, pat in enumerate(SAFE_PATTERNS):
        assert (u64(r.out["out%d" % k]).reshape(want[k].shape) == want[k]).all(), pat
        pieces = [u64(r.out["so%d_%d" % (k, j)]).reshape(n, ln, 4) for j, (kind, ln) in enumerate(pat) if kind == "squeeze"]
        assert (np.concatenate(pieces, axis=1) == want[k]).all(), pat


def test_duplex_sponge_rejects_bad_patterns():
    s = HS.Script("sponge")
    s.buf("tag", limbs(1))
    s.zero("in", 32 * 8)
    s.zero("out", 32 * 8)
    for k, pat in enumerate([[Q(1)], [A(1)], [A(1), Q(0)], []]):
        s.buf("calls%d" % k, calls_buf(pat) or b"\0\0\0\0")
        s.call("hades252_safe_hash_dev", "in", 1, "calls%d" % k, len(pat), "tag", "out", None)
    r = s.run(timeout=60)                                # measured: 0.3 s
    assert [rc for _, rc in r.rc] == [-1] * 4


# ---- chain witnesses (one chain per lane whatever the batch size) -------------------------------------------------------
def assert_wires(r, inputs_name, wires_name):
    """the defining property of every chain witness: wires == hades252_perm_witness_dev(inputs), byte for byte"""
    assert r.out[wires_name] == r.out[wires_name + "_ref"], wires_name


def add_ref_witness(s, inputs_name, wires_name, n_records):
    s.fill(wires_name + "_ref", WIRES * 32 * n_records, 0xFF)
    s.call("hades252_perm_witness_dev", inputs_name, wires_name + "_ref", n_records, None)
    s.dump(wires_name + "_ref")


def test_sponge_and_duplex_sponge_witnesses(oracle):
    n = 70                                               # two waves, ragged
    tag = CAP
    s = HS.Script("witness")
    s.buf("tag", limbs(tag))
    # sponge, pad mode 0, 6 words: [absorb(6), squeeze(1)] with the capacity as tag
    msgs = edge_scalars(n * 6, 500).reshape(n, 6, 4)
    sp_in, sp_out, _ = SW.batch_inputs([A(6), Q(1)], msgs, tag, oracle.perm_batch)
    s.buf("msgs", msgs.tobytes())
    s.fill("sp_inputs", 160 * 2 * n, 0xFF)
    s.fill("sp_wires", WIRES * 32 * 2 * n, 0xFF)
    s.fill("sp_dig", 32 * n, 0xFF)
    s.call("hades252_sponge_blocks", 6, 0)
    s.call("hades252_sponge_witness_dev", "msgs", n, 6, "tag", 0, "sp_inputs", "sp_wires", "sp_dig", None)
    for b in ("sp_inputs", "sp_wires", "sp_dig"):
        s.dump(b)
    add_ref_witness(s, "sp_inputs", "sp_wires", 2 * n)
    # duplex sponge, one-shot, and the same pattern cut into streaming witness calls
    pat = [A(3), Q(2), A(2), Q(1)]
    steps = SM.perms_closed_form(pat)
    inp = edge_scalars(n * 5, 501).reshape(n, 5, 4)
    sf_in, sf_out, sf_state = SW.batch_inputs(pat, inp, tag, oracle.perm_batch)
    assert sf_in.shape[0] == steps
    s.buf("in", inp.tobytes())
    s.buf("calls", calls_buf(pat))
    s.fill("sf_inputs", 160 * steps * n, 0xFF)
    s.fill("sf_wires", WIRES * 32 * steps * n, 0xFF)
    s.fill("sf_out", 32 * 3 * n, 0xFF)
    s.call("hades252_safe_witness_dev", "in", n, "calls", len(pat), "tag", "sf_inputs", "sf_wires", "sf_out", None)
    for b in ("sf_inputs", "sf_wires", "sf_out"):
        s.dump(b)
    add_ref_witness(s, "sf_inputs", "sf_wires", steps * n)
    s.fill("st", 160 * n, 0xFF)
    s.zero("cur", 4)
    s.zero("step", 8)
    s.fill("ss_inputs", 160 * steps * n, 0xFF)
    s.fill("ss_wires", WIRES * 32 * steps * n, 0xFF)
    s.call("hades252_sponge_init_dev", "st", n, "tag", None)
    at = 0
    for j, (kind, ln) in enumerate(pat):
        if kind == "absorb":
            s.buf("si%d" % j, np.ascontiguousarray(inp[:, at:at + ln]).tobytes())
            s.call("hades252_safe_absorb_witness_dev", "st", n, "si%d" % j, ln, "cur", "ss_inputs", "ss_wires", steps, "step",
                   None)
            at += ln
        else:
            s.fill("so%d" % j, 32 * n * ln, 0xFF)
            s.call("hades252_safe_squeeze_witness_dev", "st", n, ln, "so%d" % j, "cur", "ss_inputs", "ss_wires", steps, "step",
                   None)
            s.dump("so%d" % j)
    for b in ("ss_inputs", "ss_wires", "step", "st"):
        s.dump(b)
    r = s.run(timeout=900)                               # measured: 10 s
    assert r.rc[0] == ("hades252_sponge_blocks", 2) and all(rc == 0 for _, rc in r.rc[1:])
    assert (u64(r.out["sp_inputs"]).reshape(sp_in.shape) == sp_in).all()
    assert (u64(r.out["sp_dig"]) == oracle.sponge(msgs.reshape(-1), 6, tag, 0)).all()
    assert_wires(r, "sp_inputs", "sp_wires")
    assert (u64(r.out["sf_inputs"]).reshape(sf_in.shape) == sf_in).all()
    assert (u64(r.out["sf_out"]).reshape(sf_out.shape) == sf_out).all()
    assert_wires(r, "sf_inputs", "sf_wires")
    assert r.out["ss_inputs"] == r.out["sf_inputs"] and r.out["ss_wires"] == r.out["sf_wires"]
    assert int(np.frombuffer(r.out["step"], dtype=np.uint64)[0]) == steps
    assert (u64(r.out["st"]).reshape(sf_state.shape) == sf_state).all()
    got = np.concatenate([u64(r.out["so%d" % j]).reshape(n, ln, 4) for j, (kind, ln) in enumerate(pat) if kind == "squeeze"],
                         axis=1)
    assert (got == sf_out).all()


def test_cipher_witnesses(oracle):
    n, m = 70, 5
    steps = CM.blocks(m) + 1
    msgs, keys, nonces = cipher_inputs(n, m, 510)
    exp_c = CM.encrypt_batch(msgs, keys, nonces, m, oracle.perm_batch)
    # the input states of the chain: the start state, then each permutation's output with the block's words added
    st = CM._start(keys, nonces, m, CM.DOMAIN_MONT)
    exp_in = [st.copy()]
    for b in range(CM.blocks(m)):
        st = CM._permute(st, oracle.perm_batch)
        for j in range(min(4, m - 4 * b)):
            st[:, 1 + j] = CM.fr_add(st[:, 1 + j], msgs[:, 4 * b + j])
        exp_in.append(st.copy())
    exp_in = np.array(exp_in, dtype=np.uint64)
    tampered = exp_c.copy()
    tampered[3, m, 0] ^= np.uint64(1)
    tampered[5, 1, 0] ^= np.uint64(2)
    exp_m, exp_ok = CM.decrypt_batch(tampered, keys, nonces, m, oracle.perm_batch)
    s = HS.Script("witness")
    for name, a in (("msgs", msgs), ("keys", keys), ("nonces", nonces), ("t", tampered)):
        s.buf(name, a.tobytes())
    s.buf("dom", limbs(CM.DOMAIN_MONT))
    for tag in ("e", "d"):
        s.fill(tag + "_inputs", 160 * steps * n, 0xFF)
        s.fill(tag + "_wires", WIRES * 32 * steps * n, 0xFF)
    s.fill("c", 32 * n * (m + 1), 0xFF)
    s.fill("back", 32 * n * m, 0xFF)
    s.fill("ok", n, 0xFF)
    s.zero("rej", 4)
    s.call("hades252_cipher_perms", m)
    s.call("hades252_cipher_encrypt_witness_dev", "msgs", "keys", "nonces", n, m, "dom", "e_inputs", "e_wires", "c", None)
    s.call("hades252_cipher_decrypt_witness_dev", "t", "keys", "nonces", n, m, "dom", "d_inputs", "d_wires", "back", "ok", "rej",
           None)
    for b in ("e_inputs", "e_wires", "d_inputs", "d_wires", "c", "back", "ok", "rej"):
        s.dump(b)
    add_ref_witness(s, "e_inputs", "e_wires", steps * n)
    add_ref_witness(s, "d_inputs", "d_wires", steps * n)
    r = s.run(timeout=900)                               # measured: 8 s
    assert r.rc[0] == ("hades252_cipher_perms", steps) and all(rc == 0 for _, rc in r.rc[1:])
    assert (u64(r.out["e_inputs"]).reshape(exp_in.shape) == exp_in).all()
    assert (u64(r.out["c"]).reshape(exp_c.shape) == exp_c).all()
    assert_wires(r, "e_inputs", "e_wires")
    assert_wires(r, "d_inputs", "d_wires")
    assert (u64(r.out["back"]).reshape(exp_m.shape) == exp_m).all()
    assert (np.frombuffer(r.out["ok"], dtype=np.uint8) == exp_ok).all() and int((exp_ok == 0).sum()) == 2
    assert int(np.frombuffer(r.out["rej"], dtype=np.int32)[0]) == 2
    d_in = u64(r.out["d_inputs"]).reshape(exp_in.shape)
    untouched = np.ones(n, dtype=bool)
    untouched[[3, 5]] = False
    assert (d_in[:, untouched] == exp_in[:, untouched]).all()            # decrypt(encrypt(m)) records the encrypt witness


def test_merkle_open_witness(oracle):
    arity, n_leaves, nq = 4, 4 * 16 + 3, 70
    leaves = edge_scalars(n_leaves, 520)
    depth = 4
    pad = edge_scalars(depth, 521).reshape(depth, 4)
    levels = oracle.merkle_tree(leaves, arity, TAG[arity], 1, pad)
    assert len(levels) == depth
    rng = np.random.default_rng(522)
    idx = rng.integers(0, n_leaves, size=nq, dtype=np.uint64)
    idx[:3] = [0, n_leaves - 1, n_leaves]                 # the last one lies outside the tree
    nodes = [leaves.reshape(-1, 4)] + [l.reshape(-1, 4) for l in levels[:-1]]
    exp = np.zeros((depth, nq, 5, 4), dtype=np.uint64)
    for q, i in enumerate(idx):
        if i >= n_leaves:
            continue
        node = int(i)
        for l in range(depth):
            exp[l, q, 0] = limbs_of(TAG[arity])
            first = node - node % arity
            for c in range(arity):
                exp[l, q, 1 + c] = nodes[l][first + c] if first + c < nodes[l].shape[0] else pad[l]
            node //= arity
    s = HS.Script("witness")
    s.buf("leaves", leaves.tobytes())
    s.buf("tree", np.concatenate(levels).tobytes())
    s.buf("pad", pad.tobytes())
    s.buf("idx", idx.tobytes())
    s.buf("tag", limbs(TAG[arity]))
    s.fill("mo_inputs", 160 * depth * nq, 0xFF)
    s.fill("mo_wires", WIRES * 32 * depth * nq, 0xFF)
    s.zero("bad", 4)
    s.call("hades252_merkle_open_witness_dev", "leaves", "tree", n_leaves, arity, "tag", "pad", "idx", nq, "mo_inputs",
           "mo_wires", "bad", None)
    for b in ("mo_inputs", "mo_wires", "bad"):
        s.dump(b)
    add_ref_witness(s, "mo_inputs", "mo_wires", depth * nq)
    r = s.run(timeout=900)                               # measured: 8 s
    assert all(rc == 0 for _, rc in r.rc)
    assert (u64(r.out["mo_inputs"]).reshape(exp.shape) == exp).all()
    assert int(np.frombuffer(r.out["bad"], dtype=np.int32)[0]) == 1
    assert_wires(r, "mo_inputs", "mo_wires")


# ---- the DPP forms of hades_lanes.hpp: one chain per wave (with a helper wave, and without) and per 16-lane row ----------
# A permutation of one emulated block costs seconds (tests/hostsim/hip/hip_runtime.h), a chain several of them: the sizes
# are the smallest that reach every role of a block -- 1 (a lone state wave and its helper), 3 (a full helped block), 4 (a
# second block with idle waves), 5 for the unhelped form (a second block whose other waves return at once), 4 and 5 for the
# rows form (a full wave, a second wave with one row in use) -- and the longest chain sits where it is cheapest.  The
# helped form is what the dispatch gives these sizes; the unhelped form (769 .. 1 024) and the rows form (1 025 .. 4 096)
# are launched with their call sites' geometry by the form_* launchers (tests/hostsim/hostsim_main.cpp, namespace forms).
HELPED, UNHELPED, PER_ROW = 0, 1, 2
assert 5 < FORM_SIZES["lanes"][0] < FORM_SIZES["rows"][0] and FORM_SIZES["lanes_helped"][0] == 1


def clean(r):
    return "over_budget" not in r.stdout and "not_emulated" not in r.stdout


@pytest.mark.parametrize("form,lens,pad", [(HELPED, [3], 0), (HELPED, [5, 5, 5], 1), (HELPED, [9, 2, 5, 3], 1),
                                           (UNHELPED, [5, 0, 2, 1, 4], 1), (PER_ROW, [9, 0, 5, 3], 1), (PER_ROW, [3] * 5, 0)],
                         ids=["helped-1", "helped-3", "helped-4-three_blocks-out_of_pool", "unhelped-5", "rows-4-three_blocks",
                              "rows-5"])
def test_sponge_one_message_per_wave_and_per_row(oracle, form, lens, pad):
    """k_sponge_lanes<true> / <false> and k_sponge_rows: equal lengths go in as a fixed-length batch, unequal ones as a
    ragged one over a pool (a message of three blocks beside shorter ones: every wave of a helped block runs the block's
    maximum and latches its digest after its own last block); in the helped ragged case message 1 lies outside the pool,
    is counted and hashed as the empty message."""
    n = len(lens)
    assert sponge_form(n) == ("k_sponge_lanes<true>",) or form != HELPED
    fixed = len(set(lens)) == 1
    n_pool = sum(lens) + 3
    pool = edge_scalars(n_pool, 700 + n + pad)
    offs = np.cumsum([0] + lens[:-1]).astype(np.uint64)
    la = np.array(lens, dtype=np.uint64)
    bad = 0
    if form == HELPED and not fixed:
        offs[1], bad = n_pool - 1, 1                      # two words from the last word of the pool
    so, sl = offs.copy(), la.copy()
    if bad:
        so[1], sl[1] = 0, 0
    s = HS.Script("sponge")
    s.buf("cap", limbs(CAP))
    s.fill("dig", 32 * n, 0xFF)
    s.zero("bad", 4)
    if fixed:
        msgs = pool[:4 * n * lens[0]]
        s.buf("msgs", msgs.tobytes())
        exp = oracle.sponge(msgs, lens[0], CAP, pad)
        if form == HELPED:
            s.call("hades252_sponge_hash_dev", "msgs", n, lens[0], "cap", pad, "dig", None)
        else:
            s.call("form_sponge", "msgs", None, None, n, lens[0], "cap", pad, "dig", n * lens[0], None, form)
    else:
        s.buf("pool", pool.tobytes())
        s.buf("offs", offs.tobytes())
        s.buf("lens", la.tobytes())
        exp = oracle.sponge_var(pool, so, sl, CAP, pad)
        if form == HELPED:
            s.call("hades252_sponge_hash_var_dev", "pool", n_pool, "offs", "lens", n, "cap", pad, "dig", "bad", None)
        else:
            s.call("form_sponge", "pool", "offs", "lens", n, 0, "cap", pad, "dig", n_pool, "bad", form)
    s.dump("dig")
    s.dump("bad")
    r = s.run(timeout=900)                               # measured: 2 .. 22 s
    assert [rc for _, rc in r.rc] == [0] and clean(r)
    assert int(np.frombuffer(r.out["bad"], dtype=np.int32)[0]) == bad
    assert (u64(r.out["dig"]) == exp).all()


@pytest.mark.parametrize("form,n,blocks", [(HELPED, 1, 3), (HELPED, 3, 2), (HELPED, 4, 1), (UNHELPED, 5, 1), (PER_ROW, 4, 1),
                                           (PER_ROW, 5, 2)])
def test_sponge_streaming_one_state_per_wave_and_per_row(oracle, form, n, blocks):
    """k_sponge_absorb_lanes<true> / <false> and k_sponge_absorb_rows between init and squeeze: the digest of the
    zero-filled fixed-length sponge over the same words, and the whole state written back."""
    msg_len = 4 * blocks - 1
    msgs = edge_scalars(n * msg_len, 710 + n).reshape(n, msg_len, 4)
    blk = np.zeros((n, 4 * blocks, 4), dtype=np.uint64)
    blk[:, :msg_len] = msgs
    s = HS.Script("sponge")
    s.buf("cap", limbs(CAP))
    s.fill("st", 160 * n, 0xFF)
    s.buf("blk", blk.tobytes())
    s.fill("dig", 32 * n, 0xFF)
    s.call("hades252_sponge_init_dev", "st", n, "cap", None)
    if form == HELPED:
        assert absorb_form(n) == "k_sponge_absorb_lanes<true>"
        s.call("hades252_sponge_absorb_dev", "st", "blk", n, blocks, None)
    else:
        s.call("form_sponge_absorb", "st", "blk", n, blocks, form)
    s.call("hades252_sponge_squeeze_dev", "st", "dig", n, 1, None)
    s.dump("dig")
    s.dump("st")
    r = s.run(timeout=900)                               # measured: 3 .. 12 s
    assert [rc for _, rc in r.rc] == [0, 0, 0] and clean(r)
    assert (u64(r.out["dig"]) == oracle.sponge(msgs.reshape(-1), msg_len, CAP, 0)).all()
    # the state: absorbing block by block with the oracle's permutation
    st = np.zeros((n, 5, 4), dtype=np.uint64)
    st[:, 0] = limbs_of(CAP)
    for b in range(blocks):
        for j in range(4):
            st[:, 1 + j] = CM.fr_add(st[:, 1 + j], blk[:, 4 * b + j])
        st = oracle.perm_batch(st.reshape(-1)).reshape(n, 5, 4)
    assert (u64(r.out["st"]).reshape(n, 5, 4) == st).all()


@pytest.mark.parametrize("form,n,m", [(HELPED, 1, 5), (HELPED, 3, 1), (HELPED, 4, 2), (UNHELPED, 4, 1)])
def test_cipher_one_message_per_wave(oracle, form, n, m):
    """k_cipher_lanes, encrypt and decrypt.  The decrypt launch gets the ciphers with message 0 tampered (its tag when it
    is the only one, else a word), and from two messages on message 1 non-canonical (word 0 + p or 2^256 - 1), message 2
    intact, message 3 with a wrong tag: rejected messages come out as zeros and are counted, the intact one round-trips."""
    msgs, keys, nonces = cipher_inputs(n, m, 720 + n)
    exp_c = CM.encrypt_batch(msgs, keys, nonces, m, oracle.perm_batch)
    t = exp_c.copy()
    t[0, m if n == 1 else 0, 0] ^= np.uint64(1)
    if n > 1:
        v = oracle_lib.int_of(t[1, 0]) + P
        t[1, 0] = CM.limbs(v if v < (1 << 256) else (1 << 256) - 1)
    if n > 3:
        t[3, m, 1] ^= np.uint64(1 << 40)
    exp_m, exp_ok = CM.decrypt_batch(t, keys, nonces, m, oracle.perm_batch)
    assert list(exp_ok) == [0, 0, 1, 0][:n]
    s = HS.Script("sponge")
    for name, a in (("msgs", msgs), ("keys", keys), ("nonces", nonces), ("t", t)):
        s.buf(name, a.tobytes())
    s.buf("dom", limbs(CM.DOMAIN_MONT))
    s.fill("c", 32 * n * (m + 1), 0xFF)
    s.fill("back", 32 * n * m, 0xFF)
    s.fill("ok", n, 0xFF)
    s.zero("rej", 4)
    if form == HELPED:
        s.call("hades252_cipher_encrypt_dev", "msgs", "keys", "nonces", n, m, "dom", "c", None)
        s.call("hades252_cipher_decrypt_dev", "t", "keys", "nonces", n, m, "dom", "back", "ok", "rej", None)
    else:
        s.call("form_cipher", 0, "msgs", "keys", "nonces", n, m, "dom", "c", None, None, form)
        s.call("form_cipher", 1, "t", "keys", "nonces", n, m, "dom", "back", "ok", "rej", form)
    for b in ("c", "back", "ok", "rej"):
        s.dump(b)
    r = s.run(timeout=900)                               # measured: 13 .. 28 s
    assert [rc for _, rc in r.rc] == [0, 0] and clean(r)
    assert (u64(r.out["c"]).reshape(exp_c.shape) == exp_c).all()
    assert (u64(r.out["back"]).reshape(exp_m.shape) == exp_m).all()
    assert (np.frombuffer(r.out["ok"], dtype=np.uint8) == exp_ok).all()
    assert int(np.frombuffer(r.out["rej"], dtype=np.int32)[0]) == int((exp_ok == 0).sum())


def safe_script(s, form, k, pat, inp, n, one_shot, streaming):
    """the calls of pattern `pat` on n sponges: the whole pattern in one launch and / or call by call over the states"""
    n_out = SM.words_out(pat)
    s.buf("in%d" % k, inp.tobytes())
    s.buf("calls%d" % k, calls_buf(pat))
    if one_shot:
        s.fill("out%d" % k, 32 * n * n_out, 0xFF)
        if form == HELPED:
            s.call("hades252_safe_hash_dev", "in%d" % k, n, "calls%d" % k, len(pat), "tag", "out%d" % k, None)
        else:
            s.call("form_safe", "in%d" % k, "out%d" % k, None, n, "calls%d" % k, len(pat), None, "tag", form)
        s.dump("out%d" % k)
    if streaming:
        s.fill("st%d" % k, 160 * n, 0xFF)
        s.zero("cur%d" % k, 4)
        s.call("hades252_sponge_init_dev", "st%d" % k, n, "tag", None)
        at = 0
        for j, (kind, ln) in enumerate(pat):
            one = np.array(SM.encode([(kind, ln)]), dtype=np.uint32).tobytes()
            s.buf("call%d_%d" % (k, j), one)
            if kind == "absorb":
                s.buf("si%d_%d" % (k, j), np.ascontiguousarray(inp[:, at:at + ln]).tobytes())
                if form == HELPED:
                    s.call("hades252_safe_absorb_dev", "st%d" % k, n, "si%d_%d" % (k, j), ln, "cur%d" % k, None)
                else:
                    s.call("form_safe", "si%d_%d" % (k, j), None, "st%d" % k, n, "call%d_%d" % (k, j), 1, "cur%d" % k, None, form)
                at += ln
            else:
                s.fill("so%d_%d" % (k, j), 32 * n * ln, 0xFF)
                if form == HELPED:
                    s.call("hades252_safe_squeeze_dev", "st%d" % k, n, ln, "so%d_%d" % (k, j), "cur%d" % k, None)
                else:
                    s.call("form_safe", None, "so%d_%d" % (k, j), "st%d" % k, n, "call%d_%d" % (k, j), 1, "cur%d" % k, None, form)
                s.dump("so%d_%d" % (k, j))


@pytest.mark.parametrize("form,n,patterns,one_shot,streaming", [
    (HELPED, 1, [0, 1, 2, 3, 4], True, False), (HELPED, 1, [0, 1, 2, 3, 4], False, True), (HELPED, 3, [1], False, True),
    (HELPED, 4, [2], True, False), (UNHELPED, 5, [0], True, True)],
    ids=["helped-1-one_shot", "helped-1-streaming", "helped-3-streaming", "helped-4-one_shot", "unhelped-5-both"])
def test_duplex_sponge_one_sponge_per_wave(oracle, form, n, patterns, one_shot, streaming):
    """k_safe_lanes over the patterns of test_duplex_sponge_one_shot_and_streaming: the whole pattern in one launch (no
    states: from the second sponge of a launch on this is where the kernel used to form states + offset from a null
    pointer) and call by call over the streaming states."""
    tag = S.to_mont(0x1234)
    s = HS.Script("sponge")
    s.buf("tag", limbs(tag))
    want = {}
    for k in patterns:
        pat = SAFE_PATTERNS[k]
        inp = edge_scalars(n * SM.words_in(pat), 730 + 10 * n + k).reshape(n, SM.words_in(pat), 4)
        want[k] = SM.run_batch(pat, inp, tag, oracle.perm_batch)
        safe_script(s, form, k, pat, inp, n, one_shot, streaming)
    r = s.run(timeout=1200)                              # measured: 11 .. 28 s
    assert all(rc == 0 for _, rc in r.rc) and clean(r)
    for k in patterns:
        pat = SAFE_PATTERNS[k]
        if one_shot:
            assert (u64(r.out["out%d" % k]).reshape(want[k].shape) == want[k]).all(), pat
        if streaming:
            pieces = [u64(r.out["so%d_%d" % (k, j)]).reshape(n, ln, 4) for j, (kind, ln) in enumerate(pat) if kind == "squeeze"]
            assert (np.concatenate(pieces, axis=1) == want[k]).all(), pat
