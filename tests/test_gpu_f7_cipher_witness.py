"""GPU tier: the gadget witnesses of the batched Poseidon cipher (hades252_cipher_{encrypt,decrypt}_witness_dev).  The
defining property wires == perm_witness(inputs), byte for byte, on every case; the inputs against the big-integer model
(tests/cipher_witness_model.py, over the C oracle's perm_batch); the side outputs against hades252_cipher_*_dev; sampled
records against the spec's GadgetStrategy wire for wire; guard words, untouched inputs, tampering and non-canonical cipher
words, the round trip (the decrypt witness of encrypt(m) is the encrypt witness of m), a non-default stream, M = MAX_LEN
and 2^18 messages.  Convention of f5 (UNPINNED, include/hades252.h)."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cipher_model as C  # noqa: E402
import cipher_witness_model as CW  # noqa: E402
from cipher_witness_model import P, S  # noqa: E402
from gpu_common import (WIRES, Guarded, assert_wires_are_perm_witness, gadget_check, mont_rows, perm_many_over,  # noqa: E402
                        to_dev, to_host)
from oracle_lib import int_of  # noqa: E402

pytestmark = pytest.mark.gpu

NG = 64                                          # guard bytes behind ok (a byte per message: not Guarded's int64 rows)


def _case(rng, n, m):
    """Canonical integers: n messages of m words (edge values mixed in), keys, nonces."""
    kinds = [lambda: 0, lambda: P - 1, lambda: rng.randrange(P)]
    msgs = [[rng.choice(kinds)() if i % 4 == 3 else kinds[i % 3]() for _ in range(m)] for i in range(n)]
    keys = [[rng.randrange(P), rng.randrange(P)] for _ in range(n)]
    nonces = [rng.randrange(P) for _ in range(n)]
    return msgs, keys, nonces


def _run_encrypt(torch, hades_lib, dm, dk, dn, n, m, dom):
    S_ = CW.cipher_perms(m)
    inputs, wires = Guarded(torch, (5 * S_ * n * 4,)), Guarded(torch, (WIRES * S_ * n * 4,))
    ciphers = Guarded(torch, (n * (m + 1) * 4,))
    rc = hades_lib.hades252_cipher_encrypt_witness_dev(dm.data_ptr(), dk.data_ptr(), dn.data_ptr(), n, m, dom,
                                                       inputs.ptr, wires.ptr, ciphers.ptr, None)
    assert rc == 0
    return inputs.check((n, m)), wires.check((n, m)), ciphers.check((n, m))      # guards whole, every word written


def _run_decrypt(torch, hades_lib, dc, dk, dn, n, m, dom, rej0=5):
    S_ = CW.cipher_perms(m)
    inputs, wires = Guarded(torch, (5 * S_ * n * 4,)), Guarded(torch, (WIRES * S_ * n * 4,))
    msgs = Guarded(torch, (n * m * 4,))
    ok = torch.full((n + NG,), 0x77, dtype=torch.uint8, device="cuda")
    rej = torch.full((1,), rej0, dtype=torch.int32, device="cuda")          # the entry point ADDS to it
    rc = hades_lib.hades252_cipher_decrypt_witness_dev(dc.data_ptr(), dk.data_ptr(), dn.data_ptr(), n, m, dom,
                                                       inputs.ptr, wires.ptr, msgs.ptr, ok.data_ptr(), rej.data_ptr(), None)
    assert rc == 0
    # guards whole, every word written: a rejected lane's message too (zeroed, and zero is not the sentinel)
    got = inputs.check((n, m)), wires.check((n, m)), msgs.check((n, m))
    assert bool((ok[n:] == 0x77).all())
    return got + (ok[:n], int(rej.item()) - rej0)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 9])
def test_cipher_witness_against_model_and_perm_witness(torch_cuda, H, hades_lib, oracle, m):
    torch = torch_cuda
    S_ = CW.cipher_perms(m)
    assert hades_lib.hades252_cipher_perms(m) == S_
    for n in (1, 63, 64, 65, 257):
        rng = random.Random(100 * m + n)
        msgs, keys, nonces = _case(rng, n, m)
        dom_int = rng.choice([C.DOMAIN, rng.randrange(P)])
        dom = H._tag_arr(S.to_mont(dom_int))
        hm = mont_rows([v for x in msgs for v in x])
        hk, hn = mont_rows([v for k in keys for v in k]), mont_rows(nonces)
        dm, dk, dn = to_dev(torch, hm), to_dev(torch, hk), to_dev(torch, hn)
        # ---- encrypt ----
        e_in, e_wires, e_c = _run_encrypt(torch, hades_lib, dm, dk, dn, n, m, dom)
        assert (to_host(dm) == hm.reshape(-1)).all() and (to_host(dk) == hk.reshape(-1)).all()
        assert (to_host(dn) == hn.reshape(-1)).all()
        exp_in, exp_c = CW.encrypt_inputs(msgs, keys, nonces, dom_int, perm_many_over(oracle))
        got_in = to_host(e_in).reshape(S_, n, 5, 4)
        assert (got_in == mont_rows([v for step in exp_in for st in step for v in st]).reshape(S_, n, 5, 4)).all(), n
        assert_wires_are_perm_witness(torch, H, e_in, e_wires)
        ref_c = torch.empty((n, m + 1, 4), dtype=torch.int64, device="cuda")
        assert hades_lib.hades252_cipher_encrypt_dev(dm.data_ptr(), dk.data_ptr(), dn.data_ptr(), n, m, dom,
                                                     ref_c.data_ptr(), None) == 0
        assert torch.equal(e_c.view(n, m + 1, 4), ref_c), n
        assert (to_host(ref_c).reshape(n, m + 1, 4) == mont_rows([v for c in exp_c for v in c]).reshape(n, m + 1, 4)).all()
        wires_h = to_host(e_wires).reshape(WIRES, S_, n, 4)
        pairs = {(0, 0), (S_ - 1, n - 1), (rng.randrange(S_), rng.randrange(n))}
        gadget_check(wires_h, got_in, sorted(pairs))
        # ---- decrypt of the encryption: the same witness, the messages back ----
        c_before = ref_c.clone()
        d_in, d_wires, d_m, d_ok, d_rej = _run_decrypt(torch, hades_lib, ref_c, dk, dn, n, m, dom)
        assert torch.equal(ref_c, c_before)
        assert torch.equal(d_in, e_in) and torch.equal(d_wires, e_wires), n
        assert d_rej == 0 and bool((d_ok == 1).all()) and torch.equal(d_m, dm.view(-1)), n
        if n == 65:                                   # the Python layer: same bytes, shapes [972, S, n, 4] / [S, n, 5, 4]
            pw, pi, pc = H.cipher_encrypt_witness(dm.view(n, m, 4), dk.view(n, 2, 4), dn.view(n, 4), m, S.to_mont(dom_int))
            assert tuple(pw.shape) == (WIRES, S_, n, 4) and tuple(pi.shape) == (S_, n, 5, 4)
            assert tuple(pc.shape) == (n, m + 1, 4)
            assert torch.equal(pw.view(-1), e_wires) and torch.equal(pi.view(-1), e_in) and torch.equal(pc, ref_c)
            qw, qi, qm, qok, qrej = H.cipher_decrypt_witness(ref_c, dk, dn, m, S.to_mont(dom_int))
            assert tuple(qw.shape) == (WIRES, S_, n, 4) and tuple(qi.shape) == (S_, n, 5, 4)
            assert tuple(qm.shape) == (n, m, 4) and tuple(qok.shape) == (n,) and qok.dtype == torch.uint8
            assert torch.equal(qw.view(-1), e_wires) and torch.equal(qi.view(-1), e_in)
            assert torch.equal(qm.view(-1), dm.view(-1)) and bool((qok == 1).all()) and qrej == 0


@pytest.mark.parametrize("n,m", [(300, 2), (257, 5), (65, 9)])
def test_decrypt_witness_tampered_and_non_canonical(torch_cuda, H, hades_lib, oracle, n, m):
    """A wrong tag, a wrong word, and non-canonical words (c + p, c + 2p, 2^256 - 1) reject exactly their messages: ok, the
    count and the zeroed messages are hades252_cipher_decrypt_dev's, the inputs are the model's (every word reduced, so
    canonical) and the wires are perm_witness(inputs)."""
    torch = torch_cuda
    S_ = CW.cipher_perms(m)
    rng = random.Random(n * 31 + m)
    msgs, keys, nonces = _case(rng, n, m)
    hk, hn = mont_rows([v for k in keys for v in k]), mont_rows(nonces)
    dk, dn = to_dev(torch, hk), to_dev(torch, hn)
    dom = H._tag_arr(H.CIPHER_DOMAIN)
    c = to_host(H.cipher_encrypt(to_dev(torch, mont_rows([v for x in msgs for v in x])), dk, dn, m)).reshape(n, m + 1, 4)
    c = c.copy()
    raw = [[int_of(w) for w in row] for row in c]                # the 256-bit words as stored
    kinds = ["tag", "word", "p", "2p", "max"]
    bad = {}
    for i in sorted(rng.sample(range(n), 5 * 6)):
        kind = kinds[len(bad) % len(kinds)]
        k = m if kind == "tag" else rng.randrange(m + 1)
        v = raw[i][k]
        if kind in ("tag", "word"):
            v = (v + rng.randrange(1, P)) % P
        elif kind == "p":
            v = v + P
        elif kind == "2p":
            v = v + 2 * P if v + 2 * P < 1 << 256 else v + P
        else:
            v = (1 << 256) - 1
        raw[i][k] = v
        c[i, k] = C.limbs(v)
        bad[i] = kind
    dc = to_dev(torch, c)
    d_in, d_wires, d_m, d_ok, d_rej = _run_decrypt(torch, hades_lib, dc, dk, dn, n, m, dom)
    assert (to_host(dc) == c.reshape(-1)).all()                   # the ciphers are untouched
    # verdicts and messages: those of the cipher itself
    ref_m, ref_ok, ref_rej = H.cipher_decrypt(dc, dk, dn, m)
    assert torch.equal(d_m.view(n, m, 4), ref_m) and torch.equal(d_ok, ref_ok) and d_rej == ref_rej
    want_ok = np.ones(n, dtype=np.uint8)
    want_ok[list(bad)] = 0
    assert (d_ok.cpu().numpy() == want_ok).all() and d_rej == len(bad)
    got_m = to_host(d_m).reshape(n, m, 4)
    assert (got_m[list(bad)] == 0).all()
    keep = want_ok == 1
    assert (got_m[keep] == mont_rows([v for x in msgs for v in x]).reshape(n, m, 4)[keep]).all()
    # inputs: the model's, every word canonical.  The model takes a stored word w = mont(v) + k p as the integer v + k p: the
    # field element v, and not canonical when k > 0
    ints = [[S.from_mont(w % P) + (w // P) * P for w in row] for row in raw]
    exp_in, exp_m, exp_ok = CW.decrypt_inputs(ints, keys, nonces, C.DOMAIN, perm_many_over(oracle))
    assert [int(x) for x in exp_ok] == want_ok.tolist()
    got_in = to_host(d_in).reshape(S_, n, 5, 4)
    assert (got_in == mont_rows([v for step in exp_in for st in step for v in st]).reshape(S_, n, 5, 4)).all()
    assert C.canonical(got_in).all()
    assert_wires_are_perm_witness(torch, H, d_in, d_wires)
    gadget_check(to_host(d_wires).reshape(WIRES, S_, n, 4), got_in, sorted({(S_ - 1, i) for i in list(bad)[:3]}))
    # side outputs are optional: NULL msgs / ok / counter write the same witness
    bare_in, bare_w = torch.empty_like(d_in), torch.empty_like(d_wires)
    assert hades_lib.hades252_cipher_decrypt_witness_dev(dc.data_ptr(), dk.data_ptr(), dn.data_ptr(), n, m, dom,
                                                         bare_in.data_ptr(), bare_w.data_ptr(), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(bare_in, d_in) and torch.equal(bare_w, d_wires)


def test_non_default_stream_and_max_len(torch_cuda, H, oracle):
    """M = HADES252_CIPHER_MAX_LEN (257 dependent permutations per message) at small n, on a side stream."""
    torch = torch_cuda
    from hades252_amd import _lib
    m = _lib.CIPHER_MAX_LEN
    S_ = CW.cipher_perms(m)
    for n in (1, 3):
        msgs = to_dev(torch, oracle.gen_b(11 + n, n * m)).view(n, m, 4)
        keys = to_dev(torch, oracle.gen_b(1 << 20, 2 * n)).view(n, 2, 4)
        nonces = to_dev(torch, oracle.gen_b(1 << 21, n)).view(n, 4)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            wires, inputs, ciphers = H.cipher_encrypt_witness(msgs, keys, nonces, m)
            dwires, dinputs, dmsgs, ok, rej = H.cipher_decrypt_witness(ciphers, keys, nonces, m)
        side.synchronize()
        assert tuple(wires.shape) == (WIRES, S_, n, 4)
        assert torch.equal(ciphers, H.cipher_encrypt(msgs, keys, nonces, m))
        assert torch.equal(wires.view(WIRES, S_ * n, 4), H.perm_witness(inputs.view(S_ * n, 20)))
        assert torch.equal(dwires, wires) and torch.equal(dinputs, inputs)
        assert torch.equal(dmsgs, msgs) and bool((ok == 1).all()) and rej == 0
        # step s >= 1 absorbs message words 4 (s - 1) .. 4 (s - 1) + 3: the cipher words
        assert torch.equal(inputs[1:, :, 1:].permute(1, 0, 2, 3).reshape(n, 4 * (S_ - 1), 4), ciphers[:, :m])
        assert torch.equal(wires[WIRES - 9 + 2, S_ - 1], ciphers[:, m])                 # the tag: r2[1] of the last record


def test_cipher_witness_at_scale(torch_cuda, H):
    """2^18 messages x M = 2: 2^19 permutations (16.3 GB of wires, as much again for the reference), compared on the device:
    wires == perm_witness(inputs), ciphers == cipher_encrypt, and the decrypt witness of the ciphers is the same witness."""
    torch = torch_cuda
    n, m = 1 << 18, 2
    S_ = CW.cipher_perms(m)
    msgs = H.gen_b(n * m, "cuda", first_elem=1 << 32).view(n, m, 4)
    keys = H.gen_b(2 * n, "cuda", first_elem=1 << 33).view(n, 2, 4)
    nonces = H.gen_b(n, "cuda", first_elem=1 << 34).view(n, 4)
    wires, inputs, ciphers = H.cipher_encrypt_witness(msgs, keys, nonces, m)
    assert torch.equal(ciphers, H.cipher_encrypt(msgs, keys, nonces, m))
    ref = H.perm_witness(inputs.view(S_ * n, 20))
    assert torch.equal(wires.view(WIRES, S_ * n, 4), ref)
    del ref
    dwires, dinputs, dmsgs, ok, rej = H.cipher_decrypt_witness(ciphers, keys, nonces, m)
    assert rej == 0 and bool((ok == 1).all()) and torch.equal(dmsgs, msgs)
    assert torch.equal(dinputs, inputs)
    assert torch.equal(dwires, wires)
