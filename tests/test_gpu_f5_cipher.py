"""GPU tier, row f5 (beyond SURVEY section 8): the batched Poseidon cipher (hades252_cipher_*) against its model
(tests/cipher_model.py, over the C oracle's perm_batch) -- both kernel forms, every residue of M mod 4, edge values, round
trips, tampering, non-canonical cipher words, guard words, a non-default stream, the host entry points, 2^24 messages.
Convention: dusk-poseidon's PoseidonCipher as recalled, UNPINNED (include/hades252.h)."""
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cipher_model as C  # noqa: E402
from gpu_common import to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

P = C.P
NS = [1, 3, 64, 1024, 1025, 4099, 65537]        # one per wave (<= 1024, helped <= 768) and one per lane, ragged waves


def _inputs(oracle, n, m, seed):
    msgs = oracle.gen_b(seed * 1000003, n * m).reshape(n, m, 4)
    keys = oracle.gen_b(seed * 1000003 + 400_000_000, 2 * n).reshape(n, 2, 4)
    nonces = oracle.gen_b(seed * 1000003 + 800_000_000, n).reshape(n, 4)
    return msgs, keys, nonces


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 9])
def test_encrypt_decrypt_against_the_model(torch_cuda, H, oracle, m):
    torch = torch_cuda
    for n in NS:
        msgs, keys, nonces = _inputs(oracle, n, m, 7 * m + n)
        dm, dk, dn = to_dev(torch, msgs), to_dev(torch, keys), to_dev(torch, nonces)
        c = H.cipher_encrypt(dm, dk, dn, m)
        exp = C.encrypt_batch(msgs, keys, nonces, m, oracle.perm_batch)
        assert (to_host(c).reshape(n, m + 1, 4) == exp).all(), (n, m)
        back, ok, rej = H.cipher_decrypt(c, dk, dn, m)
        assert rej == 0 and bool((ok == 1).all()), (n, m)
        assert torch.equal(back.view(-1), dm.view(-1)), (n, m)


def test_edge_values_and_borrowing_subtractions(torch_cuda, H, oracle):
    """0, 1, p - 1, p - 2 as raw words everywhere; a message word p - 1 makes its cipher word the keystream minus one, so
    decryption's subtraction borrows (and a message word 0 makes the cipher word equal to the keystream)."""
    torch = torch_cuda
    edge = [0, 1, P - 1, P - 2, (1 << 254) - 1]
    for n, m in ((5, 2), (3000, 5), (1500, 4)):
        rng = random.Random(n * m)
        def word():
            return C.limbs(rng.choice(edge) if rng.random() < 0.7 else rng.randrange(P))
        msgs = np.array([[word() for _ in range(m)] for _ in range(n)], dtype=np.uint64)
        keys = np.array([[word(), word()] for _ in range(n)], dtype=np.uint64)
        nonces = np.array([word() for _ in range(n)], dtype=np.uint64)
        c = H.cipher_encrypt(to_dev(torch, msgs), to_dev(torch, keys), to_dev(torch, nonces), m)
        exp = C.encrypt_batch(msgs, keys, nonces, m, oracle.perm_batch)
        got = to_host(c).reshape(n, m + 1, 4)
        assert (got == exp).all()
        borrows = sum(C.int_of(got[i, j]) < C.int_of(C.fr_sub(got[i, j], msgs[i, j])) for i in range(n) for j in range(m))
        assert borrows > 0                                     # the keystream exceeded the cipher word somewhere
        back, ok, rej = H.cipher_decrypt(c, to_dev(torch, keys), to_dev(torch, nonces), m)
        assert rej == 0 and (to_host(back).reshape(n, m, 4) == msgs).all()


@pytest.mark.parametrize("n,m", [(300, 2), (1024, 5), (4099, 2), (4099, 9)])
def test_tampering_rejects_exactly_the_tampered(torch_cuda, H, hades_lib, oracle, n, m):
    torch = torch_cuda
    msgs, keys, nonces = _inputs(oracle, n, m, 31 + m)
    dk, dn = to_dev(torch, keys), to_dev(torch, nonces)
    c = to_host(H.cipher_encrypt(to_dev(torch, msgs), dk, dn, m)).reshape(n, m + 1, 4).copy()
    rng = random.Random(n + m)
    bad = sorted(rng.sample(range(n), max(1, n // 10)))
    for i in bad:
        k = rng.randrange(m + 1)                               # any word, the tag included
        c[i, k] = C.fr_add(c[i, k][None], C.limbs(rng.randrange(1, P))[None])[0]
    rej = torch.full((1,), 5, dtype=torch.int32, device="cuda")      # the entry point ADDS to it
    out = torch.empty((n, m, 4), dtype=torch.int64, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    dc = to_dev(torch, c)
    assert hades_lib.hades252_cipher_decrypt_dev(dc.data_ptr(), dk.data_ptr(), dn.data_ptr(), n, m, H._tag_arr(H.CIPHER_DOMAIN),
                                                 out.data_ptr(), ok.data_ptr(), rej.data_ptr(), None) == 0
    torch.cuda.synchronize()
    want_ok = np.ones(n, dtype=np.uint8)
    want_ok[bad] = 0
    assert (ok.cpu().numpy() == want_ok).all()
    assert int(rej.item()) == 5 + len(bad)
    got = to_host(out).reshape(n, m, 4)
    assert (got[bad] == 0).all()
    keep = want_ok == 1
    assert (got[keep] == msgs[keep]).all()
    exp_m, exp_ok = C.decrypt_batch(c, keys, nonces, m, oracle.perm_batch)
    assert (exp_ok == want_ok).all() and (got == exp_m).all()


@pytest.mark.parametrize("n", [2, 2000])
def test_non_canonical_cipher_word_is_rejected(torch_cuda, H, oracle, n):
    """c + p encodes the same field element as c but is not canonical: rejected (so is 2^256 - 1), the rest accepted."""
    torch = torch_cuda
    m = 5
    msgs, keys, nonces = _inputs(oracle, n, m, 77)
    dk, dn = to_dev(torch, keys), to_dev(torch, nonces)
    c = to_host(H.cipher_encrypt(to_dev(torch, msgs), dk, dn, m)).reshape(n, m + 1, 4).copy()
    c[0, 1] = C.limbs(C.int_of(c[0, 1]) + P)
    c[n - 1, m] = C.limbs((1 << 256) - 1)
    back, ok, rej = H.cipher_decrypt(to_dev(torch, c), dk, dn, m)
    okh = ok.cpu().numpy()
    assert rej == 2 and okh[0] == 0 and okh[n - 1] == 0 and okh[1:n - 1].all()
    got = to_host(back).reshape(n, m, 4)
    assert (got[0] == 0).all() and (got[n - 1] == 0).all() and (got[1:n - 1] == msgs[1:n - 1]).all()


@pytest.mark.parametrize("n", [3, 1000, 5000])
def test_guard_words_stay_untouched(torch_cuda, H, hades_lib, oracle, n):
    torch = torch_cuda
    m, g = 3, 64                                               # g guard scalars (bytes for ok) after each output
    msgs, keys, nonces = _inputs(oracle, n, m, 5)
    dm, dk, dn = to_dev(torch, msgs), to_dev(torch, keys), to_dev(torch, nonces)
    dom = H._tag_arr(H.CIPHER_DOMAIN)
    cbuf = torch.full((n * (m + 1) + g, 4), 0x5A5A, dtype=torch.int64, device="cuda")
    assert hades_lib.hades252_cipher_encrypt_dev(dm.data_ptr(), dk.data_ptr(), dn.data_ptr(), n, m, dom, cbuf.data_ptr(), None) == 0
    mbuf = torch.full((n * m + g, 4), 0x3C3C, dtype=torch.int64, device="cuda")
    okbuf = torch.full((n + g,), 0x77, dtype=torch.uint8, device="cuda")
    assert hades_lib.hades252_cipher_decrypt_dev(cbuf.data_ptr(), dk.data_ptr(), dn.data_ptr(), n, m, dom, mbuf.data_ptr(),
                                                 okbuf.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert bool((cbuf[n * (m + 1):] == 0x5A5A).all()) and bool((mbuf[n * m:] == 0x3C3C).all())
    assert bool((okbuf[n:] == 0x77).all()) and bool((okbuf[:n] == 1).all())
    assert torch.equal(mbuf[:n * m].reshape(-1), dm.view(-1))


def test_non_default_stream(torch_cuda, H, oracle):
    torch = torch_cuda
    for n in (10, 3000):
        msgs, keys, nonces = _inputs(oracle, n, 2, 9)
        dm, dk, dn = to_dev(torch, msgs), to_dev(torch, keys), to_dev(torch, nonces)
        ref = H.cipher_encrypt(dm, dk, dn, 2)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            c = H.cipher_encrypt(dm, dk, dn, 2)
            back, ok, rej = H.cipher_decrypt(c, dk, dn, 2)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(c, ref) and torch.equal(back.view(-1), dm.view(-1)) and rej == 0


def test_known_answers_on_the_device(torch_cuda, H):
    torch = torch_cuda
    with open(os.path.join(ROOT, "tests", "golden", "cipher_kat.json")) as f:
        kat = json.load(f)
    dom = C.S.to_mont(int(kat["domain"], 16))
    for case in kat["cases"]:
        m = case["M"]
        mont = lambda vs: np.array([C.mont_limbs(int(v, 16)) for v in vs], dtype=np.uint64)   # noqa: E731
        c = H.cipher_encrypt(to_dev(torch, mont(case["msg"])), to_dev(torch, mont(case["key"])),
                             to_dev(torch, mont([case["nonce"]])), m, dom)
        assert (to_host(c).reshape(m + 1, 4) == mont(case["cipher"])).all(), case["seed"]


def test_host_entry_points_equal_the_device_ones(torch_cuda, H, oracle):
    """n = 2^20 + 5 at M = 2: several chunks of the host path, from ordinary and from page-locked memory."""
    torch = torch_cuda
    n, m = (1 << 20) + 5, 2
    dm = H.gen_b(n * m, "cuda", first_elem=0)
    dk = H.gen_b(2 * n, "cuda", first_elem=1 << 30)
    dn = H.gen_b(n, "cuda", first_elem=1 << 31)
    dc = H.cipher_encrypt(dm, dk, dn, m)
    want_c = to_host(dc)
    hm, hk, hn = to_host(dm).copy(), to_host(dk).copy(), to_host(dn).copy()
    c = H.cipher_encrypt_host(hm, hk, hn, m)
    assert (c.reshape(-1) == want_c).all()
    hc = want_c.copy()
    bad = [5, n // 2, n - 1]                                   # rejections in the first, a middle and the last chunk
    for i in bad:
        hc[i * (m + 1) * 4] ^= 1                               # its first cipher word
    back, ok, rej = H.cipher_decrypt_host(hc, hk, hn, m)
    assert rej == len(bad) and (ok[bad] == 0).all() and int(ok.sum()) == n - len(bad)
    want_m = hm.reshape(n, m, 4).copy()
    want_m[bad] = 0
    assert (back == want_m).all()
    pinned = [torch.empty(a.size, dtype=torch.int64, pin_memory=True) for a in (hm, hk, hn, hc)]
    for t, a in zip(pinned, (hm, hk, hn, hc)):
        t.numpy().view(np.uint64)[:] = a
    pm, pk, pn, pc = (t.numpy().view(np.uint64) for t in pinned)
    assert (H.cipher_encrypt_host(pm, pk, pn, m).reshape(-1) == want_c).all()
    back2, ok2, rej2 = H.cipher_decrypt_host(pc, pk, pn, m)
    assert rej2 == len(bad) and (back2 == want_m).all() and (ok2 == ok).all()


def test_2_24_messages_round_trip_and_samples(torch_cuda, H, oracle):
    torch = torch_cuda
    n, m = 1 << 24, 2
    dm = H.gen_b(n * m, "cuda", first_elem=0)
    dk = H.gen_b(2 * n, "cuda", first_elem=1 << 34)
    dn = H.gen_b(n, "cuda", first_elem=1 << 35)
    dc = H.cipher_encrypt(dm, dk, dn, m)
    back, ok, rej = H.cipher_decrypt(dc, dk, dn, m)
    assert rej == 0 and bool((ok == 1).all()) and torch.equal(back.view(-1), dm.view(-1))
    del back, ok
    idx = torch.tensor(sorted(random.Random(24).sample(range(n), 4096)), device="cuda")
    sm = to_host(dm.view(n, m, 4)[idx]).reshape(-1, m, 4)
    sk = to_host(dk.view(n, 2, 4)[idx]).reshape(-1, 2, 4)
    sn = to_host(dn.view(n, 4)[idx]).reshape(-1, 4)
    got = to_host(dc[idx]).reshape(-1, m + 1, 4)
    assert (got == C.encrypt_batch(sm, sk, sn, m, oracle.perm_batch)).all()

