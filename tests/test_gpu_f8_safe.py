"""GPU tier, row f8 (beyond SURVEY section 8): the batched duplex sponge (hades252_safe_*) against its model
(tests/safe_model.py, over the C oracle's perm_batch) and against the kernels already trusted -- both kernel forms, patterns
that reach every (emit, add) step, split calls, every cut of a pattern into streaming calls, the cipher composed over the
streaming calls, edge values, guard words, a non-default stream, the host entry point, 2^22 sponges.  Bit-exact everywhere.
Convention: dusk-safe's sponge as recalled, UNPINNED (include/hades252.h)."""
import itertools
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cipher_model as C  # noqa: E402
import safe_model as M  # noqa: E402
from safe_model import A, Q  # noqa: E402
from gpu_common import CAP, TAG4, Guarded, to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

P = M.P
NS = [1, 3, 64, 1024, 1025, 4099, 65537]        # one per wave (<= 1024, helped <= 768) and one per lane, ragged waves
PATTERNS = [[A(L), Q(1)] for L in range(1, 10)] + [
    [A(1), Q(9)], [A(5), Q(6)], [A(3), Q(2), A(2), Q(1)], [A(4), Q(4), A(4), Q(4)], [A(2), A(1), Q(1), Q(2)],
    [A(1), A(1), Q(1), A(2), A(3), Q(2), Q(3)]]
TAG = M.S.to_mont(0x5AFE)


def _name(pattern):
    return "".join("%s%d" % ("A" if kind == "absorb" else "S", n) for kind, n in pattern)


def _inputs(oracle, n, pattern, seed):
    return oracle.gen_b(seed * 1000003, n * M.words_in(pattern)).reshape(n, M.words_in(pattern), 4)


@pytest.mark.parametrize("pattern", PATTERNS, ids=_name)
def test_one_shot_against_the_model(torch_cuda, H, oracle, pattern):
    torch = torch_cuda
    for n in NS:
        inputs = _inputs(oracle, n, pattern, 13 * len(pattern) + n)
        got = H.safe_hash(to_dev(torch, inputs), pattern, TAG)
        exp = M.run_batch(pattern, inputs, TAG, oracle.perm_batch)
        assert got.shape == (n, M.words_out(pattern), 4)
        assert (to_host(got).reshape(exp.shape) == exp).all(), (n, pattern)


@pytest.mark.parametrize("length", [1, 2, 3, 4, 5, 8, 9])
def test_absorb_then_one_word_equals_the_zero_fill_sponge_kernel(torch_cuda, H, length):
    torch = torch_cuda
    n = 65537
    msgs = H.gen_b(n * length, "cuda", first_elem=length << 24)
    got = H.safe_hash(msgs, [A(length), Q(1)], CAP)
    assert torch.equal(got.view(n, 4), H.sponge_hash(msgs, length, CAP, pad_mode=0))


def test_four_words_with_tag_15_equals_the_merkle_level_kernel(torch_cuda, H):
    torch = torch_cuda
    n = 65537
    children = H.gen_b(n * 4, "cuda", first_elem=7 << 24)
    got = H.safe_hash(children, [A(4), Q(1)], TAG4)
    assert torch.equal(got.view(n, 4), H.merkle4_level(children, TAG4))


def _cuts(length):
    """every way of cutting `length` words into consecutive calls"""
    for k in range(length):
        for at in itertools.combinations(range(1, length), k):
            edges = (0,) + at + (length,)
            yield [b - a for a, b in zip(edges, edges[1:])]


@pytest.mark.parametrize("pattern", [[A(3), Q(2), A(2), Q(1)], [A(5), Q(6)], [A(2), A(1), Q(1), Q(2)]], ids=_name)
@pytest.mark.parametrize("n", [70, 1100])
def test_every_cut_into_streaming_calls_equals_the_one_shot_bytes(torch_cuda, H, oracle, pattern, n):
    torch = torch_cuda
    inputs = _inputs(oracle, n, pattern, 91 + n)
    d_in = to_dev(torch, inputs).view(n, -1, 4)
    want = H.safe_hash(d_in, pattern, TAG)
    assert (to_host(want).reshape(n, -1, 4) == M.run_batch(pattern, inputs, TAG, oracle.perm_batch)).all()
    agg = M.aggregate(pattern)
    ways = 0
    for cut in itertools.product(*[list(_cuts(k)) for _, k in agg]):
        sp, outs, at = H.SafeSponge(n, pattern, TAG), [], 0
        for (kind, _), pieces in zip(agg, cut):
            for k in pieces:
                if kind == "absorb":
                    sp.absorb(d_in[:, at:at + k].contiguous())
                    at += k
                else:
                    outs.append(sp.squeeze(k))
        sp.finish()
        assert torch.equal(torch.cat(outs, dim=1), want), cut
        ways += 1
    assert ways == int(np.prod([2 ** (k - 1) for _, k in agg]))


def test_streaming_states_and_guards(torch_cuda, H, hades_lib, oracle):
    """The raw streaming calls on guarded buffers: the state array and the output keep their guard rows, the states after
    the calls are the model's, the cursor moves as the positions do."""
    import ctypes
    torch = torch_cuda
    for n in (5, 1000, 3000):
        xs = oracle.gen_b(n + 17, n * 6).reshape(n, 6, 4)
        model = M.SpongeBatch(n, TAG, oracle.perm_batch)
        init = torch.zeros((n, 5, 4), dtype=torch.int64, device="cuda")
        init[:, 0] = to_dev(torch, C.limbs(TAG))
        st = Guarded(torch, (n, 5, 4), init=init)
        cur = ctypes.c_uint32(0)
        d_x = to_dev(torch, xs).view(n, 6, 4)
        assert hades_lib.hades252_safe_absorb_dev(st.ptr, n, d_x.data_ptr(), 6, ctypes.byref(cur), None) == 0
        model.absorb(xs)
        assert cur.value == 2 | (4 << 4)
        assert (to_host(st.check("after absorb")).reshape(n, 5, 4) == model.state).all()
        out = Guarded(torch, (n, 5, 4))
        assert hades_lib.hades252_safe_squeeze_dev(st.ptr, n, 5, out.ptr, ctypes.byref(cur), None) == 0
        exp = model.squeeze(5)
        assert cur.value == 0 | (1 << 4)
        assert (to_host(out.check("squeezed")).reshape(n, 5, 4) == exp).all()
        assert (to_host(st.check("after squeeze")).reshape(n, 5, 4) == model.state).all()


def test_cipher_composed_over_the_streaming_calls(torch_cuda, H, oracle):
    """[A(2) key, A(1) nonce, S(M), A(M) message, S(1)] with cipher = message + squeezed words (H.fr_op), decrypted back,
    and equal to the golden file's ciphers."""
    torch = torch_cuda
    minus_one = to_dev(torch, C.mont_limbs(P - 1))

    def run(key_t, nonce_t, words_t, m, tag, decrypt):
        n = nonce_t.numel() // 4
        sp = H.SafeSponge(n, M.cipher_pattern(m), tag)
        sp.absorb(key_t)
        sp.absorb(nonce_t)
        ks = sp.squeeze(m)
        if decrypt:
            neg = H.fr_op(H.FR_MUL, ks.view(-1, 4), minus_one.view(1, 4).expand(n * m, 4).contiguous())
            msg = H.fr_op(H.FR_ADD, words_t.view(n, m + 1, 4)[:, :m].contiguous().view(-1, 4), neg).view(n, m, 4)
            sp.absorb(msg)
            tag_word = sp.squeeze(1)
            sp.finish()
            return msg, (tag_word.view(n, 4) == words_t.view(n, m + 1, 4)[:, m]).all(dim=1)
        c = H.fr_op(H.FR_ADD, words_t.view(-1, 4), ks.view(-1, 4)).view(n, m, 4)
        sp.absorb(words_t)
        out = torch.cat([c, sp.squeeze(1)], dim=1)
        sp.finish()
        return out

    with open(os.path.join(ROOT, "tests", "golden", "safe_kat.json")) as f:
        kat = json.load(f)
    seen = 0
    for case in kat["cases"]:
        if "cipher" not in case:
            continue
        mont = lambda vs: np.array([C.mont_limbs(int(v, 16)) for v in vs], dtype=np.uint64)   # noqa: E731
        inp, m, tag = mont(case["inputs"]), len(case["cipher"]) - 1, M.S.to_mont(int(case["tag"], 16))
        c = run(to_dev(torch, inp[:2]), to_dev(torch, inp[2:3]), to_dev(torch, inp[3:]), m, tag, False)
        assert (to_host(c).reshape(m + 1, 4) == mont(case["cipher"])).all(), case["seed"]
        seen += 1
    assert seen == 2
    for n, m in ((3, 2), (900, 5), (5000, 2)):
        keys, nonces = oracle.gen_b(n, 2 * n).reshape(n, 2, 4), oracle.gen_b(n + (1 << 20), n).reshape(n, 4)
        msgs = oracle.gen_b(n + (1 << 21), n * m).reshape(n, m, 4)
        dk, dn, dm = to_dev(torch, keys), to_dev(torch, nonces), to_dev(torch, msgs)
        c = run(dk, dn, dm, m, TAG, False)
        squeezed = M.run_batch(M.cipher_pattern(m), np.concatenate([keys, nonces[:, None], msgs], axis=1), TAG, oracle.perm_batch)
        exp = np.concatenate([C.fr_add(msgs, squeezed[:, :m]), squeezed[:, m:]], axis=1)
        assert (to_host(c).reshape(n, m + 1, 4) == exp).all(), (n, m)
        back, ok = run(dk, dn, c, m, TAG, True)
        assert bool(ok.all()) and torch.equal(back.reshape(-1), dm.view(-1)), (n, m)


def test_edge_values_as_inputs_and_as_tag(torch_cuda, H, oracle):
    torch = torch_cuda
    edge = [0, 1, P - 1, P - 2]
    for n, pattern in ((5, [A(4), Q(1)]), (700, [A(3), Q(2), A(2), Q(1)]), (3000, [A(5), Q(6)]), (1500, [A(1), Q(9)])):
        rng = random.Random(n)
        k = M.words_in(pattern)
        inputs = np.array([[C.limbs(rng.choice(edge) if rng.random() < 0.7 else rng.randrange(P)) for _ in range(k)]
                           for _ in range(n)], dtype=np.uint64)
        inputs[0] = C.limbs(0)
        inputs[n - 1] = C.limbs(P - 1)
        for tag in edge:
            got = H.safe_hash(to_dev(torch, inputs), pattern, tag)
            exp = M.run_batch(pattern, inputs, tag, oracle.perm_batch)
            assert (to_host(got).reshape(exp.shape) == exp).all(), (n, pattern, tag)


@pytest.mark.parametrize("n", [3, 1000, 5000])
def test_guard_words_after_the_output_stay_untouched(torch_cuda, H, hades_lib, oracle, n):
    torch = torch_cuda
    for pattern in ([A(3), Q(2), A(2), Q(1)], [A(1), Q(9)]):
        inputs = _inputs(oracle, n, pattern, 5)
        d_in = to_dev(torch, inputs)
        arr, k = H._safe_calls(pattern, "test")
        out = Guarded(torch, (n, M.words_out(pattern), 4))
        assert hades_lib.hades252_safe_hash_dev(d_in.data_ptr(), n, arr, k, H._tag_arr(TAG), out.ptr, None) == 0
        got = out.check((n, pattern))
        assert torch.equal(got, H.safe_hash(d_in, pattern, TAG))


def test_non_default_stream(torch_cuda, H, oracle):
    torch = torch_cuda
    pattern = [A(3), Q(2), A(2), Q(1)]
    for n in (10, 3000):
        d_in = to_dev(torch, _inputs(oracle, n, pattern, 9))
        ref = H.safe_hash(d_in, pattern, TAG)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = H.safe_hash(d_in, pattern, TAG)
            sp = H.SafeSponge(n, pattern, TAG)
            sp.absorb(d_in.view(n, 5, 4)[:, :3].contiguous())
            a = sp.squeeze(2)
            sp.absorb(d_in.view(n, 5, 4)[:, 3:].contiguous())
            b = sp.squeeze(1)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(got, ref) and torch.equal(torch.cat([a, b], dim=1), ref)


def test_host_entry_point_equals_the_device_one(torch_cuda, H):
    """n = 2^20 + 5 sponges of [A(3), S(2), A(2), S(1)]: several chunks of the host path, from ordinary and from page-locked
    memory."""
    torch = torch_cuda
    pattern = [A(3), Q(2), A(2), Q(1)]
    n = (1 << 20) + 5
    d_in = H.gen_b(n * 5, "cuda", first_elem=3 << 30)
    want = to_host(H.safe_hash(d_in, pattern, TAG))
    h_in = to_host(d_in).copy()
    assert (H.safe_hash_host(h_in, pattern, TAG).reshape(-1) == want).all()
    pinned = torch.empty(h_in.size, dtype=torch.int64, pin_memory=True)
    pinned.numpy().view(np.uint64)[:] = h_in
    assert (H.safe_hash_host(pinned.numpy().view(np.uint64), pattern, TAG).reshape(-1) == want).all()


def test_2_22_sponges_against_the_merkle_kernel_and_samples(torch_cuda, H, oracle):
    torch = torch_cuda
    n = 1 << 22
    children = H.gen_b(n * 4, "cuda", first_elem=1 << 36)
    got = H.safe_hash(children, [A(4), Q(1)], TAG4)
    assert torch.equal(got.view(n, 4), H.merkle4_level(children, TAG4))
    idx = torch.arange(0, n, 257, device="cuda")
    sample = to_host(children.view(n, 4, 4)[idx]).reshape(-1, 4, 4)
    exp = M.run_batch([A(4), Q(1)], sample, TAG4, oracle.perm_batch)
    assert (to_host(got[idx]).reshape(exp.shape) == exp).all()
