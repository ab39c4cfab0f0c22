"""GPU tier, row f9: the gadget witnesses of the batched duplex sponge (hades252_safe_witness_dev and the streaming
hades252_safe_{absorb,squeeze}_witness_dev).  The defining property wires == perm_witness(inputs), byte for byte, on every
case; the inputs against the model (tests/safe_witness_model.py, over the C oracle's perm_batch); the outputs against
hades252_safe_hash_dev; sampled records against the spec's GadgetStrategy wire for wire; guard words behind every output
buffer, inputs untouched; every cut of a few patterns into streaming witness calls against the one-shot bytes and against
the plain streaming calls' states and cursor; the instances (zero-fill sponge witness, Merkle level-0 records), the SAFE
cipher composed over the streaming witness calls, a non-default stream and 2^18 sponges.  Convention of f8 (UNPINNED,
include/hades252.h).  No call here is refused: the argument rules are exercised on the CPU tier."""
import ctypes
import itertools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cipher_model as C  # noqa: E402
import safe_model as M  # noqa: E402
import safe_witness_model as W  # noqa: E402
from safe_model import A, Q  # noqa: E402
from safe_witness_model import P, S  # noqa: E402
from gpu_common import CAP, TAG4, WIRES, Guarded, assert_wires_are_perm_witness, gadget_check, to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

LAST_ROW = WIRES - 9                             # r2[0] of the last round; r2[j] = LAST_ROW + 2 j
NS = (1, 63, 64, 65, 257)
TAG = S.to_mont(0x5AFE)


def _name(pattern):
    return "".join("%s%d" % ("A" if kind == "absorb" else "S", n) for kind, n in pattern)


def _edge_inputs(rng, n, k):
    """n x k stored words (canonical 256-bit limbs): 0 and p - 1 mixed with random ones, the first sponge all 0 and the
    last all p - 1"""
    a = np.array([[C.limbs(rng.choice([0, P - 1]) if rng.random() < 0.4 else rng.randrange(P)) for _ in range(k)]
                  for _ in range(n)], dtype=np.uint64).reshape(n, k, 4)
    a[0] = C.limbs(0)
    a[n - 1] = C.limbs(P - 1)
    return a


def _one_shot(torch, hades_lib, H, d_in, n, pattern, tag_mont, with_out=True):
    """The raw call on guarded buffers -> (inputs [S * n, 5, 4], wires [972, S * n, 4], out [n, n_out, 4] or None)."""
    _, n_out, steps = H.safe_pattern(pattern)
    arr, k = H._safe_calls(pattern, "test")
    inputs, wires = Guarded(torch, (steps * n, 5, 4)), Guarded(torch, (WIRES, steps * n, 4))
    out = Guarded(torch, (n, n_out, 4)) if with_out else None
    rc = hades_lib.hades252_safe_witness_dev(d_in.data_ptr(), n, arr, k, H._tag_arr(tag_mont), inputs.ptr, wires.ptr,
                                             out.ptr if with_out else None, None)
    assert rc == 0
    what = (n, _name(pattern))
    return inputs.check(what), wires.check(what), out.check(what) if with_out else None


@pytest.mark.parametrize("pattern", W.GPU_PATTERNS, ids=_name)
def test_one_shot_against_model_perm_witness_and_safe_hash(torch_cuda, H, hades_lib, oracle, pattern):
    torch = torch_cuda
    n_in, n_out, steps = H.safe_pattern(pattern)
    assert steps == M.perms_closed_form(pattern) == W.GPU_PATTERN_PERMS[W.GPU_PATTERNS.index(pattern)]
    for n in NS:
        rng = random.Random(1000 * len(pattern) + 7 * n_in + n)
        tag = rng.choice([0, P - 1, TAG, rng.randrange(P)])
        h_in = _edge_inputs(rng, n, n_in)
        d_in = to_dev(torch, h_in)
        got_in, got_wires, got_out = _one_shot(torch, hades_lib, H, d_in, n, pattern, tag)
        assert (to_host(d_in) == h_in.reshape(-1)).all(), n           # d_in is not modified
        exp_in, exp_out, _ = W.batch_inputs(pattern, h_in, tag, oracle.perm_batch)
        assert exp_in.shape == (steps, n, 5, 4)
        inputs_h = to_host(got_in).reshape(steps, n, 5, 4)
        assert (inputs_h == exp_in).all(), n
        assert_wires_are_perm_witness(torch, H, got_in, got_wires)
        ref_out = H.safe_hash(d_in, pattern, tag)
        assert torch.equal(got_out, ref_out), n
        assert (to_host(ref_out).reshape(n, n_out, 4) == exp_out).all(), n
        # the output of the last permutation is r2 of the last round of the last record
        last = to_host(got_wires.view(WIRES, steps, n, 4)[LAST_ROW::2, steps - 1]).reshape(5, n, 4)
        final = oracle.perm_batch(exp_in[steps - 1].reshape(-1).copy()).reshape(n, 5, 4)
        assert (last.transpose(1, 0, 2) == final).all(), n
        # d_out = NULL leaves the rest identical
        bare_in, bare_wires, _ = _one_shot(torch, hades_lib, H, d_in, n, pattern, tag, with_out=False)
        assert torch.equal(bare_in, got_in) and torch.equal(bare_wires, got_wires), n
        wires_h = to_host(got_wires).reshape(WIRES, steps, n, 4)
        pairs = {(0, 0), (steps - 1, n - 1), (rng.randrange(steps), rng.randrange(n))}
        gadget_check(wires_h, inputs_h, sorted(pairs))
        if n == 65:                                       # the Python layer: same bytes in the documented shapes
            pw, pi, po = H.safe_witness(d_in.view(n, n_in, 4), pattern, tag)
            assert tuple(pw.shape) == (WIRES, steps, n, 4) and tuple(pi.shape) == (steps, n, 5, 4)
            assert tuple(po.shape) == (n, n_out, 4)
            assert torch.equal(pw.view(-1), got_wires.reshape(-1)) and torch.equal(pi.view(-1), got_in.reshape(-1))
            assert torch.equal(po, ref_out)


class _Stream:
    """The raw streaming witness calls on guarded record buffers, beside a plain sponge fed the same calls."""

    def __init__(self, torch, hades_lib, n, total, tag_mont):
        self.torch, self.lib, self.n, self.total = torch, hades_lib, n, total
        init = torch.zeros((n, 5, 4), dtype=torch.int64, device="cuda")
        init[:, 0] = to_dev(torch, C.limbs(tag_mont))
        self.st, self.plain = Guarded(torch, (n, 5, 4), init=init), Guarded(torch, (n, 5, 4), init=init)
        self.inputs = Guarded(torch, (max(total, 1) * n, 5, 4))
        self.wires = Guarded(torch, (WIRES, max(total, 1) * n, 4))
        self.cur, self.pcur, self.step = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_size_t(0)

    def _after(self, q, what):
        """q = the permutations the model says the call runs: *step moved by q; the states and the cursor are the plain
        call's; a call with q = 0 changed no byte of the record buffers."""
        torch = self.torch
        assert self.step.value == self._step_before + q, what
        assert self.cur.value == self.pcur.value, what
        assert torch.equal(self.st.check(what), self.plain.check(what)), what
        self.inputs.check(what, interior=False)
        self.wires.check(what, interior=False)
        if q == 0:
            assert torch.equal(self.inputs.buf, self._inputs_before) and torch.equal(self.wires.buf, self._wires_before), what

    def _before(self, q):
        self._step_before = self.step.value
        if q == 0:
            self._inputs_before, self._wires_before = self.inputs.buf.clone(), self.wires.buf.clone()

    def absorb(self, words, q):
        k = words.shape[1]
        self._before(q)
        assert self.lib.hades252_safe_absorb_witness_dev(self.st.ptr, self.n, words.data_ptr(), k, ctypes.byref(self.cur),
                                                         self.inputs.ptr, self.wires.ptr, self.total,
                                                         ctypes.byref(self.step), None) == 0
        assert self.lib.hades252_safe_absorb_dev(self.plain.ptr, self.n, words.data_ptr(), k, ctypes.byref(self.pcur),
                                                 None) == 0
        self._after(q, ("absorb", k))

    def squeeze(self, k, q):
        self._before(q)
        out, pout = Guarded(self.torch, (self.n, k, 4)), Guarded(self.torch, (self.n, k, 4))
        assert self.lib.hades252_safe_squeeze_witness_dev(self.st.ptr, self.n, k, out.ptr, ctypes.byref(self.cur),
                                                          self.inputs.ptr, self.wires.ptr, self.total,
                                                          ctypes.byref(self.step), None) == 0
        assert self.lib.hades252_safe_squeeze_dev(self.plain.ptr, self.n, k, pout.ptr, ctypes.byref(self.pcur), None) == 0
        self._after(q, ("squeeze", k))
        got = out.check(("squeeze", k))
        assert self.torch.equal(got, pout.check())
        return got


@pytest.mark.parametrize("pattern", W.GPU_CUT_PATTERNS, ids=_name)
@pytest.mark.parametrize("n", [70, 300])
def test_every_cut_into_streaming_witness_calls_equals_the_one_shot_bytes(torch_cuda, H, hades_lib, oracle, pattern, n):
    torch = torch_cuda
    n_in, n_out, steps = H.safe_pattern(pattern)
    rng = random.Random(91 + n)
    h_in = _edge_inputs(rng, n, n_in)
    d_in = to_dev(torch, h_in).view(n, n_in, 4)
    want_in, want_wires, want_out = _one_shot(torch, hades_lib, H, d_in, n, pattern, TAG)
    assert (to_host(want_in).reshape(steps, n, 5, 4) == W.batch_inputs(pattern, h_in, TAG, oracle.perm_batch)[0]).all()
    assert_wires_are_perm_witness(torch, H, want_in, want_wires)
    agg = M.aggregate(pattern)
    ways = 0
    for pieces in itertools.product(*[list(W.cuts(k)) for _, k in agg]):
        calls = W.cut(pattern, pieces)
        sp, outs, at, cursor = _Stream(torch, hades_lib, n, steps, TAG), [], 0, 0
        for kind, k in calls:
            w_steps, cursor = W.walk([(kind, k)], cursor)
            q = len(w_steps) - 1
            if kind == "absorb":
                sp.absorb(d_in[:, at:at + k].contiguous(), q)
                at += k
            else:
                outs.append(sp.squeeze(k, q))
            assert sp.cur.value == cursor, calls
        assert sp.step.value == steps, calls
        assert torch.equal(sp.inputs.check(calls), want_in), calls
        assert torch.equal(sp.wires.check(calls), want_wires), calls
        assert torch.equal(torch.cat(outs, dim=1), want_out), calls
        assert torch.equal(d_in.reshape(-1), to_dev(torch, h_in).reshape(-1))
        ways += 1
    assert ways == int(np.prod([2 ** (k - 1) for _, k in agg]))


def test_python_streaming_sponge(torch_cuda, H, oracle):
    torch = torch_cuda
    pattern, n = [A(3), Q(2), A(2), Q(1)], 130
    d_in = to_dev(torch, oracle.gen_b(77, n * 5)).view(n, 5, 4)
    wires, inputs, out = H.safe_witness(d_in, pattern, TAG)
    sp = H.SafeWitnessSponge(n, pattern, TAG)
    sp.absorb(d_in[:, :1].contiguous())
    sp.absorb(d_in[:, 1:3].contiguous())
    a = sp.squeeze(2)
    with pytest.raises(ValueError):                       # the records are complete after finish() only
        sp.wires
    with pytest.raises(ValueError):
        sp.finish()
    sp.absorb(d_in[:, 3:].contiguous())
    b = sp.squeeze(1)
    sp.finish()
    assert tuple(sp.wires.shape) == (WIRES, 2, n, 4) and tuple(sp.inputs.shape) == (2, n, 5, 4)
    assert torch.equal(sp.wires, wires) and torch.equal(sp.inputs, inputs) and torch.equal(torch.cat([a, b], dim=1), out)


@pytest.mark.parametrize("length", [1, 3, 4, 5, 8, 9])
def test_absorb_then_one_word_equals_the_zero_fill_sponge_witness(torch_cuda, H, hades_lib, length):
    torch = torch_cuda
    for n in (65, 1000):
        msgs = H.gen_b(n * length, "cuda", first_elem=length << 24)
        got_in, got_wires, got_out = _one_shot(torch, hades_lib, H, msgs, n, [A(length), Q(1)], CAP)
        wires, inputs, digests = H.sponge_witness(msgs, length, CAP, pad_mode=0, digests=True)
        assert torch.equal(got_in.reshape(-1), inputs.view(-1)) and torch.equal(got_wires.reshape(-1), wires.view(-1))
        assert torch.equal(got_out.view(n, 4), digests)


def test_four_words_with_tag_15_equals_the_merkle_level_0_records(torch_cuda, H, hades_lib):
    torch = torch_cuda
    for n in (64, 1000):                                  # n groups of four leaves: the arity-4 tree of 4 n leaves
        leaves = H.gen_b(4 * n, "cuda", first_elem=7 << 24)
        got_in, got_wires, got_out = _one_shot(torch, hades_lib, H, leaves, n, [A(4), Q(1)], TAG4)
        tree = H.merkle_build(leaves, 4, TAG4)
        idx = torch.arange(0, 4 * n, 4, dtype=torch.int64, device="cuda")
        wires, inputs, n_bad = H.merkle_open_witness(leaves, tree, 4, idx, TAG4)
        assert n_bad == 0
        assert torch.equal(got_in, inputs[0]) and torch.equal(got_wires, wires[:, 0, :])
        assert torch.equal(got_out.view(n, 4), H.merkle4_level(leaves, TAG4))


def test_cipher_composed_over_the_streaming_witness_calls(torch_cuda, H, oracle):
    """[A(2) key, A(1) nonce, S(M), A(M) message, S(1)] with cipher = message + squeezed words: encrypt and the decryption
    of its result record the witness of the one-shot pattern on (key, nonce, message)."""
    torch = torch_cuda
    minus_one = to_dev(torch, C.mont_limbs(P - 1))

    def run(key_t, nonce_t, words_t, m, decrypt):
        n = nonce_t.numel() // 4
        sp = H.SafeWitnessSponge(n, M.cipher_pattern(m), TAG)
        sp.absorb(key_t)
        sp.absorb(nonce_t)
        ks = sp.squeeze(m)
        if decrypt:
            neg = H.fr_op(H.FR_MUL, ks.view(-1, 4), minus_one.view(1, 4).expand(n * m, 4).contiguous())
            msg = H.fr_op(H.FR_ADD, words_t.view(n, m + 1, 4)[:, :m].contiguous().view(-1, 4), neg).view(n, m, 4)
            sp.absorb(msg)
            tag_word = sp.squeeze(1)
            sp.finish()
            return sp, msg, (tag_word.view(n, 4) == words_t.view(n, m + 1, 4)[:, m]).all(dim=1)
        c = H.fr_op(H.FR_ADD, words_t.view(-1, 4), ks.view(-1, 4)).view(n, m, 4)
        sp.absorb(words_t)
        out = torch.cat([c, sp.squeeze(1)], dim=1)
        sp.finish()
        return sp, out

    for n, m in ((3, 2), (900, 5), (257, 1)):
        keys, nonces = oracle.gen_b(n, 2 * n).reshape(n, 2, 4), oracle.gen_b(n + (1 << 20), n).reshape(n, 4)
        msgs = oracle.gen_b(n + (1 << 21), n * m).reshape(n, m, 4)
        dk, dn, dm = to_dev(torch, keys), to_dev(torch, nonces), to_dev(torch, msgs)
        whole = torch.cat([dk.view(n, 2, 4), dn.view(n, 1, 4), dm.view(n, m, 4)], dim=1).contiguous()
        wires, inputs, squeezed = H.safe_witness(whole, M.cipher_pattern(m), TAG)
        enc, c = run(dk, dn, dm, m, False)
        assert torch.equal(enc.wires, wires) and torch.equal(enc.inputs, inputs), (n, m)
        assert torch.equal(c[:, m:], squeezed[:, m:])
        exp_sq = M.run_batch(M.cipher_pattern(m), np.concatenate([keys, nonces[:, None], msgs], axis=1), TAG,
                             oracle.perm_batch)
        exp = np.concatenate([C.fr_add(msgs, exp_sq[:, :m]), exp_sq[:, m:]], axis=1)
        assert (to_host(c).reshape(n, m + 1, 4) == exp).all(), (n, m)
        dec, back, ok = run(dk, dn, c, m, True)
        assert bool(ok.all()) and torch.equal(back.reshape(-1), dm.view(-1)), (n, m)
        assert torch.equal(dec.wires, wires) and torch.equal(dec.inputs, inputs), (n, m)


def test_non_default_stream(torch_cuda, H, oracle):
    torch = torch_cuda
    pattern = [A(3), Q(2), A(2), Q(1)]
    for n in (10, 3000):
        d_in = to_dev(torch, oracle.gen_b(9 + n, n * 5)).view(n, 5, 4)
        wires, inputs, out = H.safe_witness(d_in, pattern, TAG)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            w2, i2, o2 = H.safe_witness(d_in, pattern, TAG)
            sp = H.SafeWitnessSponge(n, pattern, TAG)
            sp.absorb(d_in[:, :3].contiguous())
            a = sp.squeeze(2)
            sp.absorb(d_in[:, 3:].contiguous())
            b = sp.squeeze(1)
            sp.finish()
        torch.cuda.current_stream().wait_stream(s)
        s.synchronize()
        assert torch.equal(w2, wires) and torch.equal(i2, inputs) and torch.equal(o2, out)
        assert torch.equal(sp.wires, wires) and torch.equal(sp.inputs, inputs) and torch.equal(torch.cat([a, b], dim=1), out)
        assert torch.equal(out, H.safe_hash(d_in, pattern, TAG))


def test_safe_witness_at_scale(torch_cuda, H, oracle):
    """2^18 sponges of [A(3), S(2), A(2), S(1)]: 2^19 records (16.3 GB of wires, as much again for the reference), compared
    on the device: wires == perm_witness(inputs) on all records, out == safe_hash; sampled sponges against the model."""
    torch = torch_cuda
    pattern, n = [A(3), Q(2), A(2), Q(1)], 1 << 18
    d_in = H.gen_b(n * 5, "cuda", first_elem=1 << 35).view(n, 5, 4)
    wires, inputs, out = H.safe_witness(d_in, pattern, TAG)
    assert torch.equal(out, H.safe_hash(d_in, pattern, TAG))
    ref = H.perm_witness(inputs.view(2 * n, 20))
    assert torch.equal(wires.view(WIRES, 2 * n, 4), ref)
    del ref
    idx = torch.arange(0, n, 1021, device="cuda")
    sample = to_host(d_in[idx]).reshape(-1, 5, 4)
    exp_in, exp_out, _ = W.batch_inputs(pattern, sample, TAG, oracle.perm_batch)
    assert (to_host(inputs[:, idx]).reshape(exp_in.shape) == exp_in).all()
    assert (to_host(out[idx]).reshape(exp_out.shape) == exp_out).all()
