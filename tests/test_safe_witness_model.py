"""CPU tier: the model of the duplex sponge witnesses' input states (tests/safe_witness_model.py) against the sponge's own
model (tests/safe_model.py) and its neighbours -- the permutation count is the closed form, the outputs are the sponge's,
every cut of a pattern into streaming calls gives the one-shot states, the kernel's walk rebuilds the same states step by
step, [A(L), Q(1)] is the zero-fill sponge witness, decrypting an encryption of the SAFE cipher rebuilds the same states --
and committed known answers (tests/golden/safe_witness_kat.json).  Also the coverage condition of the GPU tier: its
patterns reach every step shape, its cuts the shapes only a streaming call has."""
import hashlib
import itertools
import json
import os
import random

import pytest

import safe_model as M
import safe_witness_model as W
import witness_chain_model as WC
from safe_model import A, Q
from safe_witness_model import P, S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "safe_witness_kat.json")


def _toy_perm(st):
    """a cheap stand-in for the permutation where only the bookkeeping is under test (the state words stay distinct)"""
    return [(x * x * 3 + 7 * i + 1) % P for i, x in enumerate(st)]


def _words(rng, k):
    return [rng.choice([0, P - 1, rng.randrange(P)]) for _ in range(k)]


def _all_cuts(pattern):
    agg = M.aggregate(pattern)
    for pieces in itertools.product(*[list(W.cuts(k)) for _, k in agg]):
        yield W.cut(pattern, pieces)


@pytest.mark.parametrize("pattern,perms", list(zip(W.GPU_PATTERNS, W.GPU_PATTERN_PERMS)))
def test_count_and_outputs_are_the_sponges(pattern, perms):
    rng = random.Random(len(pattern))
    inputs, tag = _words(rng, M.words_in(pattern)), rng.randrange(P)
    states, out = W.chain_inputs(pattern, inputs, tag, _toy_perm)
    assert len(states) == M.perms_closed_form(pattern) == perms
    assert (out, perms) == M.run(pattern, inputs, tag, _toy_perm)
    assert states[0][0] == tag
    # the walk rebuilds states, outputs and count step by step; a one-shot launch ends on cursor (pa, ps >= 1)
    w_states, w_out, (steps,), cursor = W.inputs_by_walk([pattern], inputs, tag, _toy_perm)
    assert (w_states, w_out) == (states, out) and len(steps) == perms + 1
    assert all(0 <= e0 <= 4 and e0 + j <= 4 and a0 + k <= 4 for e0, j, a0, k in steps)
    assert steps[-1][3] == 0 and steps[-1][1] >= 1                  # the final step: the pattern's last emits, no adds


def test_over_the_real_permutation():
    rng = random.Random(9)
    for pattern in ([A(3), Q(2), A(2), Q(1)], [A(5), Q(1)], [A(1), Q(5)]):
        inputs, tag = _words(rng, M.words_in(pattern)), rng.randrange(P)
        states, out = W.chain_inputs(pattern, inputs, tag)
        assert (out, len(states)) == M.run(pattern, inputs, tag)
        assert W.inputs_by_walk([pattern], inputs, tag)[:2] == (states, out)
        for s in range(1, len(states)):                             # word 0 is never absorbed into
            assert states[s][0] == S.perm(list(states[s - 1]))[0]


@pytest.mark.parametrize("pattern", W.GPU_CUT_PATTERNS + [[A(2), A(1), Q(2), A(2), Q(1)]])
def test_every_cut_gives_the_one_shot_states(pattern):
    rng = random.Random(sum(n for _, n in pattern))
    inputs, tag = _words(rng, M.words_in(pattern)), rng.randrange(P)
    want = W.chain_inputs(pattern, inputs, tag, _toy_perm)
    ways = 0
    for calls in _all_cuts(pattern):
        assert W.stream_inputs(calls, inputs, tag, _toy_perm) == want, calls
        # one launch per streaming call, each from the cursor the one before left
        states, out, steps, cursor = W.inputs_by_walk([[c] for c in calls], inputs, tag, _toy_perm)
        assert (states, out) == want, calls
        assert sum(len(st) - 1 for st in steps) == len(want[0])
        ways += 1
    assert ways == 2 ** sum(k - 1 for _, k in M.aggregate(pattern))


def test_gpu_patterns_reach_every_step_shape():
    seen = set()
    for pattern in W.GPU_PATTERNS:
        assert M.valid(pattern)
        steps, _ = W.walk(pattern)
        seen |= {(j, k) for _, j, _, k in steps}
    assert seen == {(j, k) for j in range(5) for k in range(5)} - {(0, 0)}          # 24 shapes; no one-shot (0, 0)
    assert len(seen) == 24


def test_gpu_cuts_reach_the_streaming_only_steps():
    """(0, 0): a squeeze that resumes on a full block permutes before it emits; and steps that start in mid-block."""
    shapes, e0s, a0s, no_perm = set(), set(), set(), 0
    for pattern in W.GPU_CUT_PATTERNS:
        for calls in _all_cuts(pattern):
            cursor = 0
            for c in calls:
                steps, cursor = W.walk([c], cursor)
                shapes |= {(j, k) for _, j, _, k in steps}
                e0s |= {e0 for e0, j, _, _ in steps if j}
                a0s |= {a0 for _, _, a0, k in steps if k}
                no_perm += len(steps) == 1
    assert (0, 0) in shapes
    assert e0s >= {0, 1, 2, 3} and a0s >= {0, 1, 2, 3}
    assert no_perm > 0                                                               # calls that record nothing


@pytest.mark.parametrize("length", [1, 3, 4, 5, 8, 9])
def test_absorb_then_one_word_is_the_zero_fill_sponge_witness(length):
    rng = random.Random(length)
    msg, cap = _words(rng, length), rng.randrange(P)
    states, out = W.chain_inputs([A(length), Q(1)], msg, cap)
    want, final = WC.sponge_inputs([msg], cap, pad_mode=0)
    assert states == [step[0] for step in want]
    assert out == [final[0][1]]


@pytest.mark.parametrize("m", [1, 2, 5])
def test_cipher_decrypt_of_encrypt_rebuilds_the_states(m):
    rng = random.Random(0xC0 + m)
    key, nonce, msg, tag = _words(rng, 2), rng.randrange(P), _words(rng, m), rng.randrange(P)
    recorded = []

    def recording(st):
        recorded.append(list(st))
        return S.perm(list(st))

    c = M.cipher_encrypt(msg, key, nonce, tag, recording)
    enc, recorded[:] = list(recorded), []
    assert M.cipher_decrypt(c, key, nonce, tag, recording) == (msg, True)
    assert recorded == enc
    # ... which are the states of the one-shot pattern on (key, nonce, message)
    assert W.chain_inputs(M.cipher_pattern(m), key + [nonce] + msg, tag)[0] == enc
    assert len(enc) == M.perms_closed_form(M.cipher_pattern(m))


# ---- known answers -----------------------------------------------------------------------------------------------------
def kat_cases():
    """The inputs of tests/golden/safe_witness_kat.json: seeded small patterns, canonical integers."""
    pats = [[A(1), Q(1)], [A(4), Q(1)], [A(5), Q(1)], [A(3), Q(2), A(2), Q(1)], [A(1), Q(5)], M.cipher_pattern(2)]
    out = []
    for seed, pat in enumerate(pats, 1):
        rng = random.Random(0x5AFE9 + seed)
        out.append({"seed": seed, "pattern": pat, "tag": rng.randrange(P),
                    "inputs": [rng.choice([0, P - 1, rng.randrange(P)]) for _ in range(M.words_in(pat))]})
    return out


def _sha(values):
    return hashlib.sha256(b"".join(int(v).to_bytes(32, "little") for v in values)).hexdigest()


def render_kat():
    cases = []
    for c in kat_cases():
        states, out = W.chain_inputs(c["pattern"], c["inputs"], c["tag"])
        wires = []
        for st in states:
            got = S.perm_gadget(list(st), wires)
            assert got == S.perm(list(st))
        assert len(wires) == WC.WIRES * len(states)
        cases.append({"seed": c["seed"], "pattern": [[k, n] for k, n in c["pattern"]], "tag": hex(c["tag"]),
                      "inputs": [hex(v) for v in c["inputs"]], "outputs": [hex(v) for v in out], "perms": len(states),
                      "states_sha256": _sha([v for st in states for v in st]), "wires_sha256": _sha(wires)})
    return {"about": "duplex sponge witness known answers (CONVENTION UNPINNED, include/hades252.h), generated by "
                     "tests/safe_witness_model.py over oracle/hades_spec.py; values are canonical integers, not Montgomery "
                     "form; states_sha256 = sha256 of the input states (step-major, 5 words each, 32 bytes little-endian per "
                     "word), wires_sha256 = the same of perm_gadget's 972 gate outputs of every state in step order",
            "cases": cases}


def test_known_answers_are_rederived_exactly():
    with open(KAT) as f:
        committed = json.load(f)
    assert committed == render_kat()
    assert len(committed["cases"]) == 6


if __name__ == "__main__":          # regenerate the golden file (only when the convention changes on purpose)
    with open(KAT, "w") as f:
        json.dump(render_kat(), f, indent=1)
        f.write("\n")
