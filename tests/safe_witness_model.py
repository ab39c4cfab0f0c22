"""Model of the input states of the duplex sponge's gadget witnesses (include/hades252.h, "gadget witnesses of the duplex
sponge"; CONVENTION UNPINNED as the sponge itself): tests/safe_model.py's Sponge with a permutation that records the state
it is given.  inputs[s] is the state that enters permutation s: the output of permutation s - 1 (or [tag, 0, 0, 0, 0]) with
the words absorbed since added at their positions; squeezed words are read, not changed.

Three forms:
  * `chain_inputs` / `stream_inputs` on canonical integers, one sponge, over oracle/hades_spec.py::perm (the definition);
    the streaming form takes any list of calls, e.g. a pattern cut into pieces (`cut`);
  * `batch_inputs` on Montgomery limb arrays, a whole batch at once, with the permutation passed in (the C oracle's
    perm_batch), for the GPU tier;
  * `walk`, the steps between permutations as the kernel derives them -- (e0, j, a0, k): emit j words at positions e0..,
    then add k words at positions a0.. -- with `inputs_by_walk`, which rebuilds the input states from those steps alone, so
    that the walk is itself checked against the definition.  `cursor` is the ABI's: pos_absorb | pos_squeeze << 4.
"""
from __future__ import annotations

import numpy as np

import safe_model as M
from safe_model import A, P, Q, S  # noqa: F401


def stream_inputs(calls, inputs, tag: int, perm=S.perm):
    """Any sequence of calls on a fresh sponge -> (input states [S][5], outputs in call order)."""
    states = []

    def recording(st):
        states.append(list(st))
        return perm(list(st))

    sp, out, at = M.Sponge(tag, recording), [], 0
    for kind, n in calls:
        if kind == "absorb":
            sp.absorb(inputs[at:at + n])
            at += n
        else:
            out += sp.squeeze(n)
    assert at == len(inputs)
    return states, out


def chain_inputs(pattern, inputs, tag: int, perm=S.perm):
    """A valid IO pattern -> (input states [S][5], outputs)."""
    assert M.valid(pattern) and len(inputs) == M.words_in(pattern)
    return stream_inputs(pattern, inputs, tag, perm)


def cut(pattern, pieces):
    """The aggregated pattern with call c cut into the lengths pieces[c] -> the list of streaming calls."""
    agg = M.aggregate(pattern)
    assert len(pieces) == len(agg) and all(sum(p) == n and min(p) > 0 for p, (_, n) in zip(pieces, agg))
    return [(kind, k) for (kind, _), p in zip(agg, pieces) for k in p]


def cuts(length):
    """every way of cutting `length` words into consecutive calls"""
    import itertools
    for k in range(length):
        for at in itertools.combinations(range(1, length), k):
            edges = (0,) + at + (length,)
            yield [b - a for a, b in zip(edges, edges[1:])]


# ---- the kernel's walk ---------------------------------------------------------------------------------------------------
def walk(calls, cursor: int = 0):
    """One launch serving `calls` from `cursor` -> (steps [(e0, j, a0, k)] -- one before each permutation and a final one,
    so len(steps) - 1 permutations --, cursor afterwards)."""
    agg = M.aggregate(calls)
    pa, ps = cursor & 15, cursor >> 4
    ci, rem, steps = 0, agg[0][1], []
    while True:
        e0, j, a0, k = ps, 0, pa, 0
        if ci < len(agg) and agg[ci][0] == "squeeze" and ps < 4:
            j = min(rem, 4 - ps)
            rem -= j
            ps += j
            if rem == 0:
                ci += 1
                rem = agg[ci][1] if ci < len(agg) else 0
        if ci < len(agg) and agg[ci][0] == "absorb" and pa < 4:
            k = min(rem, 4 - pa)
            rem -= k
            pa += k
            ps = 4
            if rem == 0:
                ci += 1
                rem = agg[ci][1] if ci < len(agg) else 0
        steps.append((e0, j, a0, k))
        if ci == len(agg):
            return steps, pa | (ps << 4)
        pa = 0                                         # a permutation
        if agg[ci][0] == "squeeze":
            ps = 0


def inputs_by_walk(launches, inputs, tag: int, perm=S.perm):
    """`launches`: a list of call lists, one per streaming call (or [pattern] for the one-shot call), served by `walk`
    step by step -> (input states, outputs, steps of every launch, final cursor)."""
    state, cursor, at = [tag % P, 0, 0, 0, 0], 0, 0
    states, out, all_steps = [], [], []
    for calls in launches:
        steps, cursor = walk(calls, cursor)
        for t, (e0, j, a0, k) in enumerate(steps):
            out += state[1 + e0:1 + e0 + j]
            for q in range(k):
                state[1 + a0 + q] = (state[1 + a0 + q] + inputs[at + q]) % P
            at += k
            if t + 1 < len(steps):
                states.append(list(state))
                state = perm(list(state))
        all_steps.append(steps)
    assert at == len(inputs)
    return states, out, all_steps, cursor


# ---- batches in the memory format ---------------------------------------------------------------------------------------
def batch_inputs(calls, inputs, tag_mont: int, perm_batch):
    """inputs [n, words in, 4] (uint64 Montgomery limbs) -> (input states [S, n, 5, 4], outputs [n, words out, 4], the
    final states [n, 5, 4]); `calls` is any sequence of calls on fresh sponges."""
    n_in = sum(k for kind, k in calls if kind == "absorb")
    inputs = np.asarray(inputs, dtype=np.uint64).reshape(-1, n_in, 4)
    n = inputs.shape[0]
    states = []

    def recording(flat):
        states.append(np.array(flat, dtype=np.uint64).reshape(n, 5, 4))
        return perm_batch(flat)

    sp, outs, at = M.SpongeBatch(n, tag_mont, recording), [], 0
    for kind, k in calls:
        if kind == "absorb":
            sp.absorb(inputs[:, at:at + k])
            at += k
        else:
            outs.append(sp.squeeze(k))
    out = np.concatenate(outs, axis=1) if outs else np.empty((n, 0, 4), dtype=np.uint64)
    return np.array(states, dtype=np.uint64).reshape(len(states), n, 5, 4), out, sp.state


# the one-shot patterns of the GPU tier: together they reach every step shape (j, k), 0 <= j, k <= 4, except (0, 0)
GPU_PATTERNS = [
    [A(1), Q(1)], [A(4), Q(1)], [A(5), Q(1)], [A(3), Q(2), A(2), Q(1)], [A(2), A(1), Q(5), A(5), Q(1)], [A(1), Q(64)],
    [A(8), Q(8)], [A(1), Q(2)], [A(6), Q(7)], [A(2), Q(1), A(2), Q(2)],
    [A(9), Q(4), A(4), Q(3), A(3), Q(4), A(1), Q(3), A(2), Q(4), A(3), Q(1), A(4), Q(2), A(4), Q(3), A(1), Q(2), A(1), Q(1),
     A(1), Q(1)],
    [A(2), Q(1), A(3), Q(1), A(4), Q(3), A(2), Q(3), A(3), Q(3), A(4), Q(2), A(3), Q(4), A(2), Q(4), A(4), Q(1)]]
GPU_PATTERN_PERMS = [1, 1, 2, 2, 4, 16, 3, 1, 3, 2, 13, 9]
# the patterns the GPU tier cuts every way into streaming calls
GPU_CUT_PATTERNS = [[A(3), Q(2), A(2), Q(1)], [A(5), Q(6)], [A(2), A(1), Q(1), Q(2)]]
