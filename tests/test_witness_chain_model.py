"""CPU tier: the model of the chain witnesses' input states (tests/witness_chain_model.py) against the spec and the C oracle
-- the sponge chain ends in S.sponge_hash and the oracle's sponge; every Merkle level's output word is the path child of the
next level's state, and the top one is the oracle tree's root (arity 2, 3, 4; full and ragged trees, padded or not)."""
import random

import numpy as np
import pytest

import witness_chain_model as W
from witness_chain_model import P, S
from oracle_lib import limbs_of, int_of


@pytest.mark.parametrize("pad_mode", [0, 1])
@pytest.mark.parametrize("msg_len", [0, 1, 3, 4, 5, 8, 13])
def test_sponge_chain_ends_in_the_sponge_hash(oracle, msg_len, pad_mode):
    rng = random.Random(msg_len * 2 + pad_mode)
    msgs = [[rng.randrange(P) for _ in range(msg_len)], [P - 1] * msg_len, [0] * msg_len]
    cap = rng.randrange(P)
    inputs, outs = W.sponge_inputs(msgs, cap, pad_mode)
    n_steps = W.sponge_blocks(msg_len, pad_mode)
    assert len(inputs) == n_steps and all(len(step) == len(msgs) for step in inputs)
    for i, m in enumerate(msgs):
        assert inputs[0][i][0] == cap
        for s in range(1, n_steps):                   # word 0 passes through; words 1..4 = previous output + block s
            prev = S.perm(list(inputs[s - 1][i]))
            block = W.padded_blocks(m, pad_mode)[s]
            assert inputs[s][i] == [prev[0]] + [(prev[1 + k] + block[k]) % P for k in range(4)]
        assert outs[i] == S.perm(list(inputs[-1][i]))
        assert outs[i][1] == S.sponge_hash(m, cap, pad_mode)
    if msg_len:
        flat = np.array([limbs_of(S.to_mont(v)) for m in msgs for v in m], dtype=np.uint64).reshape(-1)
        dig = oracle.sponge(flat, msg_len, S.to_mont(cap), pad_mode).reshape(-1, 4)
        assert [S.from_mont(int_of(d)) for d in dig] == [o[1] for o in outs]


@pytest.mark.parametrize("arity", [2, 3, 4])
@pytest.mark.parametrize("shape", ["full", "ragged"])
@pytest.mark.parametrize("padded", [False, True])
def test_merkle_path_states_chain_to_the_root(oracle, arity, shape, padded):
    rng = random.Random(arity * 10 + (shape == "ragged") * 2 + padded)
    n = arity ** 3 if shape == "full" else arity ** 2 + arity - 1
    leaves = [rng.randrange(P) for _ in range(n)]
    tag, out_idx = rng.randrange(P), arity - 1
    depth = 0
    while arity ** depth < n:
        depth += 1
    pad = None
    if padded:
        pad = [rng.randrange(P)]
        for _ in range(depth - 1):
            pad.append(S.perm([tag] + [pad[-1]] * arity + [0] * (4 - arity))[out_idx])
    levels = W.merkle_levels(leaves, arity, tag, out_idx, pad)
    assert len(levels) == depth + 1
    # the oracle's tree (Montgomery limbs) agrees level by level
    mleaves = np.array([limbs_of(S.to_mont(v)) for v in leaves], dtype=np.uint64).reshape(-1)
    mpad = None if pad is None else np.array([limbs_of(S.to_mont(v)) for v in pad], dtype=np.uint64).reshape(-1, 4)
    otree = oracle.merkle_tree(mleaves, arity, S.to_mont(tag), out_idx, mpad)
    for l in range(depth):
        assert [S.from_mont(int_of(r)) for r in otree[l].reshape(-1, 4)] == levels[l + 1], l
    indices = [0, n - 1, n - 1 - (n - 1) % arity, rng.randrange(n), n, n + 3]
    states = W.merkle_path_inputs(levels, arity, tag, indices, pad)
    assert len(states) == depth
    for q, idx in enumerate(indices):
        if idx >= n:
            assert all(states[l][q] == [0] * 5 for l in range(depth))
            continue
        for l in range(depth):
            st = states[l][q]
            assert st[0] == tag and st[1 + arity:] == [0] * (4 - arity)
            assert st[W.path_position(idx, arity, l)] == levels[l][idx // arity ** l]
            out = S.perm(list(st))[out_idx]
            if l + 1 < depth:
                assert out == states[l + 1][q][W.path_position(idx, arity, l + 1)], (idx, l)
            else:
                assert out == S.from_mont(int_of(otree[-1].reshape(-1, 4)[0])), idx
