"""Big-integer model of the input states of the mixed-height commitment witness (include/hades252.h, f17): the chain of one
opening, step by step, from the definitions of tests/mmcs_model.py (the shape, the tampers, the root it must end in),
tests/witness_chain_model.py (the sponge's block count) and the oracle's permutation, and nothing else.  Scalars are the
integers of their in-memory Montgomery words (addition mod p is the same there), so the states compare byte for byte with
what the library writes.

One opening is P = permutations(cols, depth, pad_mode) steps, in the order k_mmcs_verify walks them; `steps` names them,
`chain` gives the state that enters and the state that leaves each, `links` the copy constraints a circuit places between
them."""
import numpy as np

import mmcs_model as MM
import oracle_lib
import witness_chain_model as WC
from gpu_common import CAP, TAG
import hades_spec as S

P = oracle_lib.P
ONE = S.to_mont(1)                      # the pad scalar, as the library holds it
SPONGE, INJECT, CLIMB = 0, 1, 2         # HADES252_WMMCS_SPONGE / _INJECT / _CLIMB


def steps(heights, cols, arity, pad_mode):
    """[(kind, group, ordinal)]: per group its row's blocks, its injection (g > 0), the levels up to the next group's height;
    ordinal = the block, 0, or the child level counted from the leaves.  A climb step's group is the last one hashed."""
    depths = [MM.depth_of(h, arity) for h in heights] + [0]
    out, level = [], 0
    for g, c in enumerate(cols):
        out += [(SPONGE, g, b) for b in range(WC.sponge_blocks(c, pad_mode))]
        if g > 0:
            out.append((INJECT, g, 0))
        for _ in range(depths[g] - depths[g + 1]):
            out.append((CLIMB, g, level))
            level += 1
    return out


def _ints(words):
    return [oracle_lib.int_of(w) for w in np.asarray(words, dtype=np.uint64).reshape(-1, 4)]


def _words(states):
    return np.array([oracle_lib.limbs_of(v) for st in states for v in st], dtype=np.uint64).reshape(len(states), 5, 4)


def chain(oracle, rows, heights, index, path, arity, cap=CAP, pad_mode=1, tag=None, inject_tag=MM.INJECT, out_idx=1):
    """-> (inputs uint64 [P, 5, 4], outputs uint64 [P, 5, 4]) of one opening: rows[g] [c_g, 4] tallest first, `path`
    [depth, arity - 1, 4]; the index is not range-checked."""
    tag = TAG[arity] if tag is None else tag
    sibs = [_ints(level) for level in np.asarray(path, dtype=np.uint64).reshape(-1, arity - 1, 4)]
    ins, outs, prev, node = [], [], None, None
    for kind, g, o in steps(heights, [len(np.asarray(r).reshape(-1, 4)) for r in rows], arity, pad_mode):
        if kind == SPONGE:
            row = _ints(rows[g])
            n_blocks = WC.sponge_blocks(len(row), pad_mode)
            m = row + ([ONE] if pad_mode == 1 else [])
            m += [0] * (4 * n_blocks - len(m))
            st = [cap % P, 0, 0, 0, 0] if o == 0 else prev
            inp = [st[0]] + [(st[1 + k] + m[4 * o + k]) % P for k in range(4)]
        elif kind == INJECT:
            inp = [inject_tag % P, node, prev[1], 0, 0]
        else:
            pos = (int(index) // arity ** o) % arity
            inp = [tag % P] + sibs[o][:pos] + [node] + sibs[o][pos:] + [0] * (4 - arity)
        out = _ints(oracle.perm_batch(_words([inp]).reshape(-1), threads=1))
        if kind != SPONGE:
            node = out[out_idx]
        elif g == 0 and o == n_blocks - 1:
            node = out[1]
        ins.append(inp)
        outs.append(out)
        prev = out
    return _words(ins), _words(outs)


def batch(oracle, rows, heights, indices, paths, arity, **kw):
    """The chains of n openings as the library lays them: -> (inputs [P, n, 5, 4], outputs [P, n, 5, 4]); rows[q] is the
    list of query q's opened rows."""
    both = [chain(oracle, rows[q], heights, indices[q], paths[q], arity, **kw) for q in range(len(indices))]
    return np.stack([b[0] for b in both], axis=1), np.stack([b[1] for b in both], axis=1)


def first_affected(table, what, cols, depth):
    """The first step whose input a tamper of mmcs_model.tampers changes: the block that holds the tampered column of group
    g's row ("row g": column cols[g] // 2), the tampered level ("sibling": depth // 2), the first level ("index": the next
    index sits at another child position there)."""
    if what.startswith("row "):
        g = int(what.split()[1])
        return table.index((SPONGE, g, cols[g] // 2 // 4))
    level = depth // 2 if what == "sibling" else 0
    return [t for t, (kind, _, o) in enumerate(table) if kind == CLIMB and o == level][0]


def links(heights, cols, index, arity, pad_mode, out_idx=1):
    """The copy constraints between the records of one opening: [(t, word, from_t, from_word)] -- input word `word` of step
    t is output word `from_word` of step `from_t`.  Inject: the node (the last climb before the group's sponge) and the
    digest (the group's last block); climb: the node at its child position (the step before: word 1 of group 0's last block
    for the first level, else word out_idx); sponge block b > 0: the capacity word passes through."""
    out = []
    for t, (kind, g, o) in enumerate(steps(heights, cols, arity, pad_mode)):
        if kind == INJECT:
            out.append((t, 1, t - 1 - WC.sponge_blocks(cols[g], pad_mode), out_idx))
            out.append((t, 2, t - 1, 1))
        elif kind == CLIMB:
            out.append((t, 1 + (int(index) // arity ** o) % arity, t - 1, 1 if o == 0 else out_idx))
        elif o > 0:
            out.append((t, 0, t - 1, 0))
    return out
