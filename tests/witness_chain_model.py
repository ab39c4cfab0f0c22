"""Big-integer model of the input states of the chain witnesses (include/hades252.h, "gadget witnesses of permutation
chains"), on the spec oracle (oracle/hades_spec.py).  Values are canonical integers (not Montgomery form).

A batch of n chains of S steps is S * n permutations; inputs[s][i] is the state that enters permutation (s, i).
  sponge:  inputs[0][i] = [capacity, block 0]; inputs[s][i] = perm(inputs[s - 1][i]) with block s added to words 1..4
  Merkle:  inputs[l][q] = [tag, the arity children of the level-l group on leaf indices[q]'s path, 0 ...], a child past the
           end of level l = pad[l] (zero without a table); an index >= n_leaves gets all-zero states.

`perm_many` (a list of states -> the list of their permutations) defaults to the spec's `perm`, one state at a time; a
caller with many states may hand in a batched one (the C oracle)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402

P = S.P
WIRES = 972
LAST_ROW = WIRES - 9            # wire of r2[0] of the last round; r2[j] = LAST_ROW + 2 j: the permutation's output


def _spec_perm_many(states):
    return [S.perm(list(s)) for s in states]


def sponge_blocks(msg_len: int, pad_mode: int = 1) -> int:
    if pad_mode not in (0, 1):
        return 0
    return max(1, -(-(msg_len + pad_mode) // 4))


def padded_blocks(msg, pad_mode: int = 1):
    """The message as S blocks of 4 scalars: pad_mode 1 appends a single 1, then zeros; at least one block."""
    m = list(msg) + ([1] if pad_mode == 1 else [])
    m += [0] * (4 * sponge_blocks(len(msg), pad_mode) - len(m))
    return [m[4 * b:4 * b + 4] for b in range(len(m) // 4)]


def sponge_inputs(msgs, capacity: int, pad_mode: int = 1, perm_many=None):
    """-> (inputs [S][n][5], outputs [n][5]: the final states).  Every message of `msgs` has the same length."""
    perm_many = perm_many or _spec_perm_many
    blocks = [padded_blocks(m, pad_mode) for m in msgs]
    n_steps = sponge_blocks(len(msgs[0]) if msgs else 0, pad_mode)
    assert all(len(b) == n_steps for b in blocks), "messages of one batch have one length"
    state = [[capacity % P, 0, 0, 0, 0] for _ in msgs]
    inputs = []
    for s in range(n_steps):
        step = []
        for i, st in enumerate(state):
            step.append([st[0]] + [(st[1 + k] + blocks[i][s][k]) % P for k in range(4)])
        inputs.append(step)
        state = perm_many(step)
    return inputs, state


def merkle_levels(leaves, arity: int, tag: int, out_idx: int = 1, pad=None, perm_many=None):
    """[level 0 = the leaves, level 1, ..., [root]]: parent = perm([tag, children, 0 ...])[out_idx], a missing child of
    level l = pad[l] (zero without a table)."""
    perm_many = perm_many or _spec_perm_many
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        l, cur = len(levels) - 1, levels[-1]
        fill = 0 if pad is None else pad[l]
        states = []
        for g in range(0, len(cur), arity):
            ch = cur[g:g + arity]
            ch = ch + [fill] * (arity - len(ch))
            states.append([tag % P] + ch + [0] * (4 - arity))
        levels.append([o[out_idx] for o in perm_many(states)])
    return levels


def merkle_path_inputs(levels, arity: int, tag: int, indices, pad=None):
    """inputs [depth][n_queries][5] of the openings of `indices` in the tree `levels` (merkle_levels' layout)."""
    depth = len(levels) - 1
    n_leaves = len(levels[0])
    out = []
    for l in range(depth):
        step = []
        for idx in indices:
            if idx >= n_leaves:
                step.append([0] * 5)
                continue
            node = idx // arity ** l
            first = node - node % arity
            ch = [levels[l][first + k] if first + k < len(levels[l]) else (0 if pad is None else pad[l])
                  for k in range(arity)]
            step.append([tag % P] + ch + [0] * (4 - arity))
        out.append(step)
    return out


def path_position(idx: int, arity: int, level: int) -> int:
    """Word (1 + position) of inputs[level] that holds the path node of that level."""
    return 1 + (idx // arity ** level) % arity
