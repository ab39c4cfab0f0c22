"""GPU tier, row f4 extended to chains: the gadget witnesses of the fixed-length sponge (hades252_sponge_witness_dev) and
of Merkle openings (hades252_merkle_open_witness_dev).  The defining property wires == perm_witness(inputs), byte for byte,
on every case; the inputs against the big-integer model (tests/witness_chain_model.py, over the C oracle's perm_batch);
sampled records against the spec's GadgetStrategy wire for wire; digests, guard words, untouched inputs, a non-default
stream, out-of-range indices, and both constructions at scale.  Conventions of f1 / f2 (UNPINNED, include/hades252.h)."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import witness_chain_model as W  # noqa: E402
from witness_chain_model import P, S  # noqa: E402
from gpu_common import to_dev, to_host, TAG, CAP, Guarded, gadget_check, mont_rows, perm_many_over  # noqa: E402
from oracle_lib import limbs_of, int_of  # noqa: E402

pytestmark = pytest.mark.gpu


def _messages(rng, n, msg_len):
    kinds = [lambda: 0, lambda: P - 1, lambda: rng.randrange(P)]
    out = []
    for i in range(n):
        if i % 4 == 3:                                             # mixed words
            out.append([rng.choice(kinds)() for _ in range(msg_len)])
        else:
            out.append([kinds[i % 4]() for _ in range(msg_len)])
    return out


@pytest.mark.parametrize("pad_mode", [0, 1])
@pytest.mark.parametrize("msg_len", [0, 1, 3, 4, 5, 8, 13])
def test_sponge_witness_against_model_and_perm_witness(torch_cuda, H, hades_lib, oracle, msg_len, pad_mode):
    torch = torch_cuda
    for n in (1, 63, 64, 65, 257):
        rng = random.Random(1000 * msg_len + 10 * n + pad_mode)
        msgs = _messages(rng, n, msg_len)
        cap = rng.choice([CAP, S.to_mont(rng.randrange(P))])
        S_ = W.sponge_blocks(msg_len, pad_mode)
        assert hades_lib.hades252_sponge_blocks(msg_len, pad_mode) == S_
        host_msgs = mont_rows([v for m in msgs for v in m]) if msg_len else np.zeros((0, 4), dtype=np.uint64)
        dm = to_dev(torch, host_msgs.reshape(-1)) if msg_len else torch.zeros(0, dtype=torch.int64, device="cuda")
        g_wires, g_inputs, g_dig = Guarded(torch, (W.WIRES, S_ * n, 4)), Guarded(torch, (S_ * n, 20)), Guarded(torch, (n, 4))
        capa = (ctypes.c_uint64 * 4)(*limbs_of(cap))
        rc = hades_lib.hades252_sponge_witness_dev(dm.data_ptr() if msg_len else None, n, msg_len, capa, pad_mode,
                                                   g_inputs.ptr, g_wires.ptr, g_dig.ptr, None)
        assert rc == 0
        wires, inputs, dig = (g.check((n, msg_len)) for g in (g_wires, g_inputs, g_dig))    # guards whole, all written
        if msg_len:
            assert (to_host(dm) == host_msgs.reshape(-1)).all()                     # messages untouched
        # inputs against the model
        exp_in, exp_out = W.sponge_inputs(msgs, S.from_mont(cap), pad_mode, perm_many_over(oracle))
        got_in = to_host(inputs).reshape(S_, n, 5, 4)
        assert (got_in == mont_rows([v for step in exp_in for st in step for v in st]).reshape(S_, n, 5, 4)).all(), n
        # the defining property
        ref = H.perm_witness(inputs)
        assert torch.equal(wires, ref), n
        # digests: hades252_sponge_hash_dev and the model
        ref_d = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        assert hades_lib.hades252_sponge_hash_dev(dm.data_ptr() if msg_len else None, n, msg_len, capa, pad_mode,
                                                  ref_d.data_ptr(), None) == 0
        assert torch.equal(dig, ref_d), n
        assert (to_host(ref_d).reshape(n, 4) == mont_rows([o[1] for o in exp_out])).all()
        # sampled records against the spec's GadgetStrategy, wire for wire
        wires_h = to_host(wires).reshape(W.WIRES, S_, n, 4)
        pairs = {(0, 0), (S_ - 1, n - 1), (rng.randrange(S_), rng.randrange(n))}
        gadget_check(wires_h, got_in, sorted(pairs))
        if n == 65:                                   # the Python layer: same bytes, shapes [972, S, n, 4] / [S, n, 5, 4]
            src = dm.view(n, msg_len, 4) if msg_len else torch.zeros((n, 0, 4), dtype=torch.int64, device="cuda")
            pw, pi, pd = H.sponge_witness(src, msg_len, cap, pad_mode, digests=True)
            assert tuple(pw.shape) == (W.WIRES, S_, n, 4) and tuple(pi.shape) == (S_, n, 5, 4)
            assert torch.equal(pw.view(-1), wires.view(-1)) and torch.equal(pi.view(-1), inputs.view(-1))
            assert torch.equal(pd, ref_d)


def test_sponge_witness_at_scale_on_a_side_stream(torch_cuda, H):
    """2^17 messages x 2 blocks (msg_len 7, pad 10), on a non-default stream: wires == perm_witness(inputs) with torch.equal,
    digests == sponge_hash, and the final r2 of block 0 + block 1 == the inputs of block 1."""
    torch = torch_cuda
    n, msg_len = 1 << 17, 7
    msgs = H.gen_b(n * msg_len, "cuda", first_elem=777)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wires, inputs, dig = H.sponge_witness(msgs, msg_len, CAP, 1, digests=True)
    side.synchronize()
    assert tuple(wires.shape) == (W.WIRES, 2, n, 4)
    ref = H.perm_witness(inputs.view(2 * n, 20))
    assert torch.equal(wires.view(W.WIRES, 2 * n, 4), ref)
    del ref
    assert torch.equal(dig, H.sponge_hash(msgs, msg_len, CAP, 1))
    out0 = torch.stack([wires[W.LAST_ROW + 2 * j, 0] for j in range(5)], dim=1)          # [n, 5, 4]
    blk = msgs.view(n, msg_len, 4)[:, 4:7]
    for k in range(3):
        assert torch.equal(inputs[1, :, 1 + k].contiguous(), H.fr_op(H.FR_ADD, out0[:, 1 + k].contiguous(), blk[:, k].contiguous()))
    assert torch.equal(inputs[1, :, 0], out0[:, 0])


def _merkle_case(torch, H, oracle, n_leaves, arity, tag, out_idx, with_pad, seed):
    depth = H.merkle_depth(n_leaves, arity)
    leaves = H.gen_b(n_leaves, "cuda", first_elem=seed)
    pad = H.merkle_empty_digests(arity, depth, S.to_mont(seed % 97 + 1), tag, out_idx) if with_pad else None
    tree = H.merkle_build(leaves, arity, tag, out_idx, pad=pad)
    return depth, leaves, pad, tree


def _path_checks(torch, wires, inputs, tree, idx, n_leaves, arity, out_idx, depth):
    """On the device: r2[out_idx] of level l == the path child in inputs[l + 1]; the top level's == the root."""
    row = W.LAST_ROW + 2 * out_idx
    ok = idx < n_leaves
    for l in range(depth):
        got = wires[row, l][ok]
        if l + 1 < depth:
            pos = (idx[ok] // arity ** (l + 1)) % arity + 1
            want = inputs[l + 1][ok].gather(1, pos.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
        else:
            want = tree[-1].view(1, 4).expand(int(ok.sum().item()), 4)
        assert torch.equal(got, want), l


@pytest.mark.parametrize("arity", [2, 3, 4])
def test_merkle_open_witness_against_model_and_perm_witness(torch_cuda, H, hades_lib, oracle, arity):
    torch = torch_cuda
    for n_leaves, with_pad, out_idx, tag in ((arity ** 4, False, 1, TAG[arity]), (arity ** 4, True, 2, S.to_mont(99)),
                                             (2 * arity ** 3 + 1, True, 1, TAG[arity]),
                                             (arity ** 3 + arity + 1, False, 0, S.to_mont(5))):
        depth, leaves, pad, tree = _merkle_case(torch, H, oracle, n_leaves, arity, tag, out_idx, with_pad, n_leaves)
        rng = random.Random(n_leaves * arity + out_idx)
        last_group = n_leaves - 1 - (n_leaves - 1) % arity
        idx_list = [0, n_leaves - 1, last_group, rng.randrange(n_leaves), n_leaves, n_leaves + 7, 2 ** 64 - 1, 1]
        idx_t = torch.tensor(np.array(idx_list, dtype=np.uint64).view(np.int64), device="cuda")
        wires, inputs, n_bad = H.merkle_open_witness(leaves, tree, arity, idx_t, tag, pad=pad)
        nq = len(idx_list)
        assert n_bad == 3
        assert tuple(wires.shape) == (W.WIRES, depth, nq, 4) and tuple(inputs.shape) == (depth, nq, 5, 4)
        assert torch.equal(wires.view(W.WIRES, depth * nq, 4), H.perm_witness(inputs.view(depth * nq, 20)))
        # the model, from the leaves alone
        lv = [S.from_mont(int_of(r)) for r in to_host(leaves).reshape(-1, 4)]
        pv = None if pad is None else [S.from_mont(int_of(r)) for r in to_host(pad).reshape(-1, 4)]
        levels = W.merkle_levels(lv, arity, S.from_mont(tag), out_idx, pv, perm_many_over(oracle))
        assert S.to_mont(levels[-1][0]) == int_of(to_host(tree[-1]))
        exp = W.merkle_path_inputs(levels, arity, S.from_mont(tag), idx_list, pv)
        got = to_host(inputs).reshape(depth, nq, 5, 4)
        want = mont_rows([v for step in exp for st in step for v in st]).reshape(depth, nq, 5, 4)
        assert (got == want).all(), (n_leaves, arity)
        assert (got[:, 4:7] == 0).all()                               # out-of-range indices: all-zero states
        _path_checks(torch, wires, inputs, tree, torch.tensor(idx_list[:4] + [n_leaves] * 3 + [1], device="cuda"),
                     n_leaves, arity, out_idx, depth)
        # guard words and untouched inputs through the C entry point
        guard_w, guard_i = Guarded(torch, (W.WIRES, depth * nq, 4)), Guarded(torch, (depth * nq, 20))
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        leaves_before, tree_before = leaves.clone(), tree.clone()
        tg = (ctypes.c_uint64 * 4)(*limbs_of(tag))
        rc = hades_lib.hades252_merkle_open_witness_dev(leaves.data_ptr(), tree.data_ptr(), n_leaves, arity, tg,
                                                        None if pad is None else pad.data_ptr(), idx_t.data_ptr(), nq,
                                                        guard_i.ptr, guard_w.ptr, bad.data_ptr(), None)
        assert rc == 0
        guard_i.check((n_leaves, arity))                              # guards whole, every word written (zero states too)
        assert torch.equal(guard_w.check((n_leaves, arity)).view(-1), wires.view(-1))
        assert int(bad.item()) == 3
        assert torch.equal(leaves, leaves_before) and torch.equal(tree, tree_before)


def test_merkle_open_witness_at_scale(torch_cuda, H):
    """2^20 leaves at arity 4 (depth 10), 2^14 queries: one 163 840-state perm_witness launch; inputs against a gather in
    torch, wires == perm_witness(inputs), every level's output wire == the path child of the next, the top == the root."""
    torch = torch_cuda
    arity, n_leaves, nq, tag = 4, 1 << 20, 1 << 14, TAG[4]
    leaves = H.gen_b(n_leaves, "cuda", first_elem=99)
    tree = H.merkle_build(leaves, arity, tag, 1)
    depth = H.merkle_depth(n_leaves, arity)
    g = torch.Generator(device="cuda").manual_seed(5)
    idx = torch.randint(0, n_leaves, (nq,), device="cuda", generator=g)
    wires, inputs, n_bad = H.merkle_open_witness(leaves, tree, arity, idx, tag)
    assert n_bad == 0 and depth == 10
    assert torch.equal(wires.view(W.WIRES, depth * nq, 4), H.perm_witness(inputs.view(depth * nq, 20)))
    levels = [leaves]
    off = 0
    for n_l in H.merkle_level_sizes(n_leaves, arity):
        levels.append(tree[off:off + n_l])
        off += n_l
    tag_row = torch.tensor(np.array(limbs_of(tag), dtype=np.uint64).view(np.int64), device="cuda")
    for l in range(depth):
        first = (idx // arity ** l) // arity * arity
        want = torch.stack([levels[l][first + k] for k in range(arity)], dim=1)
        assert torch.equal(inputs[l, :, 1:], want), l
        assert torch.equal(inputs[l, :, 0], tag_row.expand(nq, 4)), l
    _path_checks(torch, wires, inputs, tree, idx, n_leaves, arity, 1, depth)
