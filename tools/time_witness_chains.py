"""Device-side timing of the chain witnesses (hades252_sponge_witness_dev, hades252_merkle_open_witness_dev) against
hades252_perm_witness_dev at the same permutation count, in one process.

    python tools/time_witness_chains.py [--reps 3]

Shapes: perm_witness on 2^20 states; the sponge witness at 2^19 messages x 2 blocks (msg_len 7, pad 10: 2^20 permutations);
perm_witness on 10 x 2^17 states and the Merkle witness at depth 10 (2^20 leaves, arity 4) x 2^17 queries; one two-block
message per call (latency).  Every shape is warmed up, then timed over `reps` back-to-back calls between two device events.
Prints one line per shape -- permutations/s and the ratio to perm_witness at the same count -- and a final JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from hades252_amd import strategy as H, _lib  # noqa: E402
from timing import WIRES, perm_witness_rate, report, timed  # noqa: E402

P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def mont(v):
    return v * (1 << 256) % P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    cap = H._tag_arr(mont(1 << 64))                    # the "sponge/pad10" capacity of include/hades252.h
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": []}

    # ---- sponge: 2^19 messages x 2 blocks ----
    n, msg_len = 1 << 19, 7
    n_perms = 2 * n
    wires = torch.empty((WIRES, n_perms, 4), dtype=torch.int64, device=dev)
    ref = perm_witness_rate(out["rows"], n_perms, wires, args.reps)
    msgs = H.gen_b(n * msg_len, dev, first_elem=1 << 30)
    inputs = torch.empty((n_perms, 5, 4), dtype=torch.int64, device=dev)
    t = timed(lambda: _lib.check(lib.hades252_sponge_witness_dev(msgs.data_ptr(), n, msg_len, cap, 1, inputs.data_ptr(),
                                                                 wires.data_ptr(), None, stream()), "sponge_witness"),
              args.reps)
    report(out["rows"], "sponge_witness", n_perms, t, ref, "  n=%d msg_len=%d" % (n, msg_len))
    del msgs, inputs, wires

    # ---- Merkle: depth 10 (2^20 leaves, arity 4) x 2^17 queries ----
    arity, n_leaves, nq = 4, 1 << 20, 1 << 17
    tag_mont = mont(15)                                # the "merkle/arity4" tag
    leaves = H.gen_b(n_leaves, dev, first_elem=1 << 33)
    tree = H.merkle_build(leaves, arity, tag_mont, 1)
    depth = H.merkle_depth(n_leaves, arity)
    n_perms = depth * nq
    wires = torch.empty((WIRES, n_perms, 4), dtype=torch.int64, device=dev)
    ref = perm_witness_rate(out["rows"], n_perms, wires, args.reps)
    idx = torch.randint(0, n_leaves, (nq,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    inputs = torch.empty((n_perms, 5, 4), dtype=torch.int64, device=dev)
    tg = H._tag_arr(tag_mont)
    t = timed(lambda: _lib.check(lib.hades252_merkle_open_witness_dev(leaves.data_ptr(), tree.data_ptr(), n_leaves, arity, tg,
                                                                      None, idx.data_ptr(), nq, inputs.data_ptr(),
                                                                      wires.data_ptr(), None, stream()),
                                 "merkle_open_witness"), args.reps)
    report(out["rows"], "merkle_witness", n_perms, t, ref, "  depth=%d queries=%d" % (depth, nq))
    del leaves, tree, wires, inputs

    # ---- one two-block message per call ----
    msg = H.gen_b(msg_len, dev, first_elem=5)
    inputs = torch.empty((2, 5, 4), dtype=torch.int64, device=dev)
    wires = torch.empty((WIRES, 2, 4), dtype=torch.int64, device=dev)
    reps1 = max(args.reps, 50)
    t1 = timed(lambda: _lib.check(lib.hades252_sponge_witness_dev(msg.data_ptr(), 1, msg_len, cap, 1, inputs.data_ptr(),
                                                                  wires.data_ptr(), None, stream()), "sponge_witness"), reps1)
    print("one message x 2 blocks: %.1f us / call (%d back-to-back calls)" % (t1 * 1e6, reps1), flush=True)
    out["one_message_2_blocks_us"] = {"us": t1 * 1e6, "calls": reps1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
