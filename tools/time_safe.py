"""Device-side timing of the batched duplex sponge (hades252_safe_hash_dev) against k_perm_fast, in one process.

    python tools/time_safe.py [--reps 5] [--log2n 24]

Shapes: k_perm_fast at 2^log2n states; n = 2^log2n sponges of [A(4), S(1)] and of [A(3), S(2), A(2), S(1)], 2^(log2n - 4)
sponges of [A(1), S(64)] (one sponge per lane, k_safe); one sponge of [A(4), S(1)] per call (one sponge per wave,
k_safe_lanes) beside one state per call through the one-state-per-wave permutation kernel.  Every shape is warmed up, then
timed over `reps` back-to-back calls between two device events.  Prints one line per shape -- sponges/s and the
perm-equivalent rate n * permutations per sponge / t -- and a final JSON line with the same numbers.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from hades252_amd import strategy as H, _lib  # noqa: E402
from timing import timed  # noqa: E402

TAG = 15 * (1 << 256) % H._FR_P


def name_of(pattern):
    return "[" + ", ".join("%s(%d)" % (kind[0].upper(), k) for kind, k in pattern) + "]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=24)
    args = ap.parse_args()
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    n = 1 << args.log2n
    tag = H._tag_arr(TAG)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "n": n, "reps": args.reps, "rows": []}

    states = H.gen_b(5 * n, dev)
    fast = H.ScalarStrategy(_lib.KERNEL_FAST)
    t = timed(lambda: fast.perm(states), args.reps)
    perm_rate = n / t
    print("k_perm_fast                      n=%-9d %9.3f ms  %8.1f M perms/s" % (n, t * 1e3, perm_rate / 1e6), flush=True)
    out["k_perm_fast"] = {"ms": t * 1e3, "perms_per_s": perm_rate}
    del states

    shapes = [(n, [("absorb", 4), ("squeeze", 1)]),
              (n, [("absorb", 3), ("squeeze", 2), ("absorb", 2), ("squeeze", 1)]),
              (max(n >> 4, 1), [("absorb", 1), ("squeeze", 64)])]
    for k, pattern in shapes:
        n_in, n_out, perms = H.safe_pattern(pattern)
        calls, n_calls = H._safe_calls(pattern, "time_safe")
        inputs = H.gen_b(k * n_in, dev)
        res = torch.empty((k, n_out, 4), dtype=torch.int64, device=dev)
        t = timed(lambda: _lib.check(lib.hades252_safe_hash_dev(inputs.data_ptr(), k, calls, n_calls, tag, res.data_ptr(),
                                                                stream()), "safe_hash"), args.reps)
        row = {"pattern": name_of(pattern), "n": k, "perms_per_sponge": perms, "ms": t * 1e3, "sponges_per_s": k / t,
               "perm_equiv_per_s": k * perms / t, "vs_k_perm_fast": k * perms / t / perm_rate}
        out["rows"].append(row)
        print("%-32s n=%-9d %9.3f ms  %8.1f M sponges/s  %8.1f M perm-equiv/s  (%.3f x k_perm_fast)"
              % (row["pattern"], k, t * 1e3, row["sponges_per_s"] / 1e6, row["perm_equiv_per_s"] / 1e6, row["vs_k_perm_fast"]),
              flush=True)
        del inputs, res

    # one sponge per call: the latency form, beside one state through the one-state-per-wave permutation kernel
    pattern = [("absorb", 4), ("squeeze", 1)]
    calls, n_calls = H._safe_calls(pattern, "time_safe")
    inputs, res = H.gen_b(4, dev), torch.empty((1, 1, 4), dtype=torch.int64, device=dev)
    one = H.gen_b(5, dev)
    lanes = H.ScalarStrategy(_lib.KERNEL_LANES)
    reps1 = max(args.reps, 50)
    t_perm = timed(lambda: lanes.perm(one), reps1)
    t_safe = timed(lambda: _lib.check(lib.hades252_safe_hash_dev(inputs.data_ptr(), 1, calls, n_calls, tag, res.data_ptr(),
                                                                 stream()), "safe_hash"), reps1)
    assert torch.equal(res.view(1, 4), H.merkle4_level(inputs, TAG))
    print("one sponge [A(4), S(1)]: %.1f us / call; one state through the one-state-per-wave permutation kernel: %.1f us / call "
          "(%d back-to-back calls each)" % (t_safe * 1e6, t_perm * 1e6, reps1), flush=True)
    out["one_sponge_a4s1_us"] = {"safe_hash": t_safe * 1e6, "perm_lanes": t_perm * 1e6, "calls": reps1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
