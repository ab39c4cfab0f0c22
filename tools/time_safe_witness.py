"""Device-side timing of the duplex sponge witness (hades252_safe_witness_dev) against hades252_perm_witness_dev at the same
number of records, in one process.

    python tools/time_safe_witness.py [--reps 3]

Shapes: perm_witness on 2^20 states, then [A4,S1] x 2^20 sponges (S = 1), [A3,S2,A2,S1] x 2^19 (S = 2) and the
squeeze-heavy [A1,S8] x 2^19 (S = 2): 2^20 records each, the target is 0.9 x perm_witness.  Two figures without a target:
[A1,S64] x 2^16 (S = 16, 2^20 records, but 2^16 lanes are one wave per SIMD against perm_witness's three: the latency of a
long chain, not the kernel's rate) and one sponge of [A4,S1] per call.  Every shape is warmed up, then timed over `reps`
back-to-back calls between two device events.  Prints one line per shape -- permutations/s and the ratio to perm_witness
at the same count -- and a final JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from hades252_amd import strategy as H, _lib  # noqa: E402
from timing import WIRES, perm_witness_rate, timed, witness_line  # noqa: E402

A = lambda n: ("absorb", n)      # noqa: E731
Q = lambda n: ("squeeze", n)     # noqa: E731
TARGET = 0.9


def name(pattern):
    return "[" + ",".join("%s%d" % ("A" if kind == "absorb" else "S", n) for kind, n in pattern) + "]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    tag = H._tag_arr(0x5AFE)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "target": TARGET, "rows": []}

    n_perms = 1 << 20
    wires = torch.empty((WIRES, n_perms, 4), dtype=torch.int64, device=dev)
    inputs = torch.empty((n_perms, 5, 4), dtype=torch.int64, device=dev)
    ref = perm_witness_rate(out["rows"], n_perms, wires, args.reps, width=34)

    for pattern, n, targeted in (([A(4), Q(1)], 1 << 20, True), ([A(3), Q(2), A(2), Q(1)], 1 << 19, True),
                                 ([A(1), Q(8)], 1 << 19, True), ([A(1), Q(64)], 1 << 16, False)):
        n_in, n_out, S = H.safe_pattern(pattern)
        assert S * n == n_perms
        arr, k = H._safe_calls(pattern, "time_safe_witness")
        d_in = H.gen_b(n * n_in, dev, first_elem=1 << 30)
        d_out = torch.empty((n, n_out, 4), dtype=torch.int64, device=dev)
        t = timed(lambda: _lib.check(lib.hades252_safe_witness_dev(d_in.data_ptr(), n, arr, k, tag, inputs.data_ptr(),
                                                                   wires.data_ptr(), d_out.data_ptr(), stream()),
                                     "safe_witness"), args.reps)
        ratio = n_perms / t / ref
        row = {"op": "safe_witness", "pattern": name(pattern), "sponges": n, "steps": S, "perms": n_perms, "ms": t * 1e3,
               "perms_per_s": n_perms / t, "vs_perm_witness": ratio, "targeted": targeted}
        if targeted:
            row["meets_target"] = ratio >= TARGET
        out["rows"].append(row)
        print("%s  (%.3f x perm_witness%s)"
              % (witness_line("safe_witness %s x 2^%d" % (name(pattern), n.bit_length() - 1), n_perms, t, width=34), ratio,
                 ", target %.1f: %s" % (TARGET, "met" if ratio >= TARGET else "MISSED") if targeted else ", no target"),
              flush=True)
        del d_in, d_out

    # ---- one sponge of [A4,S1] per call ----
    pattern = [A(4), Q(1)]
    arr, k = H._safe_calls(pattern, "time_safe_witness")
    d_in = H.gen_b(4, dev, first_elem=5)
    reps1 = max(args.reps, 50)
    t1 = timed(lambda: _lib.check(lib.hades252_safe_witness_dev(d_in.data_ptr(), 1, arr, k, tag, inputs.data_ptr(),
                                                                wires.data_ptr(), None, stream()), "safe_witness"), reps1)
    print("one sponge [A4,S1] (1 permutation): %.1f us / call (%d back-to-back calls)" % (t1 * 1e6, reps1), flush=True)
    out["one_sponge_a4s1_us"] = {"us": t1 * 1e6, "calls": reps1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
