"""Timing of the mixed-height commitment witnesses (hades252_wmmcs_*) against the fused verification and the bare witness
kernel -- per part in one process and one run, the routes alternating, every time a host clock around work that ends in a
device synchronise, best of --reps.

    python tools/time_mmcs_witness.py [--log2queries-inputs 18] [--log2queries-witness 15] [--reps 5] [--part all]

The opening shape is that of profiles/f14_mmcs's verify measurement: heights 2^20 / 2^16, columns 8 / 4, pad_mode 1, arity 2 --
3 + 2 blocks, 20 levels, one injection: 26 permutations per opening.  Rows and paths are synthetic (generator B): the chain
does the same work whatever it hashes.

  inputs   2^18 openings: hades252_wmmcs_inputs (with roots) against hades252_dmmcs_verify on the same buffers.  The same
           chain plus 160 B of stores per permutation.  Bar: at most 1.10 x the verification.
  witness  2^15 openings (about 8.5 x 10^5 records, about 26 GB of wires): hades252_wmmcs_witness against
           hades252_perm_witness_dev at the same record count and against the sum of its two stages timed alone.  Bar: at most
           1.05 x that sum; the spread of the runs is printed beside it.  The ratio to perm_witness is reported, not judged.
  single   one opening per call: the latency of hades252_wmmcs_witness and of hades252_wmmcs_inputs, 50 back-to-back calls.

--part all (the default) runs each part as a child process under a time limit of its own (`timeout -k 10 SECONDS`) and stops
at the first that fails; a part prints one line per measurement and a final JSON line with every single time."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PARTS = {"inputs": 240, "witness": 420, "single": 240}          # seconds each may take, library load and warm-up included
HEIGHTS, COLS, DEPTH, ARITY, PAD_MODE, OUT_IDX = (1 << 20, 1 << 16), (8, 4), 20, 2, 1, 1
WIRES = 972


def limbs(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)])


def alternating(torch, fns, reps):
    """One warm-up call of each, then `reps` rounds in which every function runs once, in turn; -> the times of each, in
    seconds, every one from an idle device to an idle device."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[i].append(time.perf_counter() - t0)
    return times


def ms(ts):
    return [round(t * 1e3, 4) for t in ts]


def run_part(part, args):
    import numpy as np
    import torch
    from hades252_amd import _lib, build, strategy as H
    build.build(verbose=False)
    lib = _lib.lib()
    assert torch.cuda.is_available(), "this tool measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    cap, tag, inject = limbs(1 << 64), limbs(3), limbs(31)
    lib.hades252_warm_up(1 << 20)
    hs, cs = np.array(HEIGHTS, dtype=np.uint64), np.array(COLS, dtype=np.uint64)

    def ptr(a):
        return ctypes.c_void_p(a.ctypes.data)

    P = int(lib.hades252_wmmcs_perms(ptr(hs), ptr(cs), 2, ARITY, PAD_MODE))
    assert P == 26
    nq = {"inputs": 1 << args.log2queries_inputs, "witness": 1 << args.log2queries_witness, "single": 1}[part]
    out = {"part": part, "device": torch.cuda.get_device_name(0), "reps": args.reps, "heights": list(HEIGHTS), "cols": list(COLS),
           "perms_per_opening": P, "queries": nq}
    d_rows = H.gen_b(nq * sum(COLS), dev, first_elem=1 << 28)
    d_paths = H.gen_b(nq * DEPTH, dev, first_elem=1 << 29)
    rng = np.random.default_rng(17)
    d_idx = torch.from_numpy(rng.integers(0, HEIGHTS[0], size=nq, dtype=np.int64)).to(dev)
    d_roots, d_roots_v = torch.zeros(nq * 4, dtype=torch.int64, device=dev), torch.zeros(nq * 4, dtype=torch.int64, device=dev)
    d_inputs = torch.empty(P * nq * 20, dtype=torch.int64, device=dev)
    front = (d_rows.data_ptr(), ptr(hs), ptr(cs), 2, d_idx.data_ptr(), d_paths.data_ptr(), nq, ARITY, cap, PAD_MODE, tag, inject, OUT_IDX)

    def verify():
        assert lib.hades252_dmmcs_verify(*front, d_roots_v.data_ptr(), None) == 0

    def inputs():
        assert lib.hades252_wmmcs_inputs(*front, d_inputs.data_ptr(), d_roots.data_ptr(), None) == 0

    if part == "inputs":
        t = alternating(torch, [inputs, verify], args.reps)
        same = bool(torch.equal(d_roots, d_roots_v))
        ratio = min(t[0]) / min(t[1])
        out.update({"wmmcs_inputs_ms": ms(t[0]), "dmmcs_verify_ms": ms(t[1]), "roots_equal": same, "ratio": ratio, "bar": 1.10,
                    "bar_met": bool(ratio <= 1.10), "input_bytes": P * nq * 160, "store_gb_per_s": P * nq * 160 / min(t[0]) / 1e9})
        print("inputs  %d openings x %d permutations   hades252_wmmcs_inputs %9.3f ms  %7.1f M perms/s  %6.1f GB/s of inputs   "
              "hades252_dmmcs_verify %9.3f ms  %7.1f M perms/s   ratio %.3f x   bar (<= 1.10 x) %s   roots equal: %s"
              % (nq, P, min(t[0]) * 1e3, nq * P / min(t[0]) / 1e6, out["store_gb_per_s"], min(t[1]) * 1e3, nq * P / min(t[1]) / 1e6, ratio,
                 "met" if out["bar_met"] else "MISSED", same), flush=True)
    else:
        d_wires = torch.empty(WIRES * P * nq * 4, dtype=torch.int64, device=dev)

        def witness():
            assert lib.hades252_wmmcs_witness(*front, d_inputs.data_ptr(), d_wires.data_ptr(), d_roots.data_ptr(), None) == 0

        def perm_witness():
            _lib.check(lib.hades252_perm_witness_dev(d_inputs.data_ptr(), d_wires.data_ptr(), P * nq, None), "perm_witness_dev")

        if part == "witness":
            t = alternating(torch, [witness, perm_witness, inputs], args.reps)
            verify()
            torch.cuda.synchronize()
            same = bool(torch.equal(d_roots, d_roots_v))
            best = [min(x) for x in t]
            stages = best[1] + best[2]
            spread = max(max(x) - min(x) for x in t)
            out.update({"records": P * nq, "wire_bytes": WIRES * P * nq * 32, "wmmcs_witness_ms": ms(t[0]), "perm_witness_ms": ms(t[1]),
                        "wmmcs_inputs_ms": ms(t[2]), "sum_of_stages_ms": round(stages * 1e3, 4), "spread_ms": round(spread * 1e3, 4),
                        "ratio_to_sum": best[0] / stages, "bar": 1.05, "bar_met": bool(best[0] <= 1.05 * stages),
                        "ratio_to_perm_witness": best[0] / best[1], "roots_equal": same})
            print("witness %d openings x %d = %d records, %.1f GB of wires   hades252_wmmcs_witness %9.3f ms  %7.1f M perms/s   "
                  "hades252_perm_witness_dev %9.3f ms  %7.1f M perms/s   inputs stage alone %9.3f ms" %
                  (nq, P, P * nq, WIRES * P * nq * 32 / 1e9, best[0] * 1e3, P * nq / best[0] / 1e6, best[1] * 1e3, P * nq / best[1] / 1e6,
                   best[2] * 1e3), flush=True)
            print("witness   sum of the two stages %9.3f ms   the call / the sum %.3f x   bar (<= 1.05 x) %s   spread of the runs "
                  "%.3f ms   the call / perm_witness %.3f x   roots equal: %s"
                  % (stages * 1e3, best[0] / stages, "met" if out["bar_met"] else "MISSED", spread * 1e3, best[0] / best[1], same), flush=True)
        else:
            calls = 50
            each = {}
            for name, fn in (("wmmcs_witness", witness), ("wmmcs_inputs", inputs), ("dmmcs_verify", verify), ("perm_witness", perm_witness)):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                    torch.cuda.synchronize()
                each[name] = (time.perf_counter() - t0) / calls * 1e6
            out.update({"calls": calls, "us_per_call": each})
            print("single  one opening x %d permutations per call, %d back-to-back calls   hades252_wmmcs_witness %8.1f us   "
                  "hades252_wmmcs_inputs %8.1f us   hades252_dmmcs_verify %8.1f us   hades252_perm_witness_dev (%d records) %8.1f us"
                  % (P, calls, each["wmmcs_witness"], each["wmmcs_inputs"], each["dmmcs_verify"], P, each["perm_witness"]), flush=True)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2queries-inputs", type=int, default=18)
    ap.add_argument("--log2queries-witness", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--part", default="all", choices=["all"] + list(PARTS))
    args = ap.parse_args()
    if args.part != "all":
        return run_part(args.part, args)
    for part, seconds in PARTS.items():
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(args.reps),
               "--log2queries-inputs", str(args.log2queries_inputs), "--log2queries-witness", str(args.log2queries_witness)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                                                     # nothing more is started on the device after a failure
            print("part %s ended with status %d: stopping" % (part, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
