"""Timing of the proof-of-work grinding (hades252_grind) against k_perm_fast, and the A/B of its launch window.

    python tools/time_grind.py [--reps 3] [--log2n 26] [--windows 20,22,24,0]

One child process per window size (the library reads HADES252_TEST_GRIND_WINDOW once; 0 = the built-in constant), each of
which measures, in one run:
  * k_perm_fast on 2^log2n states (device events, tools/timing.py);
  * throughput of the search: one job, target 0 (exactly max_nonces candidates run), max_nonces = 2^log2n; and 4096 jobs of
    2^(log2n - 12) candidates each -- wall clock around the host call (it uploads, launches, downloads and synchronises);
  * time to solution at target = p >> 20 and p >> 24, ten seeds each, with the nonce that was found;
  * latency of one call that hits at its first candidate (target = p).
The parent prints one line per measurement, the overhead of every time to solution over the ideal hit_nonce / throughput
(throughput = the best one-job rate of the run), its median per window, and a final JSON line with all of it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BITS = (20, 24)
N_SEEDS = 10


def seeds_of(np, values):
    """canonical integers [[v0 .. v4], ...] -> uint64 [n, 5, 4] Montgomery limbs"""
    rows = [[[(v * (1 << 256) % P >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in job] for job in values]
    return np.array(rows, dtype=np.uint64)


def wall(fn, reps):
    fn()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best.append(time.perf_counter() - t0)
    return statistics.median(best)


def child(args):
    import numpy as np
    import torch
    from hades252_amd import strategy as H, _lib
    from timing import timed
    dev = torch.device("cuda", 0)
    n = 1 << args.log2n
    out = {"window": os.environ.get("HADES252_TEST_GRIND_WINDOW", "built-in"), "device": torch.cuda.get_device_name(0), "n": n}
    states = H.gen_b(5 * n, dev)
    fast = H.ScalarStrategy(_lib.KERNEL_FAST)
    t = timed(lambda: fast.perm(states), args.reps)
    out["k_perm_fast"] = {"ms": t * 1e3, "perms_per_s": n / t}
    del states
    torch.cuda.empty_cache()

    one = seeds_of(np, [[1 << 64, 1, 2, 3, 4]])
    t = wall(lambda: H.grind(one, 4, 1, 0, max_nonces=n), args.reps)
    out["one_job"] = {"candidates": n, "ms": t * 1e3, "per_s": n / t}
    jobs = 4096
    many = seeds_of(np, [[1 << 64, j, 2, 3, 4] for j in range(jobs)])
    t = wall(lambda: H.grind(many, 4, 1, 0, max_nonces=n // jobs), args.reps)
    out["many_jobs"] = {"jobs": jobs, "candidates": n, "ms": t * 1e3, "per_s": n / t}

    out["solve"] = []
    for bits in BITS:
        for j in range(N_SEEDS):
            seed = seeds_of(np, [[1 << 64, 1000 + j, 2, 3, 4]])
            res = []

            def run():
                res[:] = H.grind(seed, 4, 1, P >> bits)

            t = wall(run, 3)
            assert bool(res[1][0])
            out["solve"].append({"bits": bits, "seed": j, "nonce": int(res[0][0]), "ms": t * 1e3})
    t = wall(lambda: H.grind(one, 4, 1, P, max_nonces=1), 200)
    out["first_candidate_us"] = t * 1e6
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--windows", default="20,22,24,0", help="log2 of the windows to try; 0 = the built-in constant")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for w in [int(x) for x in args.windows.split(",")]:
        env = dict(os.environ)
        env.pop("HADES252_TEST_GRIND_WINDOW", None)
        if w:
            env["HADES252_TEST_GRIND_WINDOW"] = str(1 << w)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--log2n",
                            str(args.log2n)], env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode != 0 or len(lines) != 1:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1
        runs.append(json.loads(lines[0][6:]))
    best = max(r["one_job"]["per_s"] for r in runs)
    for r in runs:
        fast = r["k_perm_fast"]["perms_per_s"]
        print("window %-9s k_perm_fast n=2^%d %8.3f ms %7.1f M perms/s | one job %8.3f ms %7.1f M/s (%.3f x) | 4096 jobs "
              "%8.3f ms %7.1f M/s (%.3f x) | first-candidate call %6.1f us"
              % (r["window"], args.log2n, r["k_perm_fast"]["ms"], fast / 1e6, r["one_job"]["ms"], r["one_job"]["per_s"] / 1e6,
                 r["one_job"]["per_s"] / fast, r["many_jobs"]["ms"], r["many_jobs"]["per_s"] / 1e6,
                 r["many_jobs"]["per_s"] / fast, r["first_candidate_us"]), flush=True)
    print("time to solution, overhead over the ideal (hit nonce + 1) / %.1f M candidates/s:" % (best / 1e6))
    for r in runs:
        r["median_overhead_ms"] = {}
        for bits in BITS:
            rows = [s for s in r["solve"] if s["bits"] == bits]
            for s in rows:
                s["ideal_ms"] = (s["nonce"] + 1) / best * 1e3
                s["overhead_ms"] = s["ms"] - s["ideal_ms"]
            med = statistics.median(s["overhead_ms"] for s in rows)
            rel = statistics.median(s["ms"] / s["ideal_ms"] for s in rows)
            r["median_overhead_ms"][str(bits)] = med
            print("window %-9s p >> %d  median overhead %7.3f ms  median time / ideal %6.3f   [%s]"
                  % (r["window"], bits, med, rel, " ".join("%d:%.2f/%.2f" % (s["nonce"], s["ms"], s["ideal_ms"]) for s in rows)))
    print(json.dumps({"best_one_job_per_s": best, "runs": runs}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
