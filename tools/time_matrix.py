"""Timing of the matrix commitment (hades252_matrix_commit, root only) against what a caller had to do before it existed: the
numpy transpose of the column-major matrix, then hades252_sponge_hash + hades252_merkle_root on the result -- in one
process and one run, every buffer page-locked.

    python tools/time_matrix.py [--log2rows 20] [--cols 4,16,64] [--reps 3] [--arity 4]
    python tools/time_matrix.py --ab [--log2rows 20] [--cols 16,64] [--targets-mib 4,8,16,32,64,128]

Per column count it measures, wall clock around the synchronous host calls (median of --reps after one warm-up call):
  (a) hades252_matrix_commit with digests = tree = NULL;
  (b) the transpose (numpy, into a page-locked row-major buffer), reported on its own, and then hades252_sponge_hash into a
      page-locked digest buffer + hades252_merkle_root of it;
  and hades252_perm_batch (160 bytes each way per permutation: the link-bound reference) on as many states as the
  commitment runs permutations, or as many as the row-major buffer holds if that is fewer (then the time is scaled and
  the line says so).
The roots of (a) and (b) are compared.  Prints one line per measurement and a final JSON line.

--ab: the A/B behind kMatrixTargetBytes (host_matrix.hpp).  The chunk size is read once per process, so every setting is a
child process with HADES252_TEST_MATRIX_CHUNK_ROWS = target / (32 * n_cols); the children run one after the other and the
sweep stops at the first one that fails.  Not measurable here: the kernel alone on device memory (there is no
device-pointer form) and a host that is not a PyTorch process (PyTorch's bundled runtime overlaps copies worse than the
system's: hades252_amd/build.py, build_host_path_bench).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def wall(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def limbs(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)])


def pinned_u64(torch, np, n_u64):
    t = torch.empty(max(n_u64, 4), dtype=torch.int64).pin_memory()
    return t, t.numpy().view(np.uint64)[:n_u64]


def measure(args, cols_list, quick):
    """quick: (a) only (the A/B children)."""
    import numpy as np
    import torch
    from hades252_amd import _lib, build, strategy as H
    build.build(verbose=False)
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    n_rows, arity = 1 << args.log2rows, args.arity
    cap, tag = limbs(1 << 64), limbs(15)
    max_cols = max(cols_list)
    keep_p, planes_all = pinned_u64(torch, np, max_cols * n_rows * 4)
    gen = H.gen_b(max_cols * n_rows, dev)
    keep_p.copy_(gen.view(-1))
    del gen
    if not quick:
        keep_r, rowmajor_all = pinned_u64(torch, np, max_cols * n_rows * 4)
        keep_d, digests = pinned_u64(torch, np, n_rows * 4)
    lib.hades252_warm_up(1 << 20)
    out = {"device": torch.cuda.get_device_name(0), "n_rows": n_rows, "arity": arity, "reps": args.reps, "pad_mode": 1,
           "chunk_rows_env": os.environ.get("HADES252_TEST_MATRIX_CHUNK_ROWS"), "cols": {}}
    for n_cols in cols_list:
        planes = planes_all[:n_cols * n_rows * 4].reshape(n_cols, n_rows, 4)
        root_a, root_b = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        pp = ctypes.c_void_p(planes.ctypes.data)

        def commit():
            rc = lib.hades252_matrix_commit(pp, n_rows, n_cols, n_rows, cap, 1, arity, tag, 1, None, None, None,
                                            ctypes.c_void_p(root_a.ctypes.data))
            assert rc == 0, rc

        t_a = wall(commit, args.reps)
        blocks = lib.hades252_sponge_blocks(n_cols, 1)
        n_perms = n_rows * blocks + lib.hades252_merkle_tree_bytes(n_rows, arity) // 32
        rec = {"matrix_mib": n_cols * n_rows * 32 / 2 ** 20, "perms": n_perms, "commit_ms": t_a * 1e3,
               "commit_perms_per_s": n_perms / t_a, "commit_in_gb_per_s": n_cols * n_rows * 32 / t_a / 1e9}
        print("cols=%-3d (a) hades252_matrix_commit, root only        %9.3f ms  %7.2f M perms/s  %6.2f GB/s in"
              % (n_cols, t_a * 1e3, n_perms / t_a / 1e6, rec["commit_in_gb_per_s"]), flush=True)
        if not quick:
            rowmajor = rowmajor_all[:n_cols * n_rows * 4].reshape(n_rows, n_cols, 4)
            t_t = wall(lambda: np.copyto(rowmajor, planes.transpose(1, 0, 2)), max(1, min(args.reps, 2)))
            rp, dp = ctypes.c_void_p(rowmajor.ctypes.data), ctypes.c_void_p(digests.ctypes.data)

            def two_calls():
                rc = lib.hades252_sponge_hash(rp, n_rows, n_cols, cap, 1, dp)
                assert rc == 0, rc
                rc = lib.hades252_merkle_root(dp, n_rows, arity, tag, 1, None, ctypes.c_void_p(root_b.ctypes.data))
                assert rc == 0, rc

            t_b = wall(two_calls, args.reps)
            assert root_a.tobytes() == root_b.tobytes(), "the two routes disagree on the root"
            fit = rowmajor_all.size // 20
            n_ref = min(n_perms, fit)
            t_p = wall(lambda: lib.hades252_perm_batch(ctypes.c_void_p(rowmajor_all.ctypes.data), n_ref), args.reps)
            rec.update({"transpose_ms": t_t * 1e3, "sponge_hash_plus_merkle_root_ms": t_b * 1e3, "commit_over_two_calls": t_a / t_b,
                        "perm_batch_states": n_ref, "perm_batch_ms": t_p * 1e3, "perm_batch_perms_per_s": n_ref / t_p,
                        "perm_batch_ms_at_commit_perms": t_p * n_perms / n_ref * 1e3, "root": root_a.tobytes().hex()})
            print("cols=%-3d (b) numpy transpose                           %9.3f ms" % (n_cols, t_t * 1e3))
            print("cols=%-3d (b) hades252_sponge_hash + hades252_merkle_root %7.3f ms  (a)/(b) = %.3f" % (n_cols, t_b * 1e3, t_a / t_b))
            print("cols=%-3d     hades252_perm_batch, %d states%s %9.3f ms  %7.2f M perms/s" % (
                n_cols, n_ref, "" if n_ref == n_perms else " (of %d: scaled %.3f ms)" % (n_perms, t_p * n_perms / n_ref * 1e3),
                t_p * 1e3, n_ref / t_p / 1e6), flush=True)
        out["cols"][str(n_cols)] = rec
    print(json.dumps(out), flush=True)
    return 0


def ab(args, cols_list):
    results = []
    for n_cols in cols_list:
        for mib in [int(v) for v in args.targets_mib.split(",")]:
            k = max(256, (mib << 20) // (32 * n_cols) // 256 * 256)
            env = dict(os.environ, HADES252_TEST_MATRIX_CHUNK_ROWS=str(k))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2rows", str(args.log2rows), "--cols", str(n_cols),
                   "--reps", str(args.reps), "--arity", str(args.arity)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print("target %d MiB, cols %d: child exited %d -- stopping the sweep\n%s" % (mib, n_cols, r.returncode, r.stderr[-2000:]))
                return 1
            rec = json.loads(r.stdout.strip().splitlines()[-1])["cols"][str(n_cols)]
            results.append({"cols": n_cols, "target_mib": mib, "chunk_rows": k, "commit_ms": rec["commit_ms"],
                            "perms_per_s": rec["commit_perms_per_s"]})
            print("cols=%-3d target %4d MiB  K = %8d rows  %9.3f ms  %7.2f M perms/s" % (n_cols, mib, k, rec["commit_ms"],
                                                                                      rec["commit_perms_per_s"] / 1e6), flush=True)
    print(json.dumps({"n_rows": 1 << args.log2rows, "reps": args.reps, "ab": results}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2rows", type=int, default=20)
    ap.add_argument("--cols", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--arity", type=int, default=4)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--targets-mib", default="4,8,16,32,64,128")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    cols_list = [int(v) for v in (args.cols or ("16,64" if args.ab else "4,16,64")).split(",")]
    if args.ab:
        return ab(args, cols_list)
    return measure(args, cols_list, quick=args.child)


if __name__ == "__main__":
    sys.exit(main())
