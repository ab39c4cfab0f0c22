"""Timing of the streaming matrix commitment (hades252_matstream_*, root only) against the one-shot hades252_matrix_commit on the
same planes -- in one process and one run, every buffer page-locked, the two alternating.

    python tools/time_matrix_stream.py [--narrow-log2rows 20] [--narrow-cols 4,16,64] [--wide-log2rows 16] [--wide-cols 1024]
                                       [--wide-calls 16] [--reps 5] [--arity 4] [--skip-wide]

Wall clock around the synchronous host calls, the best of --reps after one warm-up call of each:
  (a) narrow matrices (2^20 rows x 4 / 16 / 64 columns): open + one absorb + commit (digests = tree = NULL) + close against
      hades252_matrix_commit (digests = tree = NULL).  The one-shot call is code this feature does not touch.
  (b) the wide matrix (2^16 rows x 1 024 columns, 2 GiB): the same with one absorb call and with --wide-calls calls of
      equally many columns, against hades252_matrix_commit.  The roots of all three are compared.
  (c) references of the same run: hades252_perm_batch_dev on device memory at the permutation count of (b) (at most 2^23
      states at once; fewer are scaled and the line says so); the rate of a bare hipMemcpy2D of one tile of (b) from the
      same page-locked planes (through the HIP runtime this process has loaded; "not measured" if it cannot be found); and an
      absorb of three columns into a fresh stream, which permutes nothing: 2-D copies and additions alone.
Prints one line per measurement and a final JSON line.  Not measurable here: the absorb kernel alone on device memory (there
is no device-pointer form) and a host that is not a PyTorch process (hades252_amd/build.py, build_host_path_bench).
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def limbs(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)])


def pinned_u64(torch, np, n_u64):
    t = torch.empty(max(n_u64, 4), dtype=torch.int64).pin_memory()
    return t, t.numpy().view(np.uint64)[:n_u64]


def best_alternating(fns, reps):
    """One warm-up call of each, then `reps` rounds in which every function runs once, in turn: the best time of each."""
    for fn in fns:
        fn()
    best = [float("inf")] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            best[i] = min(best[i], time.perf_counter() - t0)
    return best


def loaded_hip_runtime():
    """The HIP runtime this process has mapped (the one libhades252 and PyTorch call), or None."""
    try:
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        return None
    for path in paths:
        try:
            return ctypes.CDLL(path)
        except OSError:
            continue
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--narrow-log2rows", type=int, default=20)
    ap.add_argument("--narrow-cols", default="4,16,64")
    ap.add_argument("--wide-log2rows", type=int, default=16)
    ap.add_argument("--wide-cols", type=int, default=1024)
    ap.add_argument("--wide-calls", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--arity", type=int, default=4)
    ap.add_argument("--skip-wide", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from hades252_amd import _lib, build, strategy as H
    build.build(verbose=False)
    lib = _lib.lib()
    assert torch.cuda.is_available(), "this tool measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    arity, cap, tag = args.arity, limbs(1 << 64), limbs(15)
    narrow_rows, narrow_cols = 1 << args.narrow_log2rows, [int(v) for v in args.narrow_cols.split(",")]
    wide_rows, wide_cols = 1 << args.wide_log2rows, args.wide_cols
    assert wide_cols % args.wide_calls == 0
    scalars = max(narrow_rows * max(narrow_cols), 0 if args.skip_wide else wide_rows * wide_cols)
    keep, planes_all = pinned_u64(torch, np, scalars * 4)
    piece = 1 << 24                                                    # generator B on the device, 512 MiB at a time
    for first in range(0, scalars, piece):
        n = min(piece, scalars - first)
        keep[first * 4:(first + n) * 4].copy_(H.gen_b(n, dev, first_elem=first).view(-1))
    torch.cuda.synchronize()
    lib.hades252_warm_up(1 << 20)
    out = {"device": torch.cuda.get_device_name(0), "arity": arity, "reps": args.reps, "pad_mode": 1,
           "chunk_rows_env": os.environ.get("HADES252_TEST_MATRIX_CHUNK_ROWS"),
           "chunk_cols_env": os.environ.get("HADES252_TEST_MATRIX_CHUNK_COLS"), "narrow": {}, "wide": None, "references": {}}

    def one_shot(pp, n_rows, n_cols, root):
        def run():
            rc = lib.hades252_matrix_commit(pp, n_rows, n_cols, n_rows, cap, 1, arity, tag, 1, None, None, None,
                                            ctypes.c_void_p(root.ctypes.data))
            assert rc == 0, rc
        return run

    def streamed(base, n_rows, n_cols, calls, root, finish=True):
        per = n_cols // calls

        def run():
            h = ctypes.c_void_p()
            rc = lib.hades252_matstream_open(ctypes.byref(h), n_rows, cap)
            assert rc == 0, rc
            try:
                for c in range(calls):
                    rc = lib.hades252_matstream_absorb(h, ctypes.c_void_p(base + c * per * n_rows * 32), per, n_rows)
                    assert rc == 0, rc
                if finish:
                    rc = lib.hades252_matstream_commit(h, 1, arity, tag, 1, None, None, None, ctypes.c_void_p(root.ctypes.data))
                    assert rc == 0, rc
            finally:
                lib.hades252_matstream_close(h)
        return run

    base = planes_all.ctypes.data
    # ---- (a) narrow ----
    for n_cols in narrow_cols:
        r1, r2 = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        t_one, t_str = best_alternating([one_shot(ctypes.c_void_p(base), narrow_rows, n_cols, r1),
                                         streamed(base, narrow_rows, n_cols, 1, r2)], args.reps)
        assert r1.tobytes() == r2.tobytes(), "the two routes disagree on the root"
        n_perms = narrow_rows * lib.hades252_sponge_blocks(n_cols, 1) + lib.hades252_merkle_tree_bytes(narrow_rows, arity) // 32
        out["narrow"][str(n_cols)] = {"n_rows": narrow_rows, "matrix_mib": n_cols * narrow_rows * 32 / 2 ** 20, "perms": n_perms,
                                      "matrix_commit_ms": t_one * 1e3, "stream_ms": t_str * 1e3, "stream_over_one_shot": t_str / t_one,
                                      "root": r1.tobytes().hex()}
        print("(a) 2^%d rows x %-4d  hades252_matrix_commit %9.3f ms   stream (1 absorb) %9.3f ms   stream / one-shot = %.3f"
              % (args.narrow_log2rows, n_cols, t_one * 1e3, t_str * 1e3, t_str / t_one), flush=True)
    # ---- (c) a group that permutes nothing: 2-D copies and additions alone ----
    t_add, = best_alternating([streamed(base, narrow_rows, 3, 1, None, finish=False)], args.reps)
    out["references"]["absorb_3_cols_no_permutation"] = {"n_rows": narrow_rows, "ms": t_add * 1e3,
                                                         "gb_per_s_in": 3 * narrow_rows * 32 / t_add / 1e9}
    print("(c) 2^%d rows x 3, open + absorb + close (no permutation)     %9.3f ms   %6.2f GB/s in"
          % (args.narrow_log2rows, t_add * 1e3, 3 * narrow_rows * 32 / t_add / 1e9), flush=True)
    if not args.skip_wide:
        # ---- (b) wide ----
        r1, r2, r3 = (np.zeros(4, dtype=np.uint64) for _ in range(3))
        t_one, t_s1, t_sn = best_alternating([one_shot(ctypes.c_void_p(base), wide_rows, wide_cols, r1),
                                              streamed(base, wide_rows, wide_cols, 1, r2),
                                              streamed(base, wide_rows, wide_cols, args.wide_calls, r3)], args.reps)
        assert r1.tobytes() == r2.tobytes() == r3.tobytes(), "the routes disagree on the root"
        blocks = lib.hades252_sponge_blocks(wide_cols, 1)
        n_perms = wide_rows * blocks + lib.hades252_merkle_tree_bytes(wide_rows, arity) // 32
        gib = wide_cols * wide_rows * 32 / 2 ** 30
        out["wide"] = {"n_rows": wide_rows, "n_cols": wide_cols, "matrix_gib": gib, "perms": n_perms, "blocks_per_row": blocks,
                       "matrix_commit_ms": t_one * 1e3, "stream_one_call_ms": t_s1 * 1e3, "stream_calls": args.wide_calls,
                       "stream_many_calls_ms": t_sn * 1e3, "speedup_one_call": t_one / t_s1, "speedup_many_calls": t_one / t_sn,
                       "stream_one_call_gb_per_s_in": gib * 2 ** 30 / t_s1 / 1e9, "bar_2x_met": bool(t_one / max(t_s1, t_sn) >= 2.0),
                       "root": r1.tobytes().hex()}
        print("(b) 2^%d rows x %d (%.2f GiB)  hades252_matrix_commit %9.3f ms" % (args.wide_log2rows, wide_cols, gib, t_one * 1e3))
        print("(b)   stream, 1 absorb call      %9.3f ms   %6.2f GB/s in   %.2f x faster" % (t_s1 * 1e3, gib * 2 ** 30 / t_s1 / 1e9, t_one / t_s1))
        print("(b)   stream, %2d absorb calls    %9.3f ms   %6.2f GB/s in   %.2f x faster"
              % (args.wide_calls, t_sn * 1e3, gib * 2 ** 30 / t_sn / 1e9, t_one / t_sn), flush=True)
        # ---- (c) the permutations alone, on device memory ----
        n_ref = min(n_perms, 1 << 23)
        states = H.gen_b(n_ref * 5, dev)
        torch.cuda.synchronize()

        def perms():
            rc = lib.hades252_perm_batch_dev(ctypes.c_void_p(states.data_ptr()), n_ref, None)
            assert rc == 0, rc
            torch.cuda.synchronize()

        t_p, = best_alternating([perms], args.reps)
        out["references"]["perm_batch_dev"] = {"states": n_ref, "ms": t_p * 1e3, "perms_per_s": n_ref / t_p,
                                               "ms_at_wide_perms": t_p * n_perms / n_ref * 1e3}
        print("(c) hades252_perm_batch_dev, %d states%s %9.3f ms   %7.2f M perms/s" % (
            n_ref, "" if n_ref == n_perms else " (of %d: scaled %.3f ms)" % (n_perms, t_p * n_perms / n_ref * 1e3), t_p * 1e3,
            n_ref / t_p / 1e6), flush=True)
        del states
        # ---- (c) a bare 2-D copy of one tile of (b) ----
        hip = loaded_hip_runtime()
        tile_cols = max(1, min(wide_cols, (128 << 20) // (32 * wide_rows)))
        if hip is not None and hasattr(hip, "hipMemcpy2D"):
            hip.hipMemcpy2D.restype = ctypes.c_int
            hip.hipMemcpy2D.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.c_size_t, ctypes.c_int]
            dst = torch.empty(tile_cols * wide_rows * 4, dtype=torch.int64, device=dev)

            def copy2d():                                               # hipMemcpyHostToDevice = 1; synchronous
                rc = hip.hipMemcpy2D(ctypes.c_void_p(dst.data_ptr()), wide_rows * 32, ctypes.c_void_p(base), wide_rows * 32,
                                     wide_rows * 32, tile_cols, 1)
                assert rc == 0, rc

            t_c, = best_alternating([copy2d], args.reps)
            nbytes = tile_cols * wide_rows * 32
            out["references"]["memcpy2d_tile"] = {"cols": tile_cols, "mib": nbytes / 2 ** 20, "ms": t_c * 1e3, "gb_per_s": nbytes / t_c / 1e9,
                                                  "ms_for_the_wide_matrix": t_c * wide_cols / tile_cols * 1e3}
            print("(c) hipMemcpy2D of one tile (%d columns, %d MiB)            %9.3f ms   %6.2f GB/s   (the whole matrix: %.1f ms)"
                  % (tile_cols, nbytes >> 20, t_c * 1e3, nbytes / t_c / 1e9, t_c * wide_cols / tile_cols * 1e3), flush=True)
        else:
            out["references"]["memcpy2d_tile"] = "not measured"
            print("(c) hipMemcpy2D of one tile: not measured (the loaded HIP runtime was not found)", flush=True)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
