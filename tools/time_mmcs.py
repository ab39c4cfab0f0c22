"""Timing of the mixed-height matrix commitments (hades252_mmcs_*) against what the library offered before them -- in one
process and one run, every host buffer page-locked, the routes alternating.

    python tools/time_mmcs.py [--log2rows 20,16,12] [--cols 64] [--log2queries 18] [--reps 5] [--skip-commit] [--skip-verify]

  (a) commit: groups of 2^20, 2^16 and 2^12 rows x 64 columns, arity 2, root only.  hades252_mmcs_new + one absorb per group +
      commit + free against three hades252_matstream_open + absorb + commit + close, one per matrix (three roots, three
      trees).  Wall clock around the synchronous host calls, the best of --reps after one warm-up of each.  Beside them: the
      commit alone on a handle that has absorbed everything (it is non-destructive, so it repeats), and each short group's
      row hashing alone (open + absorb + close of its stream).  Bar: mmcs <= 1.10 x the three streams.
  (b) verify: 2^18 synthetic openings (generated rows, siblings and indices: nothing has to verify), arity 2, heights 2^20 /
      2^16, columns 8 / 4, pad_mode 1: 26 permutations per query.  hades252_mmcs_verify from page-locked host memory (wall
      clock, best of --reps) as a permutation rate n S / t, against hades252_perm_batch_dev on n S states in device memory
      (tools/timing.py: HIP events).  Bar: 0.9.  Beside them: the existing device calls composed on device memory (a sponge
      per group, a path verification per tree segment, a level at arity 2 for the injection), and a bare host-to-device copy
      of the same rows and paths.
Prints one line per measurement and a final JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2rows", default="20,16,12")
    ap.add_argument("--cols", type=int, default=64)
    ap.add_argument("--log2queries", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-commit", action="store_true")
    ap.add_argument("--skip-verify", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import timing
    from hades252_amd import _lib, build, strategy as H
    build.build(verbose=False)
    lib = _lib.lib()
    assert torch.cuda.is_available(), "this tool measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    arity, cap, tag, inject = 2, limbs(1 << 64), limbs(3), limbs(31)
    lib.hades252_warm_up(1 << 20)
    out = {"device": torch.cuda.get_device_name(0), "arity": arity, "reps": args.reps, "pad_mode": 1,
           "chunk_queries_env": os.environ.get("HADES252_TEST_MMCS_CHUNK_QUERIES"), "commit": None, "verify": None}

    def pinned(n_scalars, first):
        """n_scalars generator-B scalars in page-locked host memory: (the tensor that owns them, their address)."""
        t = torch.empty(n_scalars * 4, dtype=torch.int64).pin_memory()
        piece = 1 << 24
        for at in range(0, n_scalars, piece):
            n = min(piece, n_scalars - at)
            t[at * 4:(at + n) * 4].copy_(H.gen_b(n, dev, first_elem=first + at).view(-1))
        torch.cuda.synchronize()
        return t, t.data_ptr()

    if not args.skip_commit:
        heights, n_cols = [1 << int(v) for v in args.log2rows.split(",")], args.cols
        planes = [pinned(h * n_cols, 1 << (24 + i)) for i, h in enumerate(heights)]
        roots = np.zeros((1 + len(heights), 4), dtype=np.uint64)

        def rp(i):
            return ctypes.c_void_p(roots[i].ctypes.data)

        def absorbed():
            h = ctypes.c_void_p()
            assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0
            for (_, ptr), n_rows in zip(planes, heights):
                assert lib.hades252_mmcs_absorb(h, ctypes.c_void_p(ptr), n_rows, n_cols, n_rows) == 0
            return h

        def mmcs():
            h = absorbed()
            try:
                assert lib.hades252_mmcs_commit(h, 1, arity, tag, inject, 1, None, rp(0)) == 0
            finally:
                lib.hades252_mmcs_free(h)

        def stream(i, finish=True):
            def run():
                h = ctypes.c_void_p()
                assert lib.hades252_matstream_open(ctypes.byref(h), heights[i], cap) == 0
                try:
                    assert lib.hades252_matstream_absorb(h, ctypes.c_void_p(planes[i][1]), n_cols, heights[i]) == 0
                    if finish:
                        assert lib.hades252_matstream_commit(h, 1, arity, tag, 1, None, None, None, rp(1 + i)) == 0
                finally:
                    lib.hades252_matstream_close(h)
            return run

        def streams():
            for i in range(len(heights)):
                stream(i)()

        t_mmcs, t_streams = best_alternating([mmcs, streams], args.reps)
        each = best_alternating([stream(i) for i in range(len(heights))], args.reps)
        hashing = best_alternating([stream(i, finish=False) for i in range(len(heights))], args.reps)
        live = absorbed()
        try:
            t_commit, = best_alternating([lambda: lib.hades252_mmcs_commit(live, 1, arity, tag, inject, 1, None, rp(0))], args.reps)
        finally:
            lib.hades252_mmcs_free(live)
        depth = heights[0].bit_length() - 1
        out["commit"] = {"heights": heights, "n_cols": n_cols, "mmcs_ms": t_mmcs * 1e3, "three_streams_ms": t_streams * 1e3,
                         "mmcs_over_streams": t_mmcs / t_streams, "bar_1_10_met": bool(t_mmcs <= 1.10 * t_streams),
                         "stream_each_ms": [t * 1e3 for t in each], "row_hashing_each_ms": [t * 1e3 for t in hashing],
                         "mmcs_commit_alone_ms": t_commit * 1e3, "level_launches": depth + len(heights) - 1,
                         "root": roots[0].tobytes().hex()}
        print("(a) %s rows x %d   mmcs (new, %d absorbs, commit, free) %9.3f ms   %d streams (open, absorb, commit, close) %9.3f ms   "
              "mmcs / streams = %.3f   bar 1.10 %s" % (heights, n_cols, len(heights), t_mmcs * 1e3, len(heights), t_streams * 1e3,
                                                      t_mmcs / t_streams, "met" if t_mmcs <= 1.10 * t_streams else "MISSED"))
        for i, n_rows in enumerate(heights):
            print("(a)   %8d rows: stream alone %9.3f ms   its row hashing alone (open, absorb, close) %9.3f ms"
                  % (n_rows, each[i] * 1e3, hashing[i] * 1e3))
        print("(a)   mmcs commit alone (finishes, levels, injections, build; root only) %9.3f ms" % (t_commit * 1e3), flush=True)
        del planes

    if not args.skip_verify:
        nq, heights, cols = 1 << args.log2queries, (1 << 20, 1 << 16), (8, 4)
        depth, S = 20, int(lib.hades252_sponge_blocks(8, 1) + lib.hades252_sponge_blocks(4, 1)) + 20 + 1
        rows_t, rows_p = pinned(nq * sum(cols), 1 << 28)
        paths_t, paths_p = pinned(nq * depth, 1 << 29)
        rng = np.random.default_rng(14)
        idx_t = torch.from_numpy(rng.integers(0, heights[0], size=nq, dtype=np.int64)).pin_memory()
        roots_t = torch.zeros(nq * 4, dtype=torch.int64).pin_memory()
        hs, cs = np.array(heights, dtype=np.uint64), np.array(cols, dtype=np.uint64)

        def verify():
            rc = lib.hades252_mmcs_verify(ctypes.c_void_p(rows_p), ctypes.c_void_p(hs.ctypes.data), ctypes.c_void_p(cs.ctypes.data), 2,
                                          ctypes.c_void_p(idx_t.data_ptr()), ctypes.c_void_p(paths_p), nq, arity, cap, 1, tag, inject, 1,
                                          ctypes.c_void_p(roots_t.data_ptr()))
            assert rc == 0, rc

        d_rows, d_paths = torch.empty_like(rows_t, device=dev), torch.empty_like(paths_t, device=dev)

        def copies():
            d_rows.copy_(rows_t, non_blocking=True)
            d_paths.copy_(paths_t, non_blocking=True)
            torch.cuda.synchronize()

        t_verify, t_copy = best_alternating([verify, copies], args.reps)
        # the same chain through the existing device calls, on device memory
        d_idx = idx_t.to(dev)
        r0 = d_rows.view(nq, sum(cols), 4)[:, :cols[0]].contiguous().view(-1)
        r1 = d_rows.view(nq, sum(cols), 4)[:, cols[0]:].contiguous().view(-1)
        p = d_paths.view(nq, depth, 1, 4)
        seg0, seg1, up = p[:, :4].contiguous(), p[:, 4:].contiguous(), d_idx >> 4

        def composed():
            node = H.sponge_hash(r0, cols[0], 1 << 64, 1)
            node = H.merkle_verify(node, d_idx, seg0, arity, 3)
            leaf = H.sponge_hash(r1, cols[1], 1 << 64, 1)
            node = H.merkle_level(torch.stack([node.view(nq, 4), leaf.view(nq, 4)], dim=1).contiguous().view(-1), 2, 31)
            return H.merkle_verify(node, up, seg1, arity, 3)

        got = composed()
        torch.cuda.synchronize()
        same = bool((got.cpu().view(-1) == roots_t).all())
        t_comp = timing.timed(composed, args.reps)
        del d_rows, d_paths, r0, r1, p, seg0, seg1
        states = H.gen_b(nq * S * 5, dev)
        t_perm = timing.timed(lambda: _lib.check(lib.hades252_perm_batch_dev(states.data_ptr(), nq * S, None), "perm_batch_dev"), args.reps)
        ratio = t_perm / t_verify
        out["verify"] = {"queries": nq, "heights": list(heights), "cols": list(cols), "perms_per_query": S, "mmcs_verify_ms": t_verify * 1e3,
                         "perm_equivalent_per_s": nq * S / t_verify, "perm_batch_dev_ms": t_perm * 1e3,
                         "perm_batch_dev_per_s": nq * S / t_perm, "ratio": ratio, "bar_0_9_met": bool(ratio >= 0.9),
                         "composed_dev_calls_ms": t_comp * 1e3, "composed_equals_fused": same,
                         "bare_copy_ms": t_copy * 1e3, "bare_copy_gb_per_s": (rows_t.numel() + paths_t.numel()) * 8 / t_copy / 1e9}
        print("(b) %d queries x %d permutations   hades252_mmcs_verify (host memory) %9.3f ms  %7.1f M perms/s   "
              "hades252_perm_batch_dev (device memory) %9.3f ms  %7.1f M perms/s   ratio %.3f   bar 0.9 %s"
              % (nq, S, t_verify * 1e3, nq * S / t_verify / 1e6, t_perm * 1e3, nq * S / t_perm / 1e6, ratio, "met" if ratio >= 0.9 else "MISSED"))
        print("(b)   the existing device calls composed, device memory %9.3f ms (roots equal: %s)   a bare copy of rows and paths %9.3f ms  "
              "%6.2f GB/s" % (t_comp * 1e3, same, t_copy * 1e3, out["verify"]["bare_copy_gb_per_s"]), flush=True)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
