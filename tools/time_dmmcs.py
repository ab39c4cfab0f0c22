"""Timing of the device-resident mixed-height commitments (hades252_dmmcs_*) against the host forms of f14 and the bare
permutation -- in one process and one run, the routes alternating, every time a host clock around work that ends in a
device synchronise.

    python tools/time_dmmcs.py [--log2rows 20,16,12] [--cols 64] [--log2queries 18] [--reps 5] [--skip-absorb] [--skip-open]
                               [--skip-verify]

  (a) absorb: groups of 2^20, 2^16 and 2^12 rows x 64 columns in device memory.  One three-part hades252_dmmcs_absorb (ONE
      launch) against three one-part calls, the host-form hades252_mmcs_absorb of the same matrices from page-locked memory,
      and hades252_perm_batch_dev at the same permutation count.  Bar: grouped <= three singles + the spread of the runs.
      The order of the parts in the grid is the library's (shortest first); run the tool again with
      HADES252_TEST_DMMCS_TALL_FIRST=1 for the other order (the hook is read once per process).
  (b) open: 2^18 queries on the same shape after a commit: hades252_dmmcs_open (the row gather and the paths), the gather
      alone as bytes/s (rows written + rows read), and a plain device copy of the gather's output bytes.
  (c) verify: 2^18 synthetic openings, f14's shape (heights 2^20 / 2^16, columns 8 / 4, pad_mode 1): hades252_dmmcs_verify on
      device memory against hades252_mmcs_verify from page-locked host memory.
Prints one line per measurement and a final JSON line with every single time."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2rows", default="20,16,12")
    ap.add_argument("--cols", type=int, default=64)
    ap.add_argument("--log2queries", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-absorb", action="store_true")
    ap.add_argument("--skip-open", action="store_true")
    ap.add_argument("--skip-verify", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from hades252_amd import _lib, build, strategy as H
    build.build(verbose=False)
    lib = _lib.lib()
    assert torch.cuda.is_available(), "this tool measures on a GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    arity, cap, tag, inject = 2, limbs(1 << 64), limbs(3), limbs(31)
    lib.hades252_warm_up(1 << 20)
    heights, n_cols, nq = [1 << int(v) for v in args.log2rows.split(",")], args.cols, 1 << args.log2queries
    assert n_cols % 4 == 0, "whole blocks, so that every repetition of an absorb does the same work"
    out = {"device": torch.cuda.get_device_name(0), "arity": arity, "reps": args.reps, "heights": heights, "n_cols": n_cols,
           "tall_first_env": os.environ.get("HADES252_TEST_DMMCS_TALL_FIRST"), "absorb": None, "open": None, "verify": None}
    planes = [H.gen_b(h * n_cols, dev, first_elem=1 << (24 + i)).view(n_cols, h, 4) for i, h in enumerate(heights)]
    torch.cuda.synchronize()

    def tables(parts, rows):
        return [np.array(v, dtype=np.uint64) for v in ([t.data_ptr() for t in parts], rows, [t.shape[0] for t in parts],
                                                       [t.shape[1] for t in parts])]

    def ptr(a):
        return ctypes.c_void_p(a.ctypes.data)

    def new_handle():
        h = ctypes.c_void_p()
        assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0
        return h

    def dabsorb(h, parts, rows):
        pl, r, c, s = tables(parts, rows)
        assert lib.hades252_dmmcs_absorb(h, ptr(pl), ptr(r), ptr(c), ptr(s), len(parts), None) == 0

    if not args.skip_absorb:
        n_perms = sum(heights) * (n_cols // 4)
        pinned = [p.cpu().pin_memory() for p in planes]
        hg, hs, hh = new_handle(), new_handle(), new_handle()               # 64 columns a time: the open block stays empty
        states = H.gen_b(n_perms * 5, dev)

        def grouped():
            dabsorb(hg, planes, heights)

        def singles():
            for p, n in zip(planes, heights):
                dabsorb(hs, [p], [n])

        def host():
            for p, n in zip(pinned, heights):
                assert lib.hades252_mmcs_absorb(hh, ctypes.c_void_p(p.data_ptr()), n, n_cols, n) == 0

        def perm():
            _lib.check(lib.hades252_perm_batch_dev(states.data_ptr(), n_perms, None), "perm_batch_dev")

        try:
            t = alternating(torch, [grouped, singles, host, perm], args.reps)
            each = alternating(torch, [lambda p=p, n=n: dabsorb(hs, [p], [n]) for p, n in zip(planes, heights)], args.reps)
        finally:
            for h in (hg, hs, hh):
                torch.cuda.synchronize()
                lib.hades252_mmcs_free(h)
        best = [min(x) for x in t]
        spread = max(max(x) - min(x) for x in t[:2])
        out["absorb"] = {"perms": n_perms, "grouped_ms": ms(t[0]), "three_singles_ms": ms(t[1]), "host_form_ms": ms(t[2]),
                         "perm_batch_dev_ms": ms(t[3]), "single_each_ms": [ms(x) for x in each], "spread_ms": round(spread * 1e3, 4),
                         "bar_met": bool(best[0] <= best[1] + spread)}
        print("(a) %s rows x %d, %d permutations   grouped (one launch) %9.3f ms   three single calls %9.3f ms   spread of the runs "
              "%.3f ms   bar (grouped <= singles + spread) %s" % (heights, n_cols, n_perms, best[0] * 1e3, best[1] * 1e3, spread * 1e3,
                                                                  "met" if out["absorb"]["bar_met"] else "MISSED"))
        print("(a)   host-form absorb from page-locked memory %9.3f ms   hades252_perm_batch_dev %9.3f ms  %7.1f M perms/s   grouped "
              "%7.1f M perms/s" % (best[2] * 1e3, best[3] * 1e3, n_perms / best[3] / 1e6, n_perms / best[0] / 1e6))
        for n, x in zip(heights, each):
            print("(a)   %8d rows alone %9.3f ms" % (n, min(x) * 1e3))
        sys.stdout.flush()
        del pinned, states

    if not args.skip_open:
        depth = heights[0].bit_length() - 1
        h = new_handle()
        try:
            dabsorb(h, planes, heights)
            torch.cuda.synchronize()
            root = np.zeros(4, dtype=np.uint64)
            assert lib.hades252_mmcs_commit(h, 1, arity, tag, inject, 1, None, ptr(root)) == 0
            rng = np.random.default_rng(15)
            d_idx = torch.from_numpy(rng.integers(0, heights[0], size=nq, dtype=np.int64)).to(dev)
            total = n_cols * len(heights)
            d_rows = torch.empty((nq, total, 4), dtype=torch.int64, device=dev)
            d_paths = torch.empty((nq, depth, 1, 4), dtype=torch.int64, device=dev)
            d_copy = torch.empty_like(d_rows)
            pl, r, c, s = tables(planes, heights)

            def opened():
                assert lib.hades252_dmmcs_open(h, ptr(pl), ptr(r), ptr(c), ptr(s), len(planes), d_idx.data_ptr(), nq,
                                               d_rows.data_ptr(), d_paths.data_ptr(), None) == 0

            def paths_only():
                _lib.check(lib.hades252_merkle_open_dev(tree.value, tree.value + heights[0] * 32, heights[0], arity, d_idx.data_ptr(), nq,
                                                        d_paths.data_ptr(), None), "merkle_open_dev")

            def copy():
                d_copy.copy_(d_rows)

            tree, n_bytes, a = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
            assert lib.hades252_dmmcs_tree(h, ctypes.byref(tree), ctypes.byref(n_bytes), ctypes.byref(a)) == 0
            t = alternating(torch, [opened, paths_only, copy], args.reps)
        finally:
            torch.cuda.synchronize()
            lib.hades252_mmcs_free(h)
        row_bytes = nq * total * 32
        gather = max(min(t[0]) - min(t[1]), 1e-9)                          # the two launches run one after the other
        out["open"] = {"queries": nq, "row_bytes": row_bytes, "open_ms": ms(t[0]), "paths_alone_ms": ms(t[1]), "device_copy_ms": ms(t[2]),
                       "gather_ms_by_difference": round(gather * 1e3, 4), "gather_gb_per_s_read_plus_written": 2 * row_bytes / gather / 1e9,
                       "copy_gb_per_s_read_plus_written": 2 * row_bytes / min(t[2]) / 1e9}
        print("(b) %d queries x %d columns   hades252_dmmcs_open %9.3f ms   its paths alone %9.3f ms   the gather, by difference "
              "%9.3f ms  %7.1f GB/s (read + written)   a device copy of the rows %9.3f ms  %7.1f GB/s"
              % (nq, total, min(t[0]) * 1e3, min(t[1]) * 1e3, gather * 1e3, out["open"]["gather_gb_per_s_read_plus_written"],
                 min(t[2]) * 1e3, out["open"]["copy_gb_per_s_read_plus_written"]), flush=True)
        del d_rows, d_paths, d_copy

    if not args.skip_verify:
        vh, vc, depth = (1 << 20, 1 << 16), (8, 4), 20
        S = int(lib.hades252_sponge_blocks(8, 1) + lib.hades252_sponge_blocks(4, 1)) + depth + 1
        d_rows = H.gen_b(nq * sum(vc), dev, first_elem=1 << 28)
        d_paths = H.gen_b(nq * depth, dev, first_elem=1 << 29)
        rng = np.random.default_rng(14)
        idx_t = torch.from_numpy(rng.integers(0, vh[0], size=nq, dtype=np.int64)).pin_memory()
        d_idx, d_roots = idx_t.to(dev), torch.zeros(nq * 4, dtype=torch.int64, device=dev)
        rows_t, paths_t = d_rows.cpu().pin_memory(), d_paths.cpu().pin_memory()
        roots_t = torch.zeros(nq * 4, dtype=torch.int64).pin_memory()
        hs, cs = np.array(vh, dtype=np.uint64), np.array(vc, dtype=np.uint64)

        def on_device():
            assert lib.hades252_dmmcs_verify(d_rows.data_ptr(), ptr(hs), ptr(cs), 2, d_idx.data_ptr(), d_paths.data_ptr(), nq, arity, cap, 1,
                                             tag, inject, 1, d_roots.data_ptr(), None) == 0

        def from_host():
            assert lib.hades252_mmcs_verify(ctypes.c_void_p(rows_t.data_ptr()), ptr(hs), ptr(cs), 2, ctypes.c_void_p(idx_t.data_ptr()),
                                            ctypes.c_void_p(paths_t.data_ptr()), nq, arity, cap, 1, tag, inject, 1,
                                            ctypes.c_void_p(roots_t.data_ptr())) == 0

        t = alternating(torch, [on_device, from_host], args.reps)
        same = bool((d_roots.cpu() == roots_t).all())
        out["verify"] = {"queries": nq, "heights": list(vh), "cols": list(vc), "perms_per_query": S, "dmmcs_verify_ms": ms(t[0]),
                         "mmcs_verify_host_ms": ms(t[1]), "roots_equal": same, "perm_equivalent_per_s": nq * S / min(t[0])}
        print("(c) %d queries x %d permutations   hades252_dmmcs_verify (device memory) %9.3f ms  %7.1f M perms/s   hades252_mmcs_verify "
              "(page-locked host memory) %9.3f ms   roots equal: %s" % (nq, S, min(t[0]) * 1e3, nq * S / min(t[0]) / 1e6, min(t[1]) * 1e3, same),
              flush=True)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
