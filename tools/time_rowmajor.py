"""Timing of the row-major forms of the mixed-height commitments (hades252_rmmcs_absorb_ex, hades252_rmmcs_open_ex,
hades252_rmmcs_absorb_rows) against the column-major calls they stand beside -- in one process and one run, the routes
alternating, every time a host clock around work that ends in a device synchronise.

    python tools/time_rowmajor.py [--log2rows 20,16,12] [--cols 64,63] [--log2queries 18] [--reps 5] [--host-shapes 20x64,16x1024]
                                  [--skip-absorb] [--skip-open] [--skip-host]

  (a) device absorb: groups of 2^20, 2^16 and 2^12 rows x 64 columns in device memory.  One three-part
      hades252_rmmcs_absorb_ex all row-major against one three-part hades252_dmmcs_absorb on the transposed twins, what a
      row-major caller could do before (three permute(1, 0, 2).contiguous() on the device plus that call) and
      hades252_perm_batch_dev at the same permutation count.  Bars: row-major <= 1.10 x column-major, and row-major <
      transpose + column-major.  The same again with 63 columns (rows that are no multiple of 128 bytes, an open block that
      stays open), no bar.
  (b) open: 2^18 queries on the same shape after a commit: hades252_rmmcs_open_ex all row-major, hades252_dmmcs_open on the
      twins, hades252_merkle_open_dev alone and a plain Tensor.copy_ of the rows' bytes.  Bar: the row-major call is not
      slower than the column-major one by more than the larger spread of the two.
  (c) host form, page-locked memory, 2^20 x 64 and 2^16 x 1024: hades252_rmmcs_absorb_rows, hades252_mmcs_absorb on the
      transposed twin, the numpy transpose alone (into memory that is already mapped).  Bar: row-major < transpose +
      column-major.  Where row-major / column-major is above 1.10 the pitched 2-D copy of one tile is timed by itself.
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
from time_dmmcs import alternating, limbs, ms  # noqa: E402

ROWS, COLS = 1, 0                                   # HADES252_LAYOUT_ROWS, HADES252_LAYOUT_COLS


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def loaded_hip_runtime():
    """The HIP runtime this process already runs on (the one torch loaded), for the one call the library does not export: a
    pitched copy by itself.  -> a ctypes handle, or None."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
        return ctypes.CDLL(sorted(paths)[0]) if paths else None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2rows", default="20,16,12")
    ap.add_argument("--cols", default="64,63")
    ap.add_argument("--log2queries", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-shapes", default="20x64,16x1024")
    ap.add_argument("--skip-absorb", action="store_true")
    ap.add_argument("--skip-open", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
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
    heights, nq = [1 << int(v) for v in args.log2rows.split(",")], 1 << args.log2queries
    widths = [int(v) for v in args.cols.split(",")]
    out = {"device": torch.cuda.get_device_name(0), "arity": arity, "reps": args.reps, "heights": heights, "absorb": [], "open": None,
           "host": []}

    def new_handle():
        h = ctypes.c_void_p()
        assert lib.hades252_mmcs_new(ctypes.byref(h), cap) == 0
        return h

    def free(*handles):
        for h in handles:
            torch.cuda.synchronize()
            lib.hades252_mmcs_free(h)

    def row_tables(mats):                                              # row-major device tensors [n_rows, n_cols, 4]
        return [np.array(v, dtype=np.uint64) for v in ([t.data_ptr() for t in mats], [t.shape[0] for t in mats],
                                                       [t.shape[1] for t in mats], [t.shape[1] for t in mats])] + \
               [np.full(len(mats), ROWS, dtype=np.uint32)]

    def plane_tables(planes):                                          # column-major device tensors [n_cols, n_rows, 4]
        return [np.array(v, dtype=np.uint64) for v in ([t.data_ptr() for t in planes], [t.shape[1] for t in planes],
                                                       [t.shape[0] for t in planes], [t.shape[1] for t in planes])]

    def xabsorb(h, mats):
        pl, r, c, s, lay = row_tables(mats)
        assert lib.hades252_rmmcs_absorb_ex(h, ptr(pl), ptr(r), ptr(c), ptr(s), ptr(lay), len(mats), None) == 0

    def dabsorb(h, planes):
        pl, r, c, s = plane_tables(planes)
        assert lib.hades252_dmmcs_absorb(h, ptr(pl), ptr(r), ptr(c), ptr(s), len(planes), None) == 0

    def matrices(n_cols):
        mats = [H.gen_b(h * n_cols, dev, first_elem=1 << (24 + i)).view(h, n_cols, 4) for i, h in enumerate(heights)]
        twins = [m.permute(1, 0, 2).contiguous() for m in mats]
        torch.cuda.synchronize()
        return mats, twins

    # ---- (a) device absorb ----------------------------------------------------------------------------------------------
    for n_cols in ([] if args.skip_absorb else widths):
        mats, twins = matrices(n_cols)
        n_perms = sum(heights) * (n_cols // 4)
        states = H.gen_b(n_perms * 5, dev)
        hr, hc, ht = new_handle(), new_handle(), new_handle()          # the three handles see the same history

        def rows_call():
            xabsorb(hr, mats)

        def cols_call():
            dabsorb(hc, twins)

        def transpose_then_cols():
            dabsorb(ht, [m.permute(1, 0, 2).contiguous() for m in mats])

        def perm():
            _lib.check(lib.hades252_perm_batch_dev(states.data_ptr(), n_perms, None), "perm_batch_dev")

        try:
            t = alternating(torch, [rows_call, cols_call, transpose_then_cols, perm], args.reps)
            roots = []
            for h in (hr, hc, ht):                                     # the three routes absorbed the same columns
                root = np.zeros(4, dtype=np.uint64)
                assert lib.hades252_mmcs_commit(h, 1, arity, tag, inject, 1, None, ptr(root)) == 0
                roots.append(root.tobytes())
        finally:
            free(hr, hc, ht)
        best = [min(x) for x in t]
        rec = {"n_cols": n_cols, "perms": n_perms, "rows_ex_ms": ms(t[0]), "cols_dmmcs_ms": ms(t[1]), "transpose_plus_cols_ms": ms(t[2]),
               "perm_batch_dev_ms": ms(t[3]), "rows_over_cols": round(best[0] / best[1], 4), "roots_equal": len(set(roots)) == 1,
               "bar_1_10_met": bool(best[0] <= 1.10 * best[1]) if n_cols % 4 == 0 else None,
               "bar_below_transpose_met": bool(best[0] < best[2]) if n_cols % 4 == 0 else None}
        out["absorb"].append(rec)
        print("(a) %s rows x %d, %d permutations   all-ROWS _ex %9.3f ms   column-major twins %9.3f ms   ratio %.3f   transpose + "
              "column-major %9.3f ms   hades252_perm_batch_dev %9.3f ms   roots equal: %s"
              % (heights, n_cols, n_perms, best[0] * 1e3, best[1] * 1e3, best[0] / best[1], best[2] * 1e3, best[3] * 1e3, rec["roots_equal"]))
        if n_cols % 4 == 0:
            print("(a)   bar (rows <= 1.10 x cols) %s   bar (rows < transpose + cols) %s"
                  % ("met" if rec["bar_1_10_met"] else "MISSED", "met" if rec["bar_below_transpose_met"] else "MISSED"))
        sys.stdout.flush()
        del mats, twins, states

    # ---- (b) open -------------------------------------------------------------------------------------------------------
    if not args.skip_open:
        n_cols = widths[0]
        mats, twins = matrices(n_cols)
        depth = heights[0].bit_length() - 1
        h = new_handle()
        try:
            xabsorb(h, mats)
            torch.cuda.synchronize()
            root = np.zeros(4, dtype=np.uint64)
            assert lib.hades252_mmcs_commit(h, 1, arity, tag, inject, 1, None, ptr(root)) == 0
            rng = np.random.default_rng(16)
            d_idx = torch.from_numpy(rng.integers(0, heights[0], size=nq, dtype=np.int64)).to(dev)
            total = n_cols * len(heights)
            d_rows = torch.empty((nq, total, 4), dtype=torch.int64, device=dev)
            d_rows2 = torch.empty_like(d_rows)
            d_paths = torch.empty((nq, depth, 1, 4), dtype=torch.int64, device=dev)
            d_copy = torch.empty_like(d_rows)
            rt, ct = row_tables(mats), plane_tables(twins)
            tree, n_bytes, a = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
            assert lib.hades252_dmmcs_tree(h, ctypes.byref(tree), ctypes.byref(n_bytes), ctypes.byref(a)) == 0

            def rows_open():
                assert lib.hades252_rmmcs_open_ex(h, *[ptr(x) for x in rt], len(mats), d_idx.data_ptr(), nq, d_rows.data_ptr(),
                                                  d_paths.data_ptr(), None) == 0

            def cols_open():
                assert lib.hades252_dmmcs_open(h, *[ptr(x) for x in ct], len(twins), d_idx.data_ptr(), nq, d_rows2.data_ptr(),
                                               d_paths.data_ptr(), None) == 0

            def paths_only():
                _lib.check(lib.hades252_merkle_open_dev(tree.value, tree.value + heights[0] * 32, heights[0], arity, d_idx.data_ptr(), nq,
                                                        d_paths.data_ptr(), None), "merkle_open_dev")

            def copy():
                d_copy.copy_(d_rows)

            t = alternating(torch, [rows_open, cols_open, paths_only, copy], args.reps)
            same = bool(torch.equal(d_rows, d_rows2))
        finally:
            free(h)
        best = [min(x) for x in t]
        spread = max(max(x) - min(x) for x in t[:2])
        row_bytes = nq * total * 32
        g_rows, g_cols = max(best[0] - best[2], 1e-9), max(best[1] - best[2], 1e-9)   # the two launches run one after the other
        out["open"] = {"queries": nq, "n_cols": n_cols, "row_bytes": row_bytes, "rows_open_ex_ms": ms(t[0]), "cols_open_ms": ms(t[1]),
                       "paths_alone_ms": ms(t[2]), "device_copy_ms": ms(t[3]), "spread_ms": round(spread * 1e3, 4), "rows_equal": same,
                       "gather_rows_ms_by_difference": round(g_rows * 1e3, 4), "gather_cols_ms_by_difference": round(g_cols * 1e3, 4),
                       "gather_rows_gb_per_s": 2 * row_bytes / g_rows / 1e9, "gather_cols_gb_per_s": 2 * row_bytes / g_cols / 1e9,
                       "copy_gb_per_s": 2 * row_bytes / best[3] / 1e9, "gather_rows_over_copy": round(best[3] / g_rows, 4),
                       "bar_met": bool(best[0] <= best[1] + spread)}
        print("(b) %d queries x %d columns   all-ROWS open_ex %9.3f ms   column-major open %9.3f ms   spread %.3f ms   bar (rows <= cols "
              "+ spread) %s   rows equal: %s" % (nq, total, best[0] * 1e3, best[1] * 1e3, spread * 1e3,
                                                 "met" if out["open"]["bar_met"] else "MISSED", same))
        print("(b)   paths alone %9.3f ms   gather by difference: rows %9.3f ms %7.1f GB/s, cols %9.3f ms %7.1f GB/s (read + written)   "
              "Tensor.copy_ %9.3f ms %7.1f GB/s   row gather / copy %.2f x"
              % (best[2] * 1e3, g_rows * 1e3, out["open"]["gather_rows_gb_per_s"], g_cols * 1e3, out["open"]["gather_cols_gb_per_s"],
                 best[3] * 1e3, out["open"]["copy_gb_per_s"], best[3] / g_rows), flush=True)
        del mats, twins, d_rows, d_rows2, d_paths, d_copy

    # ---- (c) host form, page-locked memory --------------------------------------------------------------------------------
    for shape in ([] if args.skip_host else args.host_shapes.split(",")):
        n_rows, n_cols = 1 << int(shape.split("x")[0]), int(shape.split("x")[1])
        rows_t = H.gen_b(n_rows * n_cols, dev, first_elem=1 << 30).view(n_rows, n_cols, 4).cpu().pin_memory()
        twin_t = rows_t.permute(1, 0, 2).contiguous().pin_memory()
        rows_np, scratch = rows_t.numpy(), np.zeros((n_cols, n_rows, 4), dtype=np.int64)
        hr, hc = new_handle(), new_handle()

        def rows_call():
            assert lib.hades252_rmmcs_absorb_rows(hr, ctypes.c_void_p(rows_t.data_ptr()), n_rows, n_cols, n_cols) == 0

        def cols_call():
            assert lib.hades252_mmcs_absorb(hc, ctypes.c_void_p(twin_t.data_ptr()), n_rows, n_cols, n_rows) == 0

        def transpose():
            np.copyto(scratch, rows_np.transpose(1, 0, 2))

        try:
            t = alternating(torch, [rows_call, cols_call, transpose], args.reps)
            roots = []
            for h in (hr, hc):
                root = np.zeros(4, dtype=np.uint64)
                assert lib.hades252_mmcs_commit(h, 1, arity, tag, inject, 1, None, ptr(root)) == 0
                roots.append(root.tobytes())
        finally:
            free(hr, hc)
        best = [min(x) for x in t]
        rec = {"n_rows": n_rows, "n_cols": n_cols, "absorb_rows_ms": ms(t[0]), "absorb_cols_ms": ms(t[1]), "numpy_transpose_ms": ms(t[2]),
               "rows_over_cols": round(best[0] / best[1], 4), "roots_equal": len(set(roots)) == 1,
               "bar_met": bool(best[0] < best[1] + best[2]), "tile_copy": None}
        print("(c) %d rows x %d from page-locked memory   hades252_rmmcs_absorb_rows %9.3f ms   hades252_mmcs_absorb (twin) %9.3f ms   "
              "ratio %.3f   numpy transpose %9.3f ms   bar (rows < transpose + cols) %s   roots equal: %s"
              % (n_rows, n_cols, best[0] * 1e3, best[1] * 1e3, best[0] / best[1], best[2] * 1e3, "met" if rec["bar_met"] else "MISSED",
                 rec["roots_equal"]), flush=True)
        hip = loaded_hip_runtime() if best[0] > 1.10 * best[1] else None
        if hip is not None:                                            # one tile's copy by itself: pitched, then contiguous
            K = min(n_rows, 1 << 18)
            G = min(n_cols, (128 << 20) // (32 * K) // 4 * 4)
            d = torch.empty(K * G * 4, dtype=torch.int64, device=dev)
            src, H2D = ctypes.c_void_p(rows_t.data_ptr()), 1
            hip.hipMemcpy2D.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.c_size_t, ctypes.c_int]
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

            def pitched():
                assert hip.hipMemcpy2D(d.data_ptr(), G * 32, src, n_cols * 32, G * 32, K, H2D) == 0

            def contiguous():
                assert hip.hipMemcpy(d.data_ptr(), src, K * G * 32, H2D) == 0

            c = alternating(torch, [pitched, contiguous], args.reps)
            tiles = -(-n_rows // K) * -(-n_cols // G)
            rec["tile_copy"] = {"tile_rows": K, "tile_cols": G, "tiles": tiles, "pitched_ms": ms(c[0]), "contiguous_ms": ms(c[1]),
                                "all_tiles_pitched_ms": round(min(c[0]) * tiles * 1e3, 4)}
            print("(c)   one tile of %d rows x %d columns (%d tiles): pitched 2-D copy %9.3f ms  %6.1f GB/s   contiguous copy of the same "
                  "bytes %9.3f ms  %6.1f GB/s   all tiles pitched %9.3f ms against the call's %9.3f ms"
                  % (K, G, tiles, min(c[0]) * 1e3, K * G * 32 / min(c[0]) / 1e9, min(c[1]) * 1e3, K * G * 32 / min(c[1]) / 1e9,
                     min(c[0]) * tiles * 1e3, best[0] * 1e3), flush=True)
            del d
        out["host"].append(rec)
        del rows_t, twin_t, rows_np, scratch
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
