"""Timing of the inverse permutation (hades252_perm_inverse_batch) against the forward host call (hades252_perm_batch) on the
same page-locked buffer, in one run.

    python tools/time_perm_inverse.py [--reps 3] [--log2n 20]

Measures, wall clock around the synchronous host calls (each uploads, runs its kernel and downloads):
  * hades252_perm_batch on 2^log2n generator-B states;
  * hades252_perm_inverse_batch on the same buffer (it then holds the states again: the round trip is checked);
  * hades252_fifth_root_batch on 5 * 2^log2n scalars (the same bytes);
and, for orientation, k_perm_fast alone on device memory (device events, tools/timing.py).  Prints one line per measurement
and a final JSON line with the rates, the measured inverse / forward ratio and the counted one,
(99 * products per root + 67 * 25) / 1972.
"""
import argparse
import ctypes
import json
import os
import statistics
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from hades252_amd import _derive, _lib, build, strategy as H
    from timing import timed
    build.build(verbose=False)
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    n = 1 << args.log2n
    states = H.gen_b(5 * n, dev)
    host = torch.empty((n, 5, 4), dtype=torch.int64).pin_memory()
    host.copy_(states.view(n, 5, 4))
    buf = host.numpy().view(np.uint64)
    before = buf.copy()
    ptr = ctypes.c_void_p(buf.ctypes.data)

    def call(fn, count):
        rc = fn(ptr, count)
        assert rc == 0, rc

    # the same number of calls each way (reps + 1), so the buffer ends where it started
    t_fwd = wall(lambda: call(lib.hades252_perm_batch, n), args.reps)
    t_inv = wall(lambda: call(lib.hades252_perm_inverse_batch, n), args.reps)
    assert (buf == before).all(), "perm_inverse(perm(x)) != x"
    t_root = wall(lambda: call(lib.hades252_fifth_root_batch, 5 * n), args.reps)
    fast = H.ScalarStrategy(_lib.KERNEL_FAST)
    t_k = timed(lambda: fast.perm(states), args.reps)

    products = _derive.inverse_chain_products()
    counted = (99 * products + 67 * 25) / 1972
    out = {"device": torch.cuda.get_device_name(0), "n": n, "products_per_root": products, "counted_ratio": counted,
           "perm_batch": {"ms": t_fwd * 1e3, "perms_per_s": n / t_fwd},
           "perm_inverse_batch": {"ms": t_inv * 1e3, "perms_per_s": n / t_inv},
           "fifth_root_batch": {"scalars": 5 * n, "ms": t_root * 1e3, "roots_per_s": 5 * n / t_root},
           "k_perm_fast_device": {"ms": t_k * 1e3, "perms_per_s": n / t_k},
           "measured_ratio": t_inv / t_fwd, "ratio_to_kernel": t_inv / t_k}
    print("hades252_perm_batch          n=2^%d %9.3f ms %8.2f M perms/s (host call, page-locked buffer)"
          % (args.log2n, t_fwd * 1e3, n / t_fwd / 1e6))
    print("hades252_perm_inverse_batch  n=2^%d %9.3f ms %8.2f M perms/s (same buffer)" % (args.log2n, t_inv * 1e3, n / t_inv / 1e6))
    print("hades252_fifth_root_batch    n=5*2^%d %7.3f ms %8.2f M roots/s" % (args.log2n, t_root * 1e3, 5 * n / t_root / 1e6))
    print("k_perm_fast (device memory)  n=2^%d %9.3f ms %8.2f M perms/s" % (args.log2n, t_k * 1e3, n / t_k / 1e6))
    print("inverse / forward host call: %.2f measured; counted (99 * %d + 67 * 25) / 1972 = %.2f; inverse host call / "
          "k_perm_fast: %.2f" % (t_inv / t_fwd, products, counted, t_inv / t_k))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
