"""Device-side timing of the batched Poseidon cipher (hades252_cipher_*_dev) against k_perm_fast, in one process.

    python tools/time_cipher.py [--reps 5] [--log2n 24]

Shapes: k_perm_fast at 2^log2n states; encrypt and decrypt at n = 2^log2n messages with M = 2, 4, 8 (one message per lane,
k_cipher); one message at M = 2 per call (one message per wave, k_cipher_lanes).  Every shape is warmed up, then timed over
`reps` back-to-back calls between two device events.  Prints one line per shape -- messages/s and the perm-equivalent rate
n * (ceil(M / 4) + 1) / t -- and a final JSON line with the same numbers.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from hades252_amd import strategy as H, _lib  # noqa: E402
from timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=24)
    args = ap.parse_args()
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    n = 1 << args.log2n
    dom = H._tag_arr(H.CIPHER_DOMAIN)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "n": n, "reps": args.reps, "rows": []}

    states = H.gen_b(5 * n, dev)
    fast = H.ScalarStrategy(_lib.KERNEL_FAST)
    t = timed(lambda: fast.perm(states), args.reps)
    perm_rate = n / t
    print("k_perm_fast        n=%-9d %9.3f ms  %8.1f M perms/s" % (n, t * 1e3, perm_rate / 1e6), flush=True)
    out["k_perm_fast"] = {"ms": t * 1e3, "perms_per_s": perm_rate}
    del states

    for m in (2, 4, 8):
        perms = (m + 3) // 4 + 1
        msgs = H.gen_b(n * m, dev)
        keys = H.gen_b(2 * n, dev, first_elem=1 << 36)
        nonces = H.gen_b(n, dev, first_elem=1 << 37)
        ciphers = torch.empty((n, m + 1, 4), dtype=torch.int64, device=dev)
        back = torch.empty((n, m, 4), dtype=torch.int64, device=dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)

        def enc():
            _lib.check(lib.hades252_cipher_encrypt_dev(msgs.data_ptr(), keys.data_ptr(), nonces.data_ptr(), n, m, dom,
                                                       ciphers.data_ptr(), stream()), "encrypt")

        def dec():
            _lib.check(lib.hades252_cipher_decrypt_dev(ciphers.data_ptr(), keys.data_ptr(), nonces.data_ptr(), n, m, dom,
                                                       back.data_ptr(), ok.data_ptr(), None, stream()), "decrypt")
        for name, fn in (("encrypt", enc), ("decrypt", dec)):
            t = timed(fn, args.reps)
            row = {"op": name, "M": m, "n": n, "ms": t * 1e3, "msgs_per_s": n / t, "perm_equiv_per_s": n * perms / t,
                   "vs_k_perm_fast": n * perms / t / perm_rate}
            out["rows"].append(row)
            print("%-7s M=%d      n=%-9d %9.3f ms  %8.1f M msgs/s  %8.1f M perm-equiv/s  (%.3f x k_perm_fast)"
                  % (name, m, n, t * 1e3, row["msgs_per_s"] / 1e6, row["perm_equiv_per_s"] / 1e6, row["vs_k_perm_fast"]),
                  flush=True)
        assert bool((ok == 1).all()) and torch.equal(back.view(-1), msgs.view(-1)), "round trip failed"
        del msgs, keys, nonces, ciphers, back, ok

    # one message per call: the latency form
    m = 2
    msgs, keys, nonces = H.gen_b(m, dev), H.gen_b(2, dev, first_elem=9), H.gen_b(1, dev, first_elem=11)
    ciphers = torch.empty((1, m + 1, 4), dtype=torch.int64, device=dev)
    back = torch.empty((1, m, 4), dtype=torch.int64, device=dev)
    ok = torch.empty(1, dtype=torch.uint8, device=dev)
    reps1 = max(args.reps, 50)
    t_enc = timed(lambda: _lib.check(lib.hades252_cipher_encrypt_dev(msgs.data_ptr(), keys.data_ptr(), nonces.data_ptr(), 1, m,
                                                                     dom, ciphers.data_ptr(), stream()), "encrypt"), reps1)
    t_dec = timed(lambda: _lib.check(lib.hades252_cipher_decrypt_dev(ciphers.data_ptr(), keys.data_ptr(), nonces.data_ptr(), 1, m,
                                                                     dom, back.data_ptr(), ok.data_ptr(), None, stream()),
                                     "decrypt"), reps1)
    assert int(ok.item()) == 1 and torch.equal(back.view(-1), msgs.view(-1))
    print("one message M=2: encrypt %.1f us / call, decrypt %.1f us / call (%d back-to-back calls)"
          % (t_enc * 1e6, t_dec * 1e6, reps1), flush=True)
    out["one_message_m2_us"] = {"encrypt": t_enc * 1e6, "decrypt": t_dec * 1e6, "calls": reps1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
