"""Device-side timing of the cipher witnesses (hades252_cipher_{encrypt,decrypt}_witness_dev) against
hades252_perm_witness_dev at the same permutation count, in one process.

    python tools/time_cipher_witness.py [--reps 3]

Shapes: perm_witness on 2^20 states, then both cipher witnesses at 2^19 messages x M = 2 (S = 2: 2^20 permutations);
perm_witness on 3 x 2^18 states and both witnesses at 2^18 messages x M = 5 (S = 3); one M = 2 message per call
(latency).  Every shape is warmed up, then timed over `reps` back-to-back calls between two device events.  Prints one line
per shape -- permutations/s and the ratio to perm_witness at the same count -- and a final JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from hades252_amd import strategy as H, _lib  # noqa: E402
from timing import WIRES, perm_witness_rate, report, timed  # noqa: E402

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    dom = H._tag_arr(H.CIPHER_DOMAIN)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": []}

    for n, m in ((1 << 19, 2), (1 << 18, 5)):
        S = H.cipher_perms(m)
        n_perms = S * n
        wires = torch.empty((WIRES, n_perms, 4), dtype=torch.int64, device=dev)
        ref = perm_witness_rate(out["rows"], n_perms, wires, args.reps)
        msgs = H.gen_b(n * m, dev, first_elem=1 << 30)
        keys = H.gen_b(2 * n, dev, first_elem=1 << 31)
        nonces = H.gen_b(n, dev, first_elem=1 << 32)
        inputs = torch.empty((n_perms, 5, 4), dtype=torch.int64, device=dev)
        ciphers = torch.empty((n, m + 1, 4), dtype=torch.int64, device=dev)
        t = timed(lambda: _lib.check(lib.hades252_cipher_encrypt_witness_dev(
            msgs.data_ptr(), keys.data_ptr(), nonces.data_ptr(), n, m, dom, inputs.data_ptr(), wires.data_ptr(),
            ciphers.data_ptr(), stream()), "cipher_encrypt_witness"), args.reps)
        report(out["rows"], "encrypt_witness", n_perms, t, ref, "  n=%d M=%d" % (n, m))
        back = torch.empty((n, m, 4), dtype=torch.int64, device=dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        rej = torch.zeros(1, dtype=torch.int32, device=dev)
        t = timed(lambda: _lib.check(lib.hades252_cipher_decrypt_witness_dev(
            ciphers.data_ptr(), keys.data_ptr(), nonces.data_ptr(), n, m, dom, inputs.data_ptr(), wires.data_ptr(),
            back.data_ptr(), ok.data_ptr(), rej.data_ptr(), stream()), "cipher_decrypt_witness"), args.reps)
        report(out["rows"], "decrypt_witness", n_perms, t, ref, "  n=%d M=%d" % (n, m))
        assert int(rej.item()) == 0 and torch.equal(back, msgs.view(n, m, 4))
        del wires, msgs, keys, nonces, inputs, ciphers, back, ok, rej

    # ---- one M = 2 message per call ----
    m = 2
    msg, key, nonce = H.gen_b(m, dev, first_elem=5), H.gen_b(2, dev, first_elem=7), H.gen_b(1, dev, first_elem=9)
    inputs = torch.empty((2, 5, 4), dtype=torch.int64, device=dev)
    wires = torch.empty((WIRES, 2, 4), dtype=torch.int64, device=dev)
    reps1 = max(args.reps, 50)
    t1 = timed(lambda: _lib.check(lib.hades252_cipher_encrypt_witness_dev(
        msg.data_ptr(), key.data_ptr(), nonce.data_ptr(), 1, m, dom, inputs.data_ptr(), wires.data_ptr(), None, stream()),
        "cipher_encrypt_witness"), reps1)
    print("one message M=2 (2 permutations): %.1f us / call (%d back-to-back calls)" % (t1 * 1e6, reps1), flush=True)
    out["one_message_m2_us"] = {"us": t1 * 1e6, "calls": reps1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
