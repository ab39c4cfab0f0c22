"""The timer of the time_*.py tools, and the reference measurement and line format of the three witness tools
(time_witness_chains.py, time_cipher_witness.py, time_safe_witness.py).  Imported by them, not run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from hades252_amd import strategy as H, _lib  # noqa: E402

WIRES = 972


def timed(fn, reps):
    fn()                                               # warm-up (code object, first touch of the buffers)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps / 1e3            # seconds per call


def witness_line(label, n_perms, t, width=18):
    return "%-*s perms=%-8d %9.3f ms  %7.1f M perms/s" % (width, label, n_perms, t * 1e3, n_perms / t / 1e6)


def perm_witness_rate(rows, n_perms, wires, reps, width=18):
    """hades252_perm_witness_dev on n_perms generated states into `wires`: appends its row, prints its line, returns
    permutations/s (what the chain witnesses at the same count are held against)."""
    lib, dev = _lib.lib(), wires.device
    states = H.gen_b(5 * n_perms, dev, first_elem=3)
    t = timed(lambda: _lib.check(lib.hades252_perm_witness_dev(states.data_ptr(), wires.data_ptr(), n_perms,
                                                               torch.cuda.current_stream(dev).cuda_stream),
                                 "perm_witness"), reps)
    rows.append({"op": "perm_witness", "perms": n_perms, "ms": t * 1e3, "perms_per_s": n_perms / t})
    print(witness_line("perm_witness", n_perms, t, width), flush=True)
    return n_perms / t


def report(rows, op, n_perms, t, ref_rate, extra=""):
    """One chain witness beside the perm_witness rate at the same count: appends its row, prints its line."""
    row = {"op": op, "perms": n_perms, "ms": t * 1e3, "perms_per_s": n_perms / t, "vs_perm_witness": n_perms / t / ref_rate}
    rows.append(row)
    print("%s  (%.3f x perm_witness)%s" % (witness_line(op, n_perms, t), row["vs_perm_witness"], extra), flush=True)
