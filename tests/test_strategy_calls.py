"""The calls hades252_amd/strategy.py makes into the library, pinned: every wrapper is run at its smallest telling shape with
``_lib.lib`` swapped for a recorder around the real library, and the symbol, the normalised arguments and the shape and dtype of
what the wrapper returns are compared with tests/golden/strategy_calls.json.  Pure size and shape queries (no data pointer, no
stream; hades252_safe_pattern with them) reach the library; every other symbol is recorded and answers OK: no kernel is
launched.  A bad call records the exception type it raises, and must raise it before any recorded call.

``host`` (CPU tier): the wrappers that take numpy arrays.  ``device`` (GPU tier): the wrappers that take CUDA tensors; real
tensors are needed for ``_dev_buffer``, the library never runs.  There the recorder also demands, at call time, that the
current device is the tensors' device and that the stream argument is that device's current stream.

The fixture is recorded from the strategy.py the refactor started from, never from the refactored one::

    python tests/test_strategy_calls.py --record        # host always, device when a GPU is visible
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "strategy_calls.json")
CAP, TAG = 1 << 64, 15
POINTERS = (ctypes.c_void_p, ctypes.c_char_p)


def _is_pointer(t) -> bool:
    return t in POINTERS or hasattr(t, "contents")                      # POINTER(x) instances have .contents


class Recorder:
    """Stands where ``_lib.lib()`` returns the library."""

    def __init__(self, real, signatures):
        self.real, self.signatures = real, signatures
        self.calls, self.names = [], {}
        self.torch, self.device, self.guard_failures = None, None, []

    def __getattr__(self, sym):
        argtypes = self.signatures[sym][1]
        if sym == "hades252_safe_pattern" or not any(_is_pointer(t) for t in argtypes):
            return getattr(self.real, sym)
        stream_at = max(i for i, t in enumerate(argtypes) if t is ctypes.c_void_p) if "_dev" in sym else -1

        def recorded(*args):
            assert len(args) == len(argtypes), (sym, len(args))
            if stream_at >= 0:
                self._guard(sym, args[stream_at])
            self.calls.append([sym] + ["stream" if i == stream_at else self._norm(a, argtypes[i]) for i, a in enumerate(args)])
            return 0

        return recorded

    def _guard(self, sym, stream):
        t = self.torch
        if t.cuda.current_device() != self.device.index:
            self.guard_failures.append("%s: current device %d, tensors on %d" % (sym, t.cuda.current_device(), self.device.index))
        if stream != t.cuda.current_stream(self.device).cuda_stream:
            self.guard_failures.append("%s: not the current stream of %s" % (sym, self.device))

    def _norm(self, a, argtype):
        if isinstance(a, ctypes.Array):
            return list(a)
        if type(a).__name__ == "CArgObject":
            return "ref"
        if _is_pointer(argtype):
            if isinstance(a, ctypes.c_void_p):
                a = a.value
            if a is None or a == 0:
                return None
            if type(a) is not int:
                return "type:" + type(a).__name__
            return self.names.get(a, "ptr")
        if a is None:
            return None
        return a if type(a) in (int, bool) else "type:" + type(a).__name__


class Ctx:
    """Names the inputs of one case, so that the recorder can tell them from what the wrapper allocates."""

    def __init__(self, rec, torch=None, device=None):
        self.rec, self.torch, self.device, self.keep = rec, torch, device, []

    def u64(self, name, *shape, dtype=np.uint64):
        a = (np.arange(int(np.prod(shape)), dtype=np.uint64) + 1).astype(dtype).reshape(shape)
        return self.named(name, a)

    def named(self, name, a):
        self.keep.append(a)
        self.rec.names[a.ctypes.data] = name
        return a

    def ten(self, name, *shape, values=None):
        t = self.torch
        x = (t.arange(int(np.prod(shape)), dtype=t.int64, device=self.device).reshape(shape) + 1 if values is None
             else t.tensor(values, dtype=t.int64, device=self.device))
        self.keep.append(x)
        if x.numel():
            self.rec.names[x.data_ptr()] = name
        return x


def describe(v):
    if v is None or type(v) in (int, bool, str):
        return v
    if isinstance(v, bytes):
        return v.hex()
    if isinstance(v, np.ndarray):
        return ["ndarray", list(v.shape), str(v.dtype)]
    if isinstance(v, (tuple, list)):
        return [describe(x) for x in v]
    if type(v).__module__.startswith("torch"):
        return ["tensor", list(v.shape), str(v.dtype)]
    return "type:" + type(v).__name__


# ---- host section -----------------------------------------------------------------------------------------------------------
PATTERN = [("absorb", 3), ("squeeze", 2)]


def _merkle_host(arity, n, with_pad):
    def case(H, c):
        pad = c.u64("pad", H.merkle_depth(n, arity), 4) if with_pad else None
        return H.merkle_root_host(c.u64("leaves", n, 4), arity, TAG, 2, pad)
    return case


def _commit_args(H, c, with_pad):
    return c.u64("pad", 3, 4) if with_pad else None


def _matrix_commit(want_digests, want_tree, with_pad):
    def case(H, c):
        return H.matrix_commit_host(c.u64("planes", 2, 6, 4), CAP, 2, TAG, 1, 2, _commit_args(H, c, with_pad), 5,
                                    want_digests, want_tree)
    return case


def _stream(H, c):
    ms = H.MatrixStream(5, CAP)
    c.keep.append(ms)
    return ms


def _opened(H, c):
    ms = _stream(H, c)
    c.rec.calls.clear()                          # the constructor's call is not the bad call's
    return ms


def _stream_commit(want_digests, want_tree, with_pad):
    def case(H, c):
        return _stream(H, c).commit(2, TAG, 1, 2, _commit_args(H, c, with_pad), want_digests, want_tree)
    return case


def _stream_with(H, c):
    with H.MatrixStream(5, CAP) as ms:
        ms.absorb(c.u64("planes", 2, 6, 4))
    return ms._h


def _closed(H):
    ms = H.MatrixStream.__new__(H.MatrixStream)
    ms._h, ms.n_rows = None, 5
    return ms


HOST_CASES = {
    "perm": lambda H, c: H.ScalarStrategy().perm(c.u64("data", 3, 5, 4)),
    "perm_multi": lambda H, c: H.perm_multi(c.u64("data", 3, 5, 4)),
    "perm_multi/virtual": lambda H, c: H.perm_multi(c.u64("data", 3, 5, 4), 2, True),
    "perm_inverse_rounds": lambda H, c: H.perm_inverse_rounds(c.u64("states", 3, 5, 4), 67, 3),
    "perm_inverse": lambda H, c: H.perm_inverse(c.u64("states", 3, 5, 4)),
    "fifth_root": lambda H, c: H.fifth_root(c.u64("scalars", 3, 4)),
    "merkle_root_multi": lambda H, c: H.merkle_root_multi(c.u64("leaves", 16, 4), 4, TAG),
    "merkle_root_multi/virtual": lambda H, c: H.merkle_root_multi(c.u64("leaves", 16, 4), 4, TAG, 2, 2, True),
    "sponge_hash_host": lambda H, c: H.sponge_hash_host(c.u64("msgs", 3, 5, 4), 3, 5, CAP, 1),
    "sponge_hash_host/empty": lambda H, c: H.sponge_hash_host(c.u64("msgs", 0, 4), 3, 0, CAP, 1),
    "sponge_hash_var_host": lambda H, c: H.sponge_hash_var_host(
        c.u64("scalars", 9, 4), c.named("offsets", np.array([0, 0, 4], dtype=np.uint64)),
        c.named("lengths", np.array([0, 4, 5], dtype=np.uint64)), CAP, 1),
    "cipher_encrypt_host": lambda H, c: H.cipher_encrypt_host(c.u64("msgs", 3, 5, 4), c.u64("keys", 3, 2, 4),
                                                               c.u64("nonces", 3, 4), 5),
    "cipher_decrypt_host": lambda H, c: H.cipher_decrypt_host(c.u64("ciphers", 3, 6, 4), c.u64("keys", 3, 2, 4),
                                                               c.u64("nonces", 3, 4), 5, 9),
    "safe_pattern": lambda H, c: H.safe_pattern(PATTERN),
    "safe_tag_input": lambda H, c: H.safe_tag_input([("absorb", 2), ("absorb", 1), ("squeeze", 1), ("squeeze", 1)], 7),
    "safe_hash_host": lambda H, c: H.safe_hash_host(c.u64("inputs", 3, 3, 4), PATTERN, TAG),
    "grind_target": lambda H, c: H.grind_target(4),
    "grind": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 1, 2, H.grind_target(4), 5, 100),
    "trace_scale_table": lambda H, c: H.trace_scale_table(),
    "host_register": lambda H, c: H.host_register(c.u64("arr", 3, 5, 4)),
    "host_unregister": lambda H, c: H.host_unregister(c.u64("arr", 3, 5, 4)),
    "host_is_pinned": lambda H, c: H.host_is_pinned(c.u64("arr", 3, 5, 4)),
    "matrix_row_digests_host": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 6, 4), CAP, 1, 5),
    "matrix_row_digests_host/all_rows": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 6, 4), CAP, 0),
    "matrix_open_host": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4), c.u64("digests", 5, 4), c.u64("tree", 6, 4), 2,
                                                        [0, 4], None, 5),
    "matrix_open_host/pad": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4), c.u64("digests", 5, 4), c.u64("tree", 6, 4),
                                                            2, [0, 4], c.u64("pad", 3, 4), 5),
    "matrix_verify_host": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 2, 4), [0, 4], c.u64("paths", 2, 3, 1, 4), 2, CAP, TAG,
                                                            1, 2),
    "MatrixStream": lambda H, c: _stream(H, c)._h.value,
    "MatrixStream.absorb": lambda H, c: _stream(H, c).absorb(c.u64("planes", 2, 6, 4)).n_rows,
    "MatrixStream.absorb/n_rows": lambda H, c: _stream(H, c).absorb(c.u64("planes", 2, 6, 4), 5).n_rows,
    "MatrixStream.absorb/no_columns": lambda H, c: _stream(H, c).absorb(c.u64("planes", 0, 6, 4)).n_rows,
    "MatrixStream.cols": lambda H, c: _stream(H, c).cols,
    "MatrixStream.digests": lambda H, c: _stream(H, c).digests(0),
    "MatrixStream.close": lambda H, c: [_stream(H, c).close(), c.keep[-1].close(), c.keep[-1]._h],
    "MatrixStream/with": _stream_with,
}
for _arity in (2, 3, 4):
    for _n in (9, 10):
        for _pad in (False, True):
            HOST_CASES["merkle_root_host/arity%d/%d%s" % (_arity, _n, "/pad" if _pad else "")] = _merkle_host(_arity, _n, _pad)
for _d in (False, True):
    for _t in (False, True):
        for _pad in (False, True):
            _k = "/digests%d/tree%d%s" % (_d, _t, "/pad" if _pad else "")
            HOST_CASES["matrix_commit_host" + _k] = _matrix_commit(_d, _t, _pad)
            HOST_CASES["MatrixStream.commit" + _k] = _stream_commit(_d, _t, _pad)

I64 = np.int64
_strided = lambda *shape: np.zeros(shape + (2,), dtype=np.uint64)[..., 0]           # right dtype, not contiguous
HOST_ERRORS = {
    "perm/dtype": lambda H, c: H.ScalarStrategy().perm(c.u64("data", 3, 5, 4, dtype=I64)),
    "perm/contiguous": lambda H, c: H.ScalarStrategy().perm(_strided(3, 5, 4)),
    "perm/size": lambda H, c: H.ScalarStrategy().perm(c.u64("data", 19)),
    "perm/list": lambda H, c: H.ScalarStrategy().perm([0] * 20),
    "perm_multi/dtype": lambda H, c: H.perm_multi(c.u64("data", 3, 5, 4, dtype=I64)),
    "perm_multi/contiguous": lambda H, c: H.perm_multi(_strided(3, 5, 4)),
    "perm_multi/size": lambda H, c: H.perm_multi(c.u64("data", 19)),
    "perm_inverse_rounds/dtype": lambda H, c: H.perm_inverse_rounds(c.u64("states", 3, 5, 4, dtype=I64), 67, 0),
    "perm_inverse_rounds/list": lambda H, c: H.perm_inverse_rounds([[[0] * 4] * 5], 67, 0),
    "perm_inverse_rounds/contiguous": lambda H, c: H.perm_inverse_rounds(_strided(3, 5, 4), 67, 0),
    "perm_inverse_rounds/shape": lambda H, c: H.perm_inverse_rounds(c.u64("states", 3, 20), 67, 0),
    "perm_inverse_rounds/bool": lambda H, c: H.perm_inverse_rounds(c.u64("states", 3, 5, 4), 67, False),
    "perm_inverse_rounds/float": lambda H, c: H.perm_inverse_rounds(c.u64("states", 3, 5, 4), 67.0, 0),
    "perm_inverse_rounds/past_the_end": lambda H, c: H.perm_inverse_rounds(c.u64("states", 3, 5, 4), 68, 0),
    "perm_inverse_rounds/order": lambda H, c: H.perm_inverse_rounds(c.u64("states", 3, 5, 4), 3, 4),
    "perm_inverse/dtype": lambda H, c: H.perm_inverse(c.u64("states", 3, 5, 4, dtype=I64)),
    "perm_inverse/shape": lambda H, c: H.perm_inverse(c.u64("states", 3, 4, 5)),
    "fifth_root/dtype": lambda H, c: H.fifth_root(c.u64("scalars", 3, 4, dtype=I64)),
    "fifth_root/shape": lambda H, c: H.fifth_root(c.u64("scalars", 12)),
    "merkle_root_host/dtype": lambda H, c: H.merkle_root_host(c.u64("leaves", 9, 4, dtype=I64), 2, TAG),
    "merkle_root_host/list": lambda H, c: H.merkle_root_host([[0] * 4] * 9, 2, TAG),
    "merkle_root_host/contiguous": lambda H, c: H.merkle_root_host(_strided(9, 4), 2, TAG),
    "merkle_root_host/size": lambda H, c: H.merkle_root_host(c.u64("leaves", 9, 3), 2, TAG),
    "merkle_root_host/one_leaf": lambda H, c: H.merkle_root_host(c.u64("leaves", 1, 4), 2, TAG),
    "merkle_root_host/arity": lambda H, c: H.merkle_root_host(c.u64("leaves", 9, 4), 5, TAG),
    "merkle_root_host/pad_dtype": lambda H, c: H.merkle_root_host(c.u64("leaves", 9, 4), 2, TAG, 1, c.u64("pad", 4, 4, dtype=I64)),
    "merkle_root_host/pad_size": lambda H, c: H.merkle_root_host(c.u64("leaves", 9, 4), 2, TAG, 1, c.u64("pad", 3, 4)),
    "merkle_root_multi/dtype": lambda H, c: H.merkle_root_multi(c.u64("leaves", 16, 4, dtype=I64), 4, TAG),
    "sponge_hash_host/dtype": lambda H, c: H.sponge_hash_host(c.u64("msgs", 3, 5, 4, dtype=I64), 3, 5, CAP),
    "sponge_hash_host/size": lambda H, c: H.sponge_hash_host(c.u64("msgs", 3, 5, 4), 3, 4, CAP),
    "sponge_hash_var_host/dtype": lambda H, c: H.sponge_hash_var_host(c.u64("scalars", 9, 4), c.u64("offsets", 3, dtype=I64),
                                                                      c.u64("lengths", 3), CAP),
    "sponge_hash_var_host/pool": lambda H, c: H.sponge_hash_var_host(c.u64("scalars", 9, 3), c.u64("offsets", 3), c.u64("lengths", 3),
                                                                     CAP),
    "sponge_hash_var_host/index": lambda H, c: H.sponge_hash_var_host(c.u64("scalars", 9, 4), c.u64("offsets", 3), c.u64("lengths", 2),
                                                                      CAP),
    "safe_pattern/squeeze_first": lambda H, c: H.safe_pattern([("squeeze", 2), ("absorb", 1)]),
    "safe_pattern/kind": lambda H, c: H.safe_pattern([("read", 2)]),
    "safe_pattern/length": lambda H, c: H.safe_pattern([("absorb", 2.0)]),
    "safe_tag_input/invalid": lambda H, c: H.safe_tag_input([("squeeze", 2)], 7),
    "safe_hash_host/pattern": lambda H, c: H.safe_hash_host(c.u64("inputs", 3, 3, 4), [("squeeze", 2)], TAG),
    "safe_hash_host/kind": lambda H, c: H.safe_hash_host(c.u64("inputs", 3, 3, 4), [("read", 2)], TAG),
    "safe_hash_host/dtype": lambda H, c: H.safe_hash_host(c.u64("inputs", 3, 3, 4, dtype=I64), PATTERN, TAG),
    "safe_hash_host/limbs": lambda H, c: H.safe_hash_host(c.u64("inputs", 3, 3, 3), PATTERN, TAG),
    "safe_hash_host/whole_inputs": lambda H, c: H.safe_hash_host(c.u64("inputs", 4, 4), PATTERN, TAG),
    "grind_target/negative": lambda H, c: H.grind_target(-1),
    "grind/dtype": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4, dtype=I64), 1, 2, 5),
    "grind/list": lambda H, c: H.grind([[[0] * 4] * 5], 1, 2, 5),
    "grind/contiguous": lambda H, c: H.grind(_strided(2, 5, 4), 1, 2, 5),
    "grind/shape": lambda H, c: H.grind(c.u64("seeds", 2, 20), 1, 2, 5),
    "grind/word": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 5, 2, 5),
    "grind/out_idx": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 1, -1, 5),
    "grind/target_negative": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 1, 2, -1),
    "grind/target_wide": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 1, 2, 1 << 256),
    "grind/target_float": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 1, 2, 5.0),
    "grind/nonce_range": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 1, 2, 5, 1 << 63, (1 << 63) + 1),
    "grind/nonce_negative": lambda H, c: H.grind(c.u64("seeds", 2, 5, 4), 1, 2, 5, -1),
    "grind/jobs": lambda H, c: H.grind(np.zeros((65536, 5, 4), dtype=np.uint64), 1, 2, 5),
    "matrix_row_digests_host/dtype": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 6, 4, dtype=I64), CAP),
    "matrix_row_digests_host/contiguous": lambda H, c: H.matrix_row_digests_host(_strided(2, 6, 4), CAP),
    "matrix_row_digests_host/ndim": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 24), CAP),
    "matrix_row_digests_host/limbs": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 6, 5), CAP),
    "matrix_row_digests_host/no_columns": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 0, 6, 4), CAP),
    "matrix_row_digests_host/too_many_columns": lambda H, c: H.matrix_row_digests_host(np.zeros((4097, 1, 4), dtype=np.uint64), CAP),
    "matrix_row_digests_host/n_rows": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 6, 4), CAP, 1, 7),
    "matrix_row_digests_host/n_rows_bool": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 6, 4), CAP, 1, True),
    "matrix_row_digests_host/pad_mode": lambda H, c: H.matrix_row_digests_host(c.u64("planes", 2, 6, 4), CAP, 2),
    "matrix_commit_host/dtype": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 6, 4, dtype=I64), CAP, 2, TAG),
    "matrix_commit_host/ndim": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 24), CAP, 2, TAG),
    "matrix_commit_host/arity": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 6, 4), CAP, 5, TAG),
    "matrix_commit_host/one_row": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 6, 4), CAP, 2, TAG, n_rows=1),
    "matrix_commit_host/pad_mode": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 6, 4), CAP, 2, TAG, 2),
    "matrix_commit_host/out_idx": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 6, 4), CAP, 2, TAG, 1, 5),
    "matrix_commit_host/pad_dtype": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 6, 4), CAP, 2, TAG, 1, 1,
                                                                      c.u64("pad", 3, 4, dtype=I64)),
    "matrix_commit_host/pad_size": lambda H, c: H.matrix_commit_host(c.u64("planes", 2, 6, 4), CAP, 2, TAG, 1, 1, c.u64("pad", 2, 4)),
    "matrix_open_host/dtype": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4, dtype=I64), c.u64("digests", 6, 4),
                                                              c.u64("tree", 6, 4), 2, [0]),
    "matrix_open_host/arity": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4), c.u64("digests", 6, 4), c.u64("tree", 6, 4), 1,
                                                              [0]),
    "matrix_open_host/digests_dtype": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4), c.u64("digests", 6, 4, dtype=I64),
                                                                      c.u64("tree", 6, 4), 2, [0]),
    "matrix_open_host/digests_size": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4), c.u64("digests", 5, 4),
                                                                     c.u64("tree", 6, 4), 2, [0]),
    "matrix_open_host/tree_size": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4), c.u64("digests", 6, 4), c.u64("tree", 5, 4),
                                                                  2, [0]),
    "matrix_open_host/pad_size": lambda H, c: H.matrix_open_host(c.u64("planes", 2, 6, 4), c.u64("digests", 6, 4), c.u64("tree", 6, 4),
                                                                 2, [0], c.u64("pad", 2, 4)),
    "matrix_verify_host/dtype": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 2, 4, dtype=I64), [0, 4], c.u64("paths", 2, 3, 1, 4),
                                                                  2, CAP, TAG),
    "matrix_verify_host/arity": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 2, 4), [0, 4], c.u64("paths", 2, 3, 1, 4), 5, CAP,
                                                                  TAG),
    "matrix_verify_host/rows": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 8), [0, 4], c.u64("paths", 2, 3, 1, 4), 2, CAP, TAG),
    "matrix_verify_host/paths": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 2, 4), [0, 4], c.u64("paths", 2, 3, 2, 4), 2, CAP,
                                                                  TAG),
    "matrix_verify_host/pad_mode": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 2, 4), [0, 4], c.u64("paths", 2, 3, 1, 4), 2, CAP,
                                                                     TAG, 2),
    "matrix_verify_host/out_idx": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 2, 4), [0, 4], c.u64("paths", 2, 3, 1, 4), 2, CAP,
                                                                    TAG, 1, 5),
    "matrix_verify_host/indices": lambda H, c: H.matrix_verify_host(c.u64("rows", 2, 2, 4), [0], c.u64("paths", 2, 3, 1, 4), 2, CAP,
                                                                    TAG),
    "MatrixStream/n_rows": lambda H, c: H.MatrixStream(0, CAP),
    "MatrixStream/n_rows_bool": lambda H, c: H.MatrixStream(True, CAP),
    "MatrixStream.absorb/closed": lambda H, c: _closed(H).absorb(c.u64("planes", 2, 6, 4)),
    "MatrixStream.cols/closed": lambda H, c: _closed(H).cols,
    "MatrixStream.digests/closed": lambda H, c: _closed(H).digests(),
    "MatrixStream.commit/closed": lambda H, c: _closed(H).commit(2, TAG),
    "MatrixStream.absorb/dtype": lambda H, c: _opened(H, c).absorb(c.u64("planes", 2, 6, 4, dtype=I64)),
    "MatrixStream.absorb/contiguous": lambda H, c: _opened(H, c).absorb(_strided(2, 6, 4)),
    "MatrixStream.absorb/ndim": lambda H, c: _opened(H, c).absorb(c.u64("planes", 2, 24)),
    "MatrixStream.absorb/limbs": lambda H, c: _opened(H, c).absorb(c.u64("planes", 2, 6, 5)),
    "MatrixStream.absorb/n_rows": lambda H, c: _opened(H, c).absorb(c.u64("planes", 2, 6, 4), 6),
    "MatrixStream.absorb/stride": lambda H, c: _opened(H, c).absorb(c.u64("planes", 2, 4, 4)),
    "MatrixStream.digests/pad_mode": lambda H, c: _opened(H, c).digests(2),
    "MatrixStream.commit/arity": lambda H, c: _opened(H, c).commit(5, TAG),
    "MatrixStream.commit/pad_mode": lambda H, c: _opened(H, c).commit(2, TAG, 2),
    "MatrixStream.commit/out_idx": lambda H, c: _opened(H, c).commit(2, TAG, 1, 5),
    "MatrixStream.commit/pad_dtype": lambda H, c: _opened(H, c).commit(2, TAG, 1, 1, c.u64("pad", 3, 4, dtype=I64)),
    "MatrixStream.commit/pad_size": lambda H, c: _opened(H, c).commit(2, TAG, 1, 1, c.u64("pad", 2, 4)),
}
for _fn in ("cipher_encrypt_host", "cipher_decrypt_host"):
    _w = 5 if _fn == "cipher_encrypt_host" else 6                                    # scalars per message / per cipher
    HOST_ERRORS.update({
        _fn + "/dtype": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w, 4, dtype=I64), c.u64("keys", 3, 2, 4),
                                                                c.u64("nonces", 3, 4), 5),
        _fn + "/keys_dtype": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w, 4), c.u64("keys", 3, 2, 4, dtype=I64),
                                                                     c.u64("nonces", 3, 4), 5),
        _fn + "/limbs": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w, 3), c.u64("keys", 3, 2, 4), c.u64("nonces", 3, 4),
                                                                5),
        _fn + "/nonce_limbs": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w, 4), c.u64("keys", 3, 2, 4),
                                                                      c.u64("nonces", 3, 3), 5),
        _fn + "/msg_len_0": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w, 4), c.u64("keys", 3, 2, 4),
                                                                    c.u64("nonces", 3, 4), 0),
        _fn + "/msg_len_long": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w, 4), c.u64("keys", 3, 2, 4),
                                                                       c.u64("nonces", 3, 4), 1025),
        _fn + "/keys": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w, 4), c.u64("keys", 3, 4), c.u64("nonces", 3, 4), 5),
        _fn + "/words": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.u64("words", 3, w + 1, 4), c.u64("keys", 3, 2, 4),
                                                                c.u64("nonces", 3, 4), 5),
    })


# ---- device section ---------------------------------------------------------------------------------------------------------
def _round(method):
    def case(H, c):
        it = H.RoundConstantsIter(10)
        return [getattr(H.ScalarStrategy(), method)(it, c.ten("words", 3, 5, 4)), it.pos]
    return case


def _tree9(c, with_pad=False):                  # 9 leaves at arity 2: levels of 5, 3, 2, 1 digests, depth 4
    return (c.ten("leaves", 9, 4), c.ten("tree", 11, 4), 2, c.ten("indices", values=[0, 8])), \
        (c.ten("pad", 4, 4) if with_pad else None)


def _cipher(fn, words_per, *more):
    return lambda H, c: getattr(H, fn)(c.ten("words", 3, words_per, 4), c.ten("keys", 3, 2, 4), c.ten("nonces", 3, 4), 5, *more)


def _sponge_states(H, c):
    s = H.SpongeStates(3, CAP, device=c.device)
    s.absorb(c.ten("blocks", 3, 2, 4, 4))
    return [s.states, s.squeeze(), s.squeeze(2)]


def _safe_sponge(cls):
    def case(H, c):
        s = getattr(H, cls)(3, PATTERN, TAG, device=c.device)
        s.absorb(c.ten("first", 3, 2, 4))
        s.absorb(c.ten("second", 3, 1, 4))
        out = s.squeeze(2)
        if cls == "SafeWitnessSponge":
            s._step.value = s._steps             # what the library would have counted: one step per permutation
        s.finish()
        return [s.states, out] + ([s.wires, s.inputs, s._step.value] if cls == "SafeWitnessSponge" else [])
    return case


def _safe_sponge_wrong(H, c):
    s = H.SafeSponge(3, PATTERN, TAG, device=c.device)
    c.rec.calls.clear()                          # the constructor's call is not the bad call's
    s.squeeze(1)


def _safe_sponge_other_device(H, c):
    s = H.SafeSponge(3, PATTERN, TAG, device=c.device)
    c.rec.calls.clear()
    s.states = s.states.cpu()                    # as far as _same_device can tell: sponges somewhere else
    s.absorb(c.ten("t", 3, 2, 4))


DEVICE_CASES = {
    "add_round_key": _round("add_round_key"),
    "apply_partial_round": _round("apply_partial_round"),
    "apply_full_round": _round("apply_full_round"),
    "mul_matrix": _round("mul_matrix"),
    "quintic_s_box": lambda H, c: H.ScalarStrategy().quintic_s_box(c.ten("value", 7, 4)),
    "perm": lambda H, c: H.ScalarStrategy().perm(c.ten("data", 3, 5, 4)),
    "perm/kernel": lambda H, c: H.ScalarStrategy(2).perm(c.ten("data", 3, 5, 4)),
    "perm_stepwise": lambda H, c: H.ScalarStrategy().perm_stepwise(c.ten("data", 3, 5, 4)),
    "perm_trace": lambda H, c: H.perm_trace(c.ten("states", 3, 5, 4)),
    "perm_trace/out": lambda H, c: H.perm_trace(c.ten("states", 3, 5, 4), 2, c.ten("out", 67, 3, 5, 4)),
    "perm_trace_scaled": lambda H, c: H.perm_trace_scaled(c.ten("states", 3, 5, 4)),
    "perm_trace_scaled/out": lambda H, c: H.perm_trace_scaled(c.ten("states", 3, 5, 4), c.ten("out", 67, 3, 5, 4)),
    "perm_witness": lambda H, c: H.perm_witness(c.ten("states", 3, 5, 4)),
    "perm_witness/out": lambda H, c: H.perm_witness(c.ten("states", 3, 5, 4), c.ten("out", 972, 3, 4)),
    "sponge_witness": lambda H, c: H.sponge_witness(c.ten("msgs", 3, 5, 4), 5, CAP),
    "sponge_witness/digests": lambda H, c: H.sponge_witness(c.ten("msgs", 3, 5, 4), 5, CAP, 0, True),
    "sponge_witness/empty": lambda H, c: H.sponge_witness(c.ten("msgs", 3, 0, 4), 0, CAP),
    "merkle_open_witness": lambda H, c: H.merkle_open_witness(*_tree9(c)[0], TAG),
    "merkle_open_witness/pad": lambda H, c: (lambda a, pad: H.merkle_open_witness(*a, TAG, pad))(*_tree9(c, True)),
    "fr_op/mul": lambda H, c: H.fr_op(H.FR_MUL, c.ten("a", 3, 4), c.ten("b", 3, 4)),
    "fr_op/square": lambda H, c: H.fr_op(H.FR_SQUARE, c.ten("a", 3, 4), None, H.FR_IMPL_SATURATED32),
    "from_bytes": lambda H, c: H.from_bytes(c.ten("bytes", 3, 4)),
    "from_bytes/out": lambda H, c: H.from_bytes(c.ten("bytes", 3, 4), c.ten("out", 3, 4)),
    "to_bytes": lambda H, c: H.to_bytes(c.ten("limbs", 3, 4)),
    "to_bytes/out": lambda H, c: H.to_bytes(c.ten("limbs", 3, 4), c.ten("out", 3, 4)),
    "merkle_level": lambda H, c: H.merkle_level(c.ten("children", 9, 4), 2, TAG),
    "merkle_level/pad": lambda H, c: H.merkle_level(c.ten("children", 9, 4), 3, TAG, 2, c.ten("pad", 1, 4)),
    "merkle_empty_digests": lambda H, c: H.merkle_empty_digests(2, 4, 5, TAG, 2, c.device),
    "merkle_root": lambda H, c: H.merkle_root(c.ten("leaves", 9, 4), 2, TAG),
    "merkle_root/scratch_pad": lambda H, c: H.merkle_root(c.ten("leaves", 9, 4), 2, TAG, 2, c.ten("scratch", 64), c.ten("pad", 4, 4)),
    "merkle_build": lambda H, c: H.merkle_build(c.ten("leaves", 9, 4), 2, TAG),
    "merkle_build/pad": lambda H, c: H.merkle_build(c.ten("leaves", 9, 4), 2, TAG, 2, c.ten("pad", 4, 4)),
    "merkle_open": lambda H, c: H.merkle_open(*_tree9(c)[0]),
    "merkle_open/pad": lambda H, c: (lambda a, pad: H.merkle_open(*a, pad))(*_tree9(c, True)),
    "merkle_verify": lambda H, c: H.merkle_verify(c.ten("values", 2, 4), c.ten("indices", values=[0, 8]), c.ten("paths", 2, 4, 1, 4), 2,
                                                  TAG, 2),
    "merkle_update": lambda H, c: H.merkle_update(*_tree9(c)[0], TAG) is c.keep[1],
    "merkle_update/pad": lambda H, c: (lambda a, pad: H.merkle_update(*a, TAG, 2, pad))(*_tree9(c, True)) is c.keep[1],
    "merkle_forest": lambda H, c: H.merkle_forest(c.ten("leaves", 16, 4), 4, 2, TAG),
    "merkle_forest/scratch": lambda H, c: H.merkle_forest(c.ten("leaves", 16, 4), 4, 2, TAG, 2, c.ten("scratch", 64)),
    "merkle4_level": lambda H, c: H.merkle4_level(c.ten("children", 9, 4), TAG),
    "merkle4_root": lambda H, c: H.merkle4_root(c.ten("leaves", 16, 4), TAG),
    "sponge_hash": lambda H, c: H.sponge_hash(c.ten("msgs", 3, 5, 4), 5, CAP),
    "sponge_hash_var": lambda H, c: H.sponge_hash_var(c.ten("scalars", 9, 4), c.ten("offsets", values=[0, 0, 4]),
                                                      c.ten("lengths", values=[0, 4, 5]), CAP),
    "sponge_hash_var/sort": lambda H, c: H.sponge_hash_var(c.ten("scalars", 9, 4), c.ten("offsets", values=[0, 0, 4]),
                                                           c.ten("lengths", values=[0, 4, 5]), CAP, 0, True),
    "SpongeStates": _sponge_states,
    "cipher_encrypt": _cipher("cipher_encrypt", 5),
    "cipher_decrypt": _cipher("cipher_decrypt", 6, 9),
    "cipher_encrypt_witness": _cipher("cipher_encrypt_witness", 5),
    "cipher_decrypt_witness": _cipher("cipher_decrypt_witness", 6, 9),
    "safe_hash": lambda H, c: H.safe_hash(c.ten("inputs", 3, 3, 4), PATTERN, TAG),
    "safe_witness": lambda H, c: H.safe_witness(c.ten("inputs", 3, 3, 4), PATTERN, TAG),
    "SafeSponge": _safe_sponge("SafeSponge"),
    "SafeWitnessSponge": _safe_sponge("SafeWitnessSponge"),
    "gen_a": lambda H, c: H.gen_a(6, c.device, 3),
    "gen_b": lambda H, c: H.gen_b(6, c.device),
    "gen_b/out": lambda H, c: H.gen_b(6, None, 3, 11, c.ten("out", 6, 4)),
    "digest": lambda H, c: len(H.digest(c.ten("t", 6, 4), 3)),
}
DEVICE_ERRORS = {
    "perm/cpu_tensor": lambda H, c: H.ScalarStrategy().perm(c.ten("data", 3, 5, 4).cpu()),
    "perm/contiguous": lambda H, c: H.ScalarStrategy().perm(c.ten("data", 3, 5, 8)[..., ::2]),
    "perm/size": lambda H, c: H.ScalarStrategy().perm(c.ten("data", 19)),
    "perm/alignment": lambda H, c: H.ScalarStrategy().perm(c.ten("data", 21)[1:]),
    "add_round_key/out_of_constants": lambda H, c: H.ScalarStrategy().add_round_key(H.RoundConstantsIter(956), c.ten("words", 3, 5, 4)),
    "apply_full_round/out_of_constants": lambda H, c: H.ScalarStrategy().apply_full_round(H.RoundConstantsIter(956),
                                                                                          c.ten("words", 3, 5, 4)),
    "apply_partial_round/size": lambda H, c: H.ScalarStrategy().apply_partial_round(H.RoundConstantsIter(), c.ten("words", 19)),
    "sponge_witness/negative": lambda H, c: H.sponge_witness(c.ten("msgs", 3, 5, 4), -1, CAP),
    "sponge_witness/whole_messages": lambda H, c: H.sponge_witness(c.ten("msgs", 3, 5, 4), 4, CAP),
    "sponge_witness/empty_needs_a_tensor": lambda H, c: H.sponge_witness(None, 0, CAP),
    "sponge_witness/pad_mode": lambda H, c: H.sponge_witness(c.ten("msgs", 3, 5, 4), 5, CAP, 2),
    "fr_op/sizes": lambda H, c: H.fr_op(H.FR_ADD, c.ten("a", 3, 4), c.ten("b", 2, 4)),
    "merkle_level/arity": lambda H, c: H.merkle_level(c.ten("children", 9, 4), 5, TAG),
    "merkle_level/pad": lambda H, c: H.merkle_level(c.ten("children", 9, 4), 2, TAG, 1, c.ten("pad", 0, 4)),
    "merkle_root/one_leaf": lambda H, c: H.merkle_root(c.ten("leaves", 1, 4), 2, TAG),
    "merkle_root/pad": lambda H, c: H.merkle_root(c.ten("leaves", 9, 4), 2, TAG, 1, None, c.ten("pad", 3, 4)),
    "merkle_build/arity": lambda H, c: H.merkle_build(c.ten("leaves", 9, 4), 5, TAG),
    "merkle_open/tree": lambda H, c: H.merkle_open(c.ten("leaves", 9, 4), c.ten("tree", 10, 4), 2, c.ten("indices", values=[0])),
    "merkle_open/index": lambda H, c: H.merkle_open(c.ten("leaves", 9, 4), c.ten("tree", 11, 4), 2, c.ten("indices", values=[9])),
    "merkle_open_witness/tree": lambda H, c: H.merkle_open_witness(c.ten("leaves", 9, 4), c.ten("tree", 10, 4), 2,
                                                                   c.ten("indices", values=[0]), TAG),
    "merkle_update/tree": lambda H, c: H.merkle_update(c.ten("leaves", 9, 4), c.ten("tree", 10, 4), 2, c.ten("indices", values=[0]),
                                                       TAG),
    "merkle_verify/counts": lambda H, c: H.merkle_verify(c.ten("values", 2, 4), c.ten("indices", values=[0]), c.ten("paths", 2, 4, 1, 4),
                                                         2, TAG),
    "merkle_forest/split": lambda H, c: H.merkle_forest(c.ten("leaves", 16, 4), 3, 2, TAG),
    "sponge_hash/msg_len": lambda H, c: H.sponge_hash(c.ten("msgs", 3, 5, 4), 0, CAP),
    "sponge_hash/whole_messages": lambda H, c: H.sponge_hash(c.ten("msgs", 3, 5, 4), 4, CAP),
    "sponge_hash_var/index": lambda H, c: H.sponge_hash_var(c.ten("scalars", 9, 4), c.ten("offsets", values=[0, 0, 4]),
                                                            c.ten("lengths", values=[0, 4]), CAP),
    "safe_hash/pattern": lambda H, c: H.safe_hash(c.ten("inputs", 3, 3, 4), [("squeeze", 2)], TAG),
    "safe_hash/whole_inputs": lambda H, c: H.safe_hash(c.ten("inputs", 4, 4), PATTERN, TAG),
    "safe_hash/cpu_tensor": lambda H, c: H.safe_hash(c.ten("inputs", 3, 3, 4).cpu(), PATTERN, TAG),
    "safe_witness/whole_inputs": lambda H, c: H.safe_witness(c.ten("inputs", 4, 4), PATTERN, TAG),
    "SafeSponge/pattern": lambda H, c: H.SafeSponge(3, [("squeeze", 2)], TAG, device=c.device),
    "SafeSponge/wrong_kind": _safe_sponge_wrong,
    "SafeSponge/other_device": _safe_sponge_other_device,
    "digest/size": lambda H, c: H.digest(c.ten("t", 6, 4)[:, :1].contiguous().view(c.torch.int8).reshape(-1)[:3]),
}
for _fn, _w in (("cipher_encrypt", 5), ("cipher_decrypt", 6), ("cipher_encrypt_witness", 5), ("cipher_decrypt_witness", 6)):
    DEVICE_ERRORS.update({
        _fn + "/msg_len": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.ten("words", 3, w, 4), c.ten("keys", 3, 2, 4), c.ten("nonces", 3, 4),
                                                                  0),
        _fn + "/keys": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.ten("words", 3, w, 4), c.ten("keys", 3, 4), c.ten("nonces", 3, 4), 5),
        _fn + "/words": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.ten("words", 3, w + 1, 4), c.ten("keys", 3, 2, 4),
                                                                c.ten("nonces", 3, 4), 5),
        _fn + "/cpu_tensor": lambda H, c, f=_fn, w=_w: getattr(H, f)(c.ten("words", 3, w, 4), c.ten("keys", 3, 2, 4).cpu(),
                                                                     c.ten("nonces", 3, 4), 5),
    })


# ---- running a section ------------------------------------------------------------------------------------------------------
def run_section(H, rec, cases, errors, torch=None, device=None):
    out = {"calls": {}, "errors": {}}
    ctx = None
    for name, case in cases.items():
        ctx = Ctx(rec, torch, device)           # the case before is dropped here (a MatrixStream closes), ahead of the reset
        rec.calls, rec.names = [], {}
        result = case(H, ctx)
        out["calls"][name] = {"calls": list(rec.calls), "returns": describe(result)}
    for name, case in errors.items():
        ctx = Ctx(rec, torch, device)
        rec.calls, rec.names = [], {}
        try:
            case(H, ctx)
            raised = None
        except Exception as e:                                          # the TYPE is the record
            raised = type(e).__name__
        out["errors"][name] = {"raises": raised, "calls": list(rec.calls)}
    return out


def record_host(swap):
    from hades252_amd import _lib, strategy as H
    rec = Recorder(_lib.lib(), _lib.SIGNATURES)
    swap(_lib, "lib", lambda: rec)
    return run_section(H, rec, HOST_CASES, HOST_ERRORS)


def record_device(swap):
    """Tensors on the LAST visible device and on a stream of their own there, the current device left at 0: with more than
    one device only the wrappers' own guard makes the recorder's check pass.  With ONE visible device both are device 0 and
    the device half of the check cannot fail; the stream half (a stream of the test's own, never the default one) still can."""
    import torch
    from hades252_amd import _lib, strategy as H
    assert torch.cuda.is_available(), "the device section needs a GPU"
    rec = Recorder(_lib.lib(), _lib.SIGNATURES)
    rec.torch, rec.device = torch, torch.device("cuda", torch.cuda.device_count() - 1)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=rec.device)
    with torch.cuda.device(rec.device):
        torch.cuda.set_stream(stream)
    swap(_lib, "lib", lambda: rec)
    try:
        out = run_section(H, rec, DEVICE_CASES, DEVICE_ERRORS, torch, rec.device)
        assert torch.cuda.current_stream(rec.device).cuda_stream == stream.cuda_stream != 0
    finally:
        with torch.cuda.device(rec.device):
            torch.cuda.set_stream(torch.cuda.default_stream(rec.device))
        torch.cuda.synchronize(rec.device)
    assert not rec.guard_failures, rec.guard_failures
    return out


def _compare(got, section):
    with open(GOLDEN) as f:
        want = json.load(f)[section]
    for kind in ("calls", "errors"):
        assert sorted(got[kind]) == sorted(want[kind]), "the fixture's %s cases are not the test's" % section
        for name in got[kind]:
            assert got[kind][name] == want[kind][name], "%s: %s: %r, recorded %r" % (section, name, got[kind][name], want[kind][name])
    for name, entry in got["errors"].items():
        assert entry["raises"] is not None and entry["calls"] == [], "%s: %s: %r" % (section, name, entry)


def test_host_wrappers_make_the_recorded_calls(hades_lib, monkeypatch):
    _compare(json.loads(json.dumps(record_host(monkeypatch.setattr))), "host")


@pytest.mark.gpu
def test_device_wrappers_make_the_recorded_calls_under_their_device_and_stream(hades_lib, torch_cuda, monkeypatch):
    _compare(json.loads(json.dumps(record_device(monkeypatch.setattr))), "device")


def _dump(doc) -> str:
    """One line per case: a diff of the fixture names the wrapper."""
    parts = []
    for section in sorted(doc):
        kinds = []
        for kind in ("calls", "errors"):
            lines = ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in doc[section][kind].items())
            kinds.append("  %s: {\n%s\n  }" % (json.dumps(kind), lines))
        parts.append(" %s: {\n%s\n }" % (json.dumps(section), ",\n".join(kinds)))
    return "{\n%s\n}\n" % ",\n".join(parts)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_strategy_calls.py --record")
    sys.path.insert(0, ROOT)
    from hades252_amd import build, _lib as L
    build.build(verbose=False)
    real = L.lib
    doc = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            doc = json.load(f)
    doc["host"] = record_host(setattr)
    L.lib = real
    try:
        import torch
        have = torch.cuda.is_available()
    except ImportError:
        have = False
    if have:
        doc["device"] = record_device(setattr)
        L.lib = real
    doc = json.loads(json.dumps(doc))
    assert json.loads(_dump(doc)) == doc
    with open(GOLDEN, "w") as f:
        f.write(_dump(doc))
    print("recorded %s into %s (%d bytes)" % (", ".join(sorted(doc)), GOLDEN, os.path.getsize(GOLDEN)))
