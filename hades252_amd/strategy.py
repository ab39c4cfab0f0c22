"""Host-side mirror of the reference's operator interface for the hot path.

The reference exposes ``pub trait Strategy<T>`` (src/strategies.rs:31-163) and the implementor
``ScalarStrategy`` (src/strategies/scalar.rs:11-50).  This module keeps the same names, argument
meaning and error behaviour, batched: wherever the reference takes ``&mut [BlsScalar]`` of
exactly ``WIDTH`` words, these methods take a buffer holding any whole number of states
(AoS, 160 bytes each, in-memory ``BlsScalar`` = 4 x u64 LE Montgomery limbs) and apply the
operation to every state, in place, on the GPU through the C ABI of ``include/hades252.h``.

Buffers
  * ``torch.Tensor`` on a ``cuda`` device (any integer dtype, contiguous): device path,
    asynchronous on the current torch stream -- zero-copy.
  * ``numpy.ndarray`` of dtype uint64 (C-contiguous): host path, synchronous, the library moves
    the data (``hades252_perm_batch``); only ``perm`` supports it.
    RATE WARNING for this path: in a process that imported ``torch`` first, the library runs on the
    HIP runtime PyTorch bundles (ROCm 7.0.2), which serialises the copy-in and copy-out streams of
    the chunk pipeline -- 2^22 states take 29.6 ms (22.7 GB/s each way: the rate the system
    runtime gives with ``HSA_ENABLE_SDMA=0``) against 15.1 ms on the system runtime (ROCm 7.2) a
    native / Rust caller links.  No environment setting repairs it (``HSA_ENABLE_SDMA``,
    ``GPU_MAX_HW_QUEUES``, ``HSA_ENABLE_INTERRUPT``, ``HIP_FORCE_DEV_KERNARG``: no change;
    ``AMD_DIRECT_DISPATCH=0``: 24 ms; chunk sizes 2^14 .. 2^18 states: 27-33 ms), and the library cannot: the cause is inside that runtime
    (profiles/r5/host_path_torch_probe.txt).  A host-only Python caller does not need torch -- use
    this module WITHOUT importing torch (the library then binds the system runtime: 15.1 ms).
    Binding the system runtime first and importing torch afterwards is also full speed, but puts
    two HIP runtimes in one process: torch tensors and streams must then never be passed to the
    device path.

There is no CPU implementation behind these methods: if ``libhades252.so`` is not built or no
GPU is usable they raise.
"""
from __future__ import annotations

import ctypes
from typing import Iterator

import numpy as np

from . import PARTIAL_ROUNDS, TOTAL_FULL_ROUNDS, WIDTH, _lib
from ._lib import check

STATE_BYTES = WIDTH * 32
ROUNDS_TOTAL = TOTAL_FULL_ROUNDS + PARTIAL_ROUNDS          # HADES252_ROUNDS_TOTAL, src/strategies.rs:160-162
N_ROUND_CONSTANTS = 960          # src/round_constants.rs:18 (335 are ever consumed)


class RoundConstantsIter:
    """``ROUND_CONSTANTS.iter()`` (src/strategies.rs:141): a cursor into the constant table.
    The table itself lives in device memory; the cursor is an index."""

    def __init__(self, pos: int = 0):
        self.pos = pos

    def __iter__(self) -> Iterator[int]:
        return self

    def __next__(self) -> int:
        if self.pos >= N_ROUND_CONSTANTS:
            raise StopIteration
        self.pos += 1
        return self.pos - 1


# ---- the device path: torch is imported here, on first use, never at module import (see the RATE WARNING above) -------
def _dev_buffer(x, unit_bytes: int, what: str):
    """-> (data_ptr, n_units, torch device) of a contiguous CUDA tensor."""
    import torch
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise TypeError("%s: expected a CUDA torch.Tensor" % what)
    if not x.is_contiguous():
        raise ValueError("%s: tensor must be contiguous" % what)
    nbytes = x.numel() * x.element_size()
    # same failure the reference has for a slice whose length is not WIDTH
    # (copy_from_slice length panic, src/strategies/scalar.rs:48)
    if nbytes % unit_bytes != 0:
        raise ValueError("%s: buffer of %d bytes is not a whole number of %d-byte units"
                         % (what, nbytes, unit_bytes))
    if x.data_ptr() % 16 != 0:
        raise ValueError("%s: buffer must be 16-byte aligned" % what)
    return x.data_ptr(), nbytes // unit_bytes, x.device


def _stream_ptr(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def _dev_call(where: str, dev, fn_name: str, *args, after=()) -> None:
    """The one way into a ``_dev`` entry point of the library: with ``dev`` current and on torch's current stream there.
    The stream follows ``args``; ``after`` is what an ``_ex`` signature still takes behind it."""
    import torch
    with torch.cuda.device(dev):
        check(getattr(_lib.lib(), fn_name)(*args, _stream_ptr(dev), *after), where)


def _dev_empty(dev, *shape, dtype: str = "int64"):
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype), device=dev)


def _dev_counter(dev):
    """One zeroed int32 the library counts into (rejected messages, indices out of range, ...)."""
    import torch
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _witness_pair(dev, steps: int, n: int):
    """(wires [972, steps, n, 4], inputs [steps, n, 5, 4]): the two record buffers of a chain witness."""
    return _dev_empty(dev, witness_wires(), steps, n, 4), _dev_empty(dev, steps, n, WIDTH, 4)


# ---- the host path ---------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _host_u64(a, what: str, tail: tuple | None = None) -> np.ndarray:
    """Type and contiguity of a host batch and, when ``tail`` is given, its shape [n, *tail]."""
    if not isinstance(a, np.ndarray) or a.dtype != np.uint64 or not a.flags.c_contiguous:
        raise TypeError("%s: host buffers must be C-contiguous numpy uint64" % what)
    if tail is not None and (a.ndim != 1 + len(tail) or a.shape[1:] != tail):
        raise ValueError("%s: the input must have shape [n, %s], got %r" % (what, ", ".join(map(str, tail)), a.shape))
    return a


def _host_units(a, what: str, limbs: int = 4) -> int:
    """How many units of ``limbs`` uint64 (4: a scalar, 20: a state) a valid host batch holds."""
    if _host_u64(a, what).size % limbs:
        raise ValueError("%s: %d limbs is not a whole number of %d-limb units" % (what, a.size, limbs))
    return a.size // limbs


def _host_pad(where: str, pad, depth: int):
    """The pointer of a host padding table [depth, 4], None for None."""
    if pad is None:
        return None
    if _host_u64(pad, where).size != depth * 4:
        raise ValueError("%s: the padding table needs %d digests" % (where, depth))
    return _ptr(pad)


def _tag_arr(tag_mont: int):
    return (ctypes.c_uint64 * 4)(*[(tag_mont >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)])


class Strategy:
    """Mirror of ``pub trait Strategy<T: Clone + Copy>`` (src/strategies.rs:31)."""

    @staticmethod
    def next_c(constants: RoundConstantsIter) -> int:
        """src/strategies.rs:33-41 -- returns the index of the constant consumed."""
        try:
            return next(constants)
        except StopIteration:
            raise RuntimeError("Hades252 out of ARK constants") from None

    # required methods of the trait (src/strategies.rs:50-65)
    def add_round_key(self, constants: RoundConstantsIter, words) -> None:
        raise NotImplementedError

    def quintic_s_box(self, value) -> None:
        raise NotImplementedError

    def mul_matrix(self, constants: RoundConstantsIter, values) -> None:
        raise NotImplementedError

    # provided methods (src/strategies.rs:79-157)
    def apply_partial_round(self, constants: RoundConstantsIter, words) -> None:
        raise NotImplementedError

    def apply_full_round(self, constants: RoundConstantsIter, words) -> None:
        raise NotImplementedError

    def perm(self, data) -> None:
        raise NotImplementedError

    @staticmethod
    def rounds() -> int:
        """src/strategies.rs:160-162."""
        return ROUNDS_TOTAL


class ScalarStrategy(Strategy):
    """Batched GPU ``ScalarStrategy`` (src/strategies/scalar.rs:11-50).  Stateless, like the
    reference's zero-sized struct; ``kernel`` selects one of the two bit-identical kernels."""

    def __init__(self, kernel: int = _lib.KERNEL_DEFAULT):
        self.kernel = kernel
        _lib.lib()                       # fail loudly at construction if the library is missing

    @classmethod
    def new(cls) -> "ScalarStrategy":
        """src/strategies/scalar.rs:17-19."""
        return cls()

    @staticmethod
    def _cursor_of(constants: RoundConstantsIter) -> int:
        # any cursor is legal (the trait methods take the iterator wherever it stands,
        # src/strategies.rs:33-41); running past the 960 constants is the reference's panic
        if constants.pos + WIDTH > N_ROUND_CONSTANTS:
            raise RuntimeError("Hades252 out of ARK constants")
        return constants.pos

    def _round_at_cursor(self, op: str, constants: RoundConstantsIter, words) -> None:
        """``hades252_<op>_at_dev`` on every state of ``words``; the cursor moves on by WIDTH constants."""
        ptr, n, dev = _dev_buffer(words, STATE_BYTES, op)
        _dev_call(op, dev, "hades252_%s_at_dev" % op, ptr, n, self._cursor_of(constants))
        for _ in range(WIDTH):
            self.next_c(constants)

    def add_round_key(self, constants: RoundConstantsIter, words) -> None:
        """src/strategies/scalar.rs:23-30: word w of every state += next_c()."""
        self._round_at_cursor("add_round_key", constants, words)

    def quintic_s_box(self, value) -> None:
        """src/strategies/scalar.rs:32-34 on every 32-byte scalar of ``value``."""
        ptr, n, dev = _dev_buffer(value, 32, "quintic_s_box")
        _dev_call("quintic_s_box", dev, "hades252_quintic_s_box_dev", ptr, n)

    def mul_matrix(self, constants: RoundConstantsIter, values) -> None:
        """src/strategies/scalar.rs:36-49 (``_constants`` is unused there too)."""
        ptr, n, dev = _dev_buffer(values, STATE_BYTES, "mul_matrix")
        _dev_call("mul_matrix", dev, "hades252_mul_matrix_dev", ptr, n)

    def apply_partial_round(self, constants: RoundConstantsIter, words) -> None:
        """src/strategies.rs:79-93, fused in one launch."""
        self._round_at_cursor("apply_partial_round", constants, words)

    def apply_full_round(self, constants: RoundConstantsIter, words) -> None:
        """src/strategies.rs:107-119, fused in one launch."""
        self._round_at_cursor("apply_full_round", constants, words)

    def perm(self, data) -> None:
        """src/strategies.rs:140-157 on every state of ``data``, in place."""
        if isinstance(data, np.ndarray):
            # the one host batch that is checked and pointed at inline, beside _host_u64 and _ptr: single-call timings
            # (bench.py single_perm, tools/small_call_latency.py) see every Python call made between here and the library
            if data.dtype != np.uint64 or not data.flags.c_contiguous:
                raise TypeError("perm: host buffers must be C-contiguous numpy uint64")
            if data.size % (WIDTH * 4) != 0:
                raise ValueError("perm: %d limbs is not a whole number of %d-word states" % (data.size, WIDTH))
            check(_lib.lib().hades252_perm_batch(data.ctypes.data_as(ctypes.c_void_p), data.size // (WIDTH * 4)), "perm")
            return
        ptr, n, dev = _dev_buffer(data, STATE_BYTES, "perm")
        _dev_call("perm", dev, "hades252_perm_batch_dev_ex", ptr, n, after=(self.kernel,))

    def perm_stepwise(self, data) -> None:
        """The provided ``perm`` body of the trait written out over the per-round entry points
        (src/strategies.rs:140-157): 4 full, 59 partial, 4 full, one shared cursor."""
        constants = RoundConstantsIter()
        for _ in range(TOTAL_FULL_ROUNDS // 2):
            self.apply_full_round(constants, data)
        for _ in range(PARTIAL_ROUNDS):
            self.apply_partial_round(constants, data)
        for _ in range(TOTAL_FULL_ROUNDS // 2):
            self.apply_full_round(constants, data)


def kernel_for(n_perms: int) -> int:
    """The selector ``hades252_perm_batch_dev`` runs for a batch of n_perms states (the library's one size rule)."""
    return _lib.lib().hades252_kernel_for(n_perms)


def chain_form_for(n_chains: int) -> int:
    """The form the chain entry points (sponge, absorb, verify, update) and Merkle levels run for n_chains chains."""
    return _lib.lib().hades252_chain_form_for(n_chains)


def kernel_name(kernel: int = _lib.KERNEL_DEFAULT, n_perms: int = 0) -> str:
    """Name of the __global__ function a profiler shows for ``hades252_perm_batch_dev_ex(.., n_perms, .., kernel)``."""
    name = _lib.lib().hades252_kernel_name(kernel, n_perms)
    if name is None:
        raise ValueError("unknown kernel selector %r" % (kernel,))
    return name.decode()


def warm_up(n_perms_hint: int = 0) -> None:
    """``hades252_warm_up``: load the code object and pre-create the pipe a host batch of ``n_perms_hint`` states would take."""
    check(_lib.lib().hades252_warm_up(int(n_perms_hint)), "warm_up")


def trim() -> None:
    """``hades252_trim``: give back everything the pool of pipes caches (device memory, streams, staging buffers)."""
    check(_lib.lib().hades252_trim(), "trim")


def pool_bytes() -> int:
    """``hades252_pool_bytes``: device memory the pool holds right now."""
    return int(_lib.lib().hades252_pool_bytes())


def fault_inject(spec: str | None) -> None:
    """Test hook ``hades252_fault_inject``: "<site>:<nth>" arms, None disarms."""
    check(_lib.lib().hades252_fault_inject(None if spec is None else spec.encode()), "fault_inject")


class HostBuffer:
    """Page-locked host memory for the host-pointer path (``hades252_host_alloc`` / ``_free``): what a Rust caller
    keeps its long-lived ``Vec<BlsScalar>`` in, so that ``perm`` goes straight to DMA instead of page-locking the
    slice on every call.  ``.array`` is a numpy uint64 view (20 limbs per state); close() frees the memory (the
    view must not be used afterwards)."""

    def __init__(self, n_states: int):
        self.ptr = ctypes.c_void_p()
        self.nbytes = max(1, n_states) * STATE_BYTES
        check(_lib.lib().hades252_host_alloc(ctypes.byref(self.ptr), self.nbytes), "host_alloc")
        raw = (ctypes.c_uint64 * (n_states * WIDTH * 4)).from_address(self.ptr.value)
        self.array = np.frombuffer(raw, dtype=np.uint64)

    def close(self) -> None:
        if self.ptr:
            self.array = None
            check(_lib.lib().hades252_host_free(self.ptr), "host_free")
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def host_register(arr: np.ndarray) -> None:
    """Page-lock an existing host array in place, once (``hades252_host_register``)."""
    check(_lib.lib().hades252_host_register(_ptr(arr), arr.nbytes), "host_register")


def host_unregister(arr: np.ndarray) -> None:
    check(_lib.lib().hades252_host_unregister(_ptr(arr)), "host_unregister")


def host_is_pinned(arr: np.ndarray) -> bool:
    return bool(_lib.lib().hades252_host_is_pinned(_ptr(arr), arr.nbytes))


def perm_multi(data: np.ndarray, n_workers: int = 0, virtual: bool = False) -> None:
    """``hades252_perm_batch_multi_ex``: a host batch sharded over n_workers host threads / devices (0 = every
    visible device), contiguous range per worker, no collective.  ``virtual``: worker g runs on device
    g % device_count, so n_workers may exceed the number of GPUs."""
    n = _host_units(data, "perm_multi", WIDTH * 4)
    check(_lib.lib().hades252_perm_batch_multi_ex(_ptr(data), n, n_workers, _lib.MULTI_VIRTUAL if virtual else 0), "perm_multi")


def merkle_root_host(leaves: np.ndarray, arity: int, tag_mont: int, out_idx: int = 1, pad: np.ndarray | None = None) -> np.ndarray:
    """``hades252_merkle_root``: root (4 limbs) of the tree over leaves held in HOST memory (n x 4 uint64); the leaves travel
    to the device in chunks while the first tree level is hashed behind them.  ``pad``: host table [depth, 4] or None."""
    n = _host_units(leaves, "merkle_root_host")
    pptr = _host_pad("merkle_root_host", pad, merkle_depth(n, arity, "merkle_root_host"))
    root = np.zeros(4, dtype=np.uint64)
    check(_lib.lib().hades252_merkle_root(_ptr(leaves), n, arity, _tag_arr(tag_mont), out_idx, pptr, _ptr(root)),
          "merkle_root_host")
    return root


def merkle_root_multi(leaves: np.ndarray, arity: int, tag_mont: int, out_idx: int = 1, n_workers: int = 0, virtual: bool = False):
    """``hades252_merkle_root_multi``: the root of a FULL tree (arity^k leaves in host memory), sub-trees sharded over
    n_workers devices (0 = all visible); ``virtual``: worker g on device g % device_count."""
    leaves = _host_u64(leaves, "merkle_root_multi")
    root = np.zeros(4, dtype=np.uint64)
    check(_lib.lib().hades252_merkle_root_multi(_ptr(leaves), leaves.size // 4, arity, _tag_arr(tag_mont), out_idx, n_workers,
                                                _lib.MULTI_VIRTUAL if virtual else 0, _ptr(root)), "merkle_root_multi")
    return root


def sponge_hash_host(msgs: np.ndarray, n_msgs: int, msg_len: int, capacity_mont: int, pad_mode: int = 1) -> np.ndarray:
    """``hades252_sponge_hash``: digests [n_msgs, 4] of n_msgs fixed-length messages held in HOST memory."""
    msgs = _host_u64(msgs, "sponge_hash_host")
    if msgs.size != n_msgs * msg_len * 4:
        raise ValueError("sponge_hash_host: buffer is not %d messages of %d scalars" % (n_msgs, msg_len))
    out = np.zeros((n_msgs, 4), dtype=np.uint64)
    check(_lib.lib().hades252_sponge_hash(_ptr(msgs) if msgs.size else None, n_msgs, msg_len, _tag_arr(capacity_mont), pad_mode,
                                          _ptr(out)), "sponge_hash_host")
    return out


def sponge_hash_var_host(scalars: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, capacity_mont: int, pad_mode: int = 1):
    """``hades252_sponge_hash_var``: (digests [n, 4], number of out-of-pool messages) for ragged messages in HOST memory."""
    scalars, offsets, lengths = (_host_u64(a, "sponge_hash_var_host") for a in (scalars, offsets, lengths))
    if scalars.size % 4 or offsets.size != lengths.size:
        raise ValueError("sponge_hash_var_host: malformed pool / index arrays")
    n = offsets.size
    out = np.zeros((n, 4), dtype=np.uint64)
    bad = ctypes.c_size_t(0)
    check(_lib.lib().hades252_sponge_hash_var(_ptr(scalars) if scalars.size else None, scalars.size // 4, _ptr(offsets),
                                              _ptr(lengths), n, _tag_arr(capacity_mont), pad_mode, _ptr(out), ctypes.byref(bad)),
          "sponge_hash_var_host")
    return out, int(bad.value)


def _trace(where: str, fn_name: str, states_t, out, after=()):
    ptr, n, dev = _dev_buffer(states_t, STATE_BYTES, where)
    trace = _dev_empty(dev, ROUNDS_TOTAL, n, WIDTH, 4) if out is None else out
    _dev_call(where, dev, fn_name, ptr, trace.data_ptr(), n, after=after)
    return trace


def perm_trace(states_t, kernel: int = _lib.KERNEL_DEFAULT, out=None):
    """State after every round (round-major: result[r] is the batch after round r); the input is
    left untouched.  Witness pre-computation for the reference's GadgetStrategy
    (src/strategies/gadget.rs:41-133)."""
    return _trace("perm_trace", "hades252_perm_trace_dev_ex", states_t, out, (kernel,))


def perm_trace_scaled(states_t, out=None):
    """The per-round trace in SCALED form (include/hades252.h: hades252_perm_trace_scaled_dev): same shape as
    ``perm_trace``; ``true[r][w] = scaled[r][w] * mul[r] + add[r][w]`` with the tables of ``trace_scale_table()``."""
    return _trace("perm_trace_scaled", "hades252_perm_trace_scaled_dev", states_t, out)


def trace_scale_table():
    """(mul [67, 4], add [67, 5, 4]) uint64 numpy arrays: in-memory BlsScalar limbs (host tables, no device call)."""
    mul = np.zeros((ROUNDS_TOTAL, 4), dtype=np.uint64)
    add = np.zeros((ROUNDS_TOTAL, WIDTH, 4), dtype=np.uint64)
    check(_lib.lib().hades252_perm_trace_scale_table(_ptr(mul), _ptr(add)), "trace_scale_table")
    return mul, add


def witness_wires() -> int:
    """Gate outputs per permutation (972): the first dimension of what ``perm_witness`` returns."""
    return int(_lib.lib().hades252_witness_wires())


def perm_witness(states_t, out=None):
    """Every gate output of the reference's GadgetStrategy (src/strategies/gadget.rs:41-133) for every state:
    [972, n, 4] int64, wire-major in gate order (include/hades252.h).  The input is left untouched."""
    ptr, n, dev = _dev_buffer(states_t, STATE_BYTES, "perm_witness")
    wires = _dev_empty(dev, witness_wires(), n, 4) if out is None else out
    _dev_call("perm_witness", dev, "hades252_perm_witness_dev", ptr, wires.data_ptr(), n)
    return wires


def sponge_blocks(msg_len: int, pad_mode: int = 1) -> int:
    """Permutations per message of the fixed-length sponge (``hades252_sponge_blocks``): ceil((msg_len + pad) / 4), at
    least one."""
    if pad_mode not in (0, 1):
        raise ValueError("sponge_blocks: pad_mode must be 0 or 1")
    return int(_lib.lib().hades252_sponge_blocks(msg_len, pad_mode))


def _dev_messages(where: str, msgs_t, msg_len: int):
    """-> (data_ptr, n, device) of a tensor that holds n messages of msg_len > 0 scalars."""
    ptr, n_scalars, dev = _dev_buffer(msgs_t, 32, where)
    if n_scalars % msg_len != 0:
        raise ValueError("%s: buffer is not a whole number of messages" % where)
    return ptr, n_scalars // msg_len, dev


def sponge_witness(msgs_t, msg_len: int, capacity_mont: int, pad_mode: int = 1, digests: bool = False):
    """Gadget witness of the fixed-length sponge (``hades252_sponge_witness_dev``): msgs_t holds n messages of msg_len
    scalars (msg_len 0: a tensor of shape [n, 0, ...] names n).  Returns (wires [972, S, n, 4], inputs [S, n, 5, 4]
    [, digests [n, 4]]) with S = sponge_blocks(msg_len, pad_mode): inputs[s, i] is the state that enters permutation s of
    message i and wires.reshape(972, S * n, 4) == perm_witness(inputs) byte for byte."""
    import torch
    if msg_len < 0:
        raise ValueError("sponge_witness: msg_len must not be negative")
    if msg_len > 0:
        ptr, n, dev = _dev_messages("sponge_witness", msgs_t, msg_len)
    else:
        if not isinstance(msgs_t, torch.Tensor) or msgs_t.device.type != "cuda" or msgs_t.dim() < 1:
            raise TypeError("sponge_witness: msg_len 0 needs a CUDA tensor of shape [n, 0, ...]")
        ptr, n, dev = None, int(msgs_t.shape[0]), msgs_t.device
    wires, inputs = _witness_pair(dev, sponge_blocks(msg_len, pad_mode), n)
    dig = _dev_empty(dev, n, 4) if digests else None
    _dev_call("sponge_witness", dev, "hades252_sponge_witness_dev", ptr, n, msg_len, _tag_arr(capacity_mont), pad_mode,
              inputs.data_ptr(), wires.data_ptr(), None if dig is None else dig.data_ptr())
    return (wires, inputs, dig) if digests else (wires, inputs)


def merkle_open_witness(leaves_t, tree_t, arity: int, indices_t, tag_mont: int, pad=None):
    """Gadget witness of Merkle openings (``hades252_merkle_open_witness_dev``) over the tree of ``merkle_build`` (same
    arity, tag, pad).  Returns (wires [972, depth, n_queries, 4], inputs [depth, n_queries, 5, 4], n_bad): inputs[l, q] =
    [tag, the children of the level-l group on leaf indices[q]'s path, 0 ...]; an index >= n_leaves gets all-zero states
    and is counted in n_bad (synchronises with the device)."""
    ptr, n, dev = _dev_buffer(leaves_t, 32, "merkle_open_witness")
    depth = merkle_depth(n, arity, "merkle_open_witness")
    tptr = _tree_of("merkle_open_witness", tree_t, n, arity)
    iptr, nq, _ = _dev_buffer(indices_t, 8, "merkle_open_witness")
    wires, inputs = _witness_pair(dev, depth, nq)
    bad = _dev_counter(dev)
    _dev_call("merkle_open_witness", dev, "hades252_merkle_open_witness_dev", ptr, tptr, n, arity, _tag_arr(tag_mont),
              _pad_ptr(pad, depth, "merkle_open_witness"), iptr, nq, inputs.data_ptr(), wires.data_ptr(), bad.data_ptr())
    return wires, inputs, int(bad.item())


FR_ADD, FR_MUL, FR_SQUARE, FR_FROM_RAW, FR_REDUCE_SIGNED = 0, 1, 2, 3, 4
FR_IMPL_SATURATED32, FR_IMPL_RADIX29 = 0, 1


def fr_op(op: int, a_t, b_t=None, impl: int = FR_IMPL_RADIX29):
    """Batched ``BlsScalar`` add / mul / square / from_raw on device (include/hades252.h)."""
    import torch
    ptr, n, dev = _dev_buffer(a_t, 32, "fr_op")
    bptr = 0
    if b_t is not None:
        bptr, nb, _ = _dev_buffer(b_t, 32, "fr_op")
        if nb != n:
            raise ValueError("fr_op: operand sizes differ")
    out = torch.empty_like(a_t)
    _dev_call("fr_op", dev, "hades252_fr_op_dev", op, impl, ptr, bptr, out.data_ptr(), n)
    return out


# ---- helpers around the strategy (wire format, Merkle, synthetic data) ----------------------
def _wire_buffers(where: str, in_t, out_t):
    """-> (in pointer, out pointer, n, device, out tensor) of a 32-byte-per-scalar conversion; out_t None: a new tensor."""
    import torch
    ptr, n, dev = _dev_buffer(in_t, 32, where)
    out_t = torch.empty_like(in_t) if out_t is None else out_t
    optr, n2, _ = _dev_buffer(out_t, 32, where)
    assert n2 == n
    return ptr, optr, n, dev, out_t


def from_bytes(bytes_t, out_t=None):
    """``BlsScalar::from_bytes`` on device: 32-byte canonical LE -> Montgomery limbs.
    Raises ValueError if any input is >= p (the reference returns an error option)."""
    ptr, optr, n, dev, out_t = _wire_buffers("from_bytes", bytes_t, out_t)
    bad = _dev_counter(dev)
    _dev_call("from_bytes", dev, "hades252_from_bytes_dev", ptr, optr, n, bad.data_ptr())
    if int(bad.item()) != 0:
        raise ValueError("from_bytes: %d scalar(s) not canonical (>= p)" % int(bad.item()))
    return out_t


def to_bytes(limbs_t, out_t=None):
    """``BlsScalar::to_bytes`` on device."""
    ptr, optr, n, dev, out_t = _wire_buffers("to_bytes", limbs_t, out_t)
    _dev_call("to_bytes", dev, "hades252_to_bytes_dev", ptr, optr, n)
    return out_t


def merkle_depth(n: int, arity: int, what: str = "merkle") -> int:
    """Levels above the leaves (n_l = ceil(n_{l-1} / arity)); raises for an invalid shape."""
    d = _lib.lib().hades252_merkle_depth(n, arity)
    if d < 1:
        raise ValueError("%s: need arity 2..4 and at least 2 leaves (got arity %d, %d leaves)" % (what, arity, n))
    return d


def merkle_level_sizes(n: int, arity: int):
    """[n_1, n_2, ..., 1]: nodes per level above the leaves."""
    out = []
    while n > 1:
        n = -(-n // arity)
        out.append(n)
    return out


def _pad_ptr(pad_t, depth: int, what: str):
    if pad_t is None:
        return 0
    ptr, n, _ = _dev_buffer(pad_t, 32, what)
    if n < depth:
        raise ValueError("%s: the padding table needs one digest per level (%d)" % (what, depth))
    return ptr


def _tree_of(where: str, tree_t, n: int, arity: int) -> int:
    """The pointer of ``tree_t`` if it is what ``merkle_build`` returns for n leaves."""
    tptr, nt, _ = _dev_buffer(tree_t, 32, where)
    if nt != sum(merkle_level_sizes(n, arity)):
        raise ValueError("%s: tree buffer does not belong to %d leaves" % (where, n))
    return tptr


def _dev_scratch(dev, scratch, need_bytes: int):
    """-> (pointer, bytes) of the caller's scratch tensor, or of a new one of need_bytes."""
    if scratch is None:
        scratch = _dev_empty(dev, max(need_bytes // 8, 2))
    return scratch.data_ptr(), scratch.numel() * scratch.element_size()


def merkle_level(children_t, arity: int, tag_mont: int, out_idx: int = 1, pad=None):
    """One tree level: parent = perm([tag, c_0 .. c_{arity-1}, 0 ..])[out_idx], arity 1..4.  A ragged level (child
    count not a multiple of the arity) takes ``pad`` (one 32-byte digest on the device; None = zero) for the missing
    children."""
    if arity not in (1, 2, 3, 4):
        raise ValueError("merkle_level: arity must be 1..4")
    ptr, n_children, dev = _dev_buffer(children_t, 32, "merkle_level")
    parents = _dev_empty(dev, -(-n_children // arity), 4)
    _dev_call("merkle_level", dev, "hades252_merkle_level_pad_dev", ptr, n_children, parents.data_ptr(), arity,
              _tag_arr(tag_mont), out_idx, _pad_ptr(pad, 1, "merkle_level"))
    return parents


def merkle_empty_digests(arity: int, depth: int, e0_mont: int, tag_mont: int, out_idx: int = 1, device="cuda"):
    """The padding table of empty subtrees: [depth, 4] int64 -- pad[0] = e0, pad[l+1] = parent of `arity` x pad[l]."""
    pad = _dev_empty(device, depth, 4)
    _dev_call("merkle_empty_digests", pad.device, "hades252_merkle_empty_digests_dev", arity, depth, _tag_arr(e0_mont),
              _tag_arr(tag_mont), out_idx, pad.data_ptr())
    return pad


def merkle_root(leaves_t, arity: int, tag_mont: int, out_idx: int = 1, scratch=None, pad=None):
    """Root of the arity-`arity` tree over ``leaves_t`` (n_leaves x 32 B; any n_leaves >= 2, arity 2..4)."""
    ptr, n, dev = _dev_buffer(leaves_t, 32, "merkle_root")
    depth = merkle_depth(n, arity, "merkle_root")
    sptr, sbytes = _dev_scratch(dev, scratch, _lib.lib().hades252_merkle_scratch_bytes(n, arity))
    root = _dev_empty(dev, 4)
    _dev_call("merkle_root", dev, "hades252_merkle_root_pad_dev", ptr, n, arity, sptr, sbytes, _tag_arr(tag_mont), out_idx,
              _pad_ptr(pad, depth, "merkle_root"), root.data_ptr())
    return root


def merkle_build(leaves_t, arity: int, tag_mont: int, out_idx: int = 1, pad=None):
    """Every level of the tree: [n_1 + n_2 + ... + 1, 4] int64 -- level 1 first, the root last."""
    ptr, n, dev = _dev_buffer(leaves_t, 32, "merkle_build")
    depth = merkle_depth(n, arity, "merkle_build")
    tree = _dev_empty(dev, sum(merkle_level_sizes(n, arity)), 4)
    _dev_call("merkle_build", dev, "hades252_merkle_build_pad_dev", ptr, n, arity, _tag_arr(tag_mont), out_idx,
              _pad_ptr(pad, depth, "merkle_build"), tree.data_ptr())
    return tree


def merkle_open(leaves_t, tree_t, arity: int, indices_t, pad=None):
    """Authentication paths: [n_queries, depth, arity-1, 4] int64 (siblings in child order, the path node's
    own position (index // arity^l) % arity skipped; positions past the end of a level read pad[l])."""
    ptr, n, dev = _dev_buffer(leaves_t, 32, "merkle_open")
    depth = merkle_depth(n, arity, "merkle_open")
    tptr = _tree_of("merkle_open", tree_t, n, arity)
    iptr, nq, _ = _dev_buffer(indices_t, 8, "merkle_open")
    if nq and int(indices_t.max().item()) >= n:
        raise IndexError("merkle_open: leaf index out of range")
    paths = _dev_empty(dev, nq, depth, arity - 1, 4)
    _dev_call("merkle_open", dev, "hades252_merkle_open_pad_dev", ptr, tptr, n, arity, iptr, nq,
              _pad_ptr(pad, depth, "merkle_open"), paths.data_ptr())
    return paths


def merkle_verify(leaf_values_t, indices_t, paths_t, arity: int, tag_mont: int, out_idx: int = 1):
    """Roots recomputed from (leaf value, index, opening) per query: [n_queries, 4] int64."""
    lptr, nq, dev = _dev_buffer(leaf_values_t, 32, "merkle_verify")
    iptr, nq2, _ = _dev_buffer(indices_t, 8, "merkle_verify")
    if nq2 != nq or paths_t.shape[0] != nq:
        raise ValueError("merkle_verify: leaves, indices and paths differ in count")
    depth = int(paths_t.shape[1])
    pptr = paths_t.data_ptr() if paths_t.numel() else 0
    roots = _dev_empty(dev, nq, 4)
    _dev_call("merkle_verify", dev, "hades252_merkle_verify_dev", lptr, iptr, pptr, nq, depth, arity, _tag_arr(tag_mont), out_idx,
              roots.data_ptr())
    return roots


def merkle_update(leaves_t, tree_t, arity: int, indices_t, tag_mont: int, out_idx: int = 1, pad=None):
    """Re-hash, in place in ``tree_t``, the ancestors of the leaves named by ``indices_t`` (device int64/uint64) after the
    caller has overwritten those rows of ``leaves_t``: depth x n_updates permutations instead of the whole tree."""
    ptr, n, dev = _dev_buffer(leaves_t, 32, "merkle_update")
    depth = merkle_depth(n, arity, "merkle_update")
    tptr = _tree_of("merkle_update", tree_t, n, arity)
    iptr, nq, _ = _dev_buffer(indices_t, 8, "merkle_update")
    _dev_call("merkle_update", dev, "hades252_merkle_update_dev", ptr, tptr, n, arity, _tag_arr(tag_mont), out_idx,
              _pad_ptr(pad, depth, "merkle_update"), iptr, nq)
    return tree_t


def merkle_forest(leaves_t, n_trees: int, arity: int, tag_mont: int, out_idx: int = 1, scratch=None):
    """Roots of n_trees equal trees (leaves contiguous, tree after tree; leaves per tree a power of the arity)."""
    ptr, n, dev = _dev_buffer(leaves_t, 32, "merkle_forest")
    if n_trees <= 0 or n % n_trees:
        raise ValueError("merkle_forest: %d leaves do not split into %d trees" % (n, n_trees))
    per = n // n_trees
    sptr, sbytes = _dev_scratch(dev, scratch, _lib.lib().hades252_merkle_forest_scratch_bytes(n_trees, per, arity))
    roots = _dev_empty(dev, n_trees, 4)
    _dev_call("merkle_forest", dev, "hades252_merkle_forest_dev", ptr, n_trees, per, arity, sptr, sbytes, _tag_arr(tag_mont),
              out_idx, roots.data_ptr())
    return roots


def merkle4_level(children_t, tag_mont: int, out_idx: int = 1):
    return merkle_level(children_t, 4, tag_mont, out_idx)


def merkle4_root(leaves_t, tag_mont: int, out_idx: int = 1, scratch=None):
    """Root of the arity-4 tree over ``leaves_t`` (BASELINE config 4)."""
    return merkle_root(leaves_t, 4, tag_mont, out_idx, scratch)


def sponge_hash(msgs_t, msg_len: int, capacity_mont: int, pad_mode: int = 1):
    """Batched fixed-length sponge (include/hades252.h): msgs_t holds n messages of msg_len
    scalars; returns [n, 4] int64 digests (word 1 of the final state)."""
    if msg_len <= 0:
        raise ValueError("sponge_hash: msg_len must be positive for a tensor batch")
    ptr, n, dev = _dev_messages("sponge_hash", msgs_t, msg_len)
    out = _dev_empty(dev, n, 4)
    _dev_call("sponge_hash", dev, "hades252_sponge_hash_dev", ptr, n, msg_len, _tag_arr(capacity_mont), pad_mode, out.data_ptr())
    return out


def sponge_hash_var(scalars_t, offsets_t, lengths_t, capacity_mont: int, pad_mode: int = 1, sort: bool = False):
    """Batched variable-length sponge: message i = scalars[offsets[i] : offsets[i] + lengths[i]]
    (offsets / lengths: int64 CUDA tensors, in scalars).  Returns [n, 4] int64 digests.  ``sort``: order the messages
    by block count on the device first (ragged batches: the 64 messages of a wave then need the same number of
    permutations); same digests."""
    sptr, n_scalars, dev = _dev_buffer(scalars_t, 32, "sponge_hash_var")
    optr, n, _ = _dev_buffer(offsets_t, 8, "sponge_hash_var")
    lptr, n2, _ = _dev_buffer(lengths_t, 8, "sponge_hash_var")
    if n != n2:
        raise ValueError("sponge_hash_var: offsets and lengths differ in size")
    out = _dev_empty(dev, n, 4)
    bad = _dev_counter(dev)
    scratch, sbytes = None, 0
    if sort:
        sbytes = _lib.lib().hades252_sponge_sort_scratch_bytes(n)
        scratch = _dev_empty(dev, (sbytes + 15) // 16 * 2)
    _dev_call("sponge_hash_var", dev, "hades252_sponge_hash_var_ex_dev", sptr, n_scalars, optr, lptr, n, _tag_arr(capacity_mont),
              pad_mode, out.data_ptr(), bad.data_ptr(), scratch.data_ptr() if sort else 0, sbytes)
    if int(bad.item()) != 0:
        raise IndexError("sponge_hash_var: %d message(s) reach outside the scalar pool" % int(bad.item()))
    return out


# Named, NOT pinned parameter sets (dusk-poseidon is outside the reference tree, README.md:9): include/hades252.h
SPONGE_PRESETS = {"sponge/pad10": {"capacity": 1 << 64, "pad_mode": 1, "digest_word": 1},
                  "merkle/arity4": {"tag": 15, "arity": 4, "digest_word": 1}}


def _resident_states(where: str, n: int, word0_mont: int, device):
    """n sponge states [n, 5, 4] on ``device``, word 0 set (``hades252_sponge_init_dev``)."""
    states = _dev_empty(device, n, WIDTH, 4)
    _dev_call(where, states.device, "hades252_sponge_init_dev", states.data_ptr(), n, _tag_arr(word0_mont))
    return states


class SpongeStates:
    """Streaming sponge (``hades252_sponge_init_dev`` / ``_absorb_dev`` / ``_squeeze_dev``): n states resident on the
    device; absorb blocks of 4 scalars whenever they arrive, squeeze when done."""

    def __init__(self, n: int, capacity_mont: int, device="cuda"):
        self.states = _resident_states("sponge_init", n, capacity_mont, device)

    def absorb(self, blocks_t) -> None:
        """blocks_t: [n, blocks_each, 4 scalars] (any shape with n * blocks_each * 128 bytes, state-major)."""
        n = self.states.shape[0]
        ptr, n_blocks, dev = _dev_buffer(blocks_t, 128, "sponge_absorb")
        if n == 0 or n_blocks % n:
            raise ValueError("sponge_absorb: %d blocks do not split evenly over %d states" % (n_blocks, n))
        _dev_call("sponge_absorb", dev, "hades252_sponge_absorb_dev", self.states.data_ptr(), ptr, n, n_blocks // n)

    def squeeze(self, word: int = 1):
        n, dev = self.states.shape[0], self.states.device
        out = _dev_empty(dev, n, 4)
        _dev_call("sponge_squeeze", dev, "hades252_sponge_squeeze_dev", self.states.data_ptr(), out.data_ptr(), n, word)
        return out


# ---- batched Poseidon cipher (include/hades252.h, CONVENTION UNPINNED) -----------------------------------------------
_FR_P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
# dusk-poseidon's domain word: BlsScalar::from_raw([0x1_0000_0000, 0, 0, 0]) = 2^32, in Montgomery form (R = 2^256)
CIPHER_DOMAIN = (1 << 32) * (1 << 256) % _FR_P


def _same_device(what: str, dev, *others) -> None:
    for d in others:
        if d != dev:
            raise ValueError("%s: every tensor must be on %s (got one on %s)" % (what, dev, d))


def _cipher_shapes(what: str, msg_len: int, decrypt: bool, words_units: int, keys_units: int, nonces_units: int) -> int:
    """The shape rules of the cipher, host and device: -> n messages.  The words are n messages of msg_len scalars
    (encrypt) or n ciphers of msg_len + 1 (decrypt)."""
    if not 1 <= msg_len <= _lib.CIPHER_MAX_LEN:
        raise ValueError("%s: msg_len must be in 1 .. %d (got %d)" % (what, _lib.CIPHER_MAX_LEN, msg_len))
    if keys_units != 2 * nonces_units:
        raise ValueError("%s: %d key scalars for %d nonces (two per message)" % (what, keys_units, nonces_units))
    each = msg_len + 1 if decrypt else msg_len
    if words_units != nonces_units * each:
        raise ValueError("%s: buffer is not %d %s of %d scalars" % (what, nonces_units, "ciphers" if decrypt else "messages", each))
    return nonces_units


def _cipher_front(what: str, words_t, keys_t, nonces_t, msg_len: int, decrypt: bool):
    """The arguments the four device calls of the cipher share: -> ((words, keys, nonces) pointers, n, device)."""
    kptr, n_keys, dev = _dev_buffer(keys_t, 32, what)
    nptr, n_nonces, ndev = _dev_buffer(nonces_t, 32, what)
    wptr, n_words, wdev = _dev_buffer(words_t, 32, what)
    _same_device(what, dev, ndev, wdev)
    return (wptr, kptr, nptr), _cipher_shapes(what, msg_len, decrypt, n_words, n_keys, n_nonces), dev


def _decrypt_outputs(dev, n: int, msg_len: int):
    """(msgs [n, msg_len, 4], ok [n] uint8, rejected counter) of a decryption."""
    return _dev_empty(dev, n, msg_len, 4), _dev_empty(dev, n, dtype="uint8"), _dev_counter(dev)


def cipher_encrypt(msgs_t, keys_t, nonces_t, msg_len: int, domain_mont: int = CIPHER_DOMAIN):
    """Batched Poseidon cipher, encrypt (``hades252_cipher_encrypt_dev``): msgs_t holds n messages of msg_len scalars,
    keys_t n x 2 scalars, nonces_t n scalars (CUDA tensors, Montgomery limbs).  Returns [n, msg_len + 1, 4] int64: the
    cipher words, the tag last."""
    ptrs, n, dev = _cipher_front("cipher_encrypt", msgs_t, keys_t, nonces_t, msg_len, False)
    out = _dev_empty(dev, n, msg_len + 1, 4)
    _dev_call("cipher_encrypt", dev, "hades252_cipher_encrypt_dev", *ptrs, n, msg_len, _tag_arr(domain_mont), out.data_ptr())
    return out


def cipher_decrypt(ciphers_t, keys_t, nonces_t, msg_len: int, domain_mont: int = CIPHER_DOMAIN):
    """Batched Poseidon cipher, decrypt (``hades252_cipher_decrypt_dev``): ciphers_t holds n x (msg_len + 1) scalars.
    Returns (msgs [n, msg_len, 4] int64, ok [n] uint8, n_rejected); a rejected message (wrong tag, or a cipher word that
    is not canonical) comes out as zeros.  n_rejected synchronises with the device."""
    ptrs, n, dev = _cipher_front("cipher_decrypt", ciphers_t, keys_t, nonces_t, msg_len, True)
    out, ok, rej = _decrypt_outputs(dev, n, msg_len)
    _dev_call("cipher_decrypt", dev, "hades252_cipher_decrypt_dev", *ptrs, n, msg_len, _tag_arr(domain_mont), out.data_ptr(),
              ok.data_ptr(), rej.data_ptr())
    return out, ok, int(rej.item())


def cipher_perms(msg_len: int) -> int:
    """Permutations per message of the cipher (``hades252_cipher_perms``): ceil(msg_len / 4) + 1."""
    if not 1 <= msg_len <= _lib.CIPHER_MAX_LEN:
        raise ValueError("cipher_perms: msg_len must be in 1 .. %d (got %d)" % (_lib.CIPHER_MAX_LEN, msg_len))
    return int(_lib.lib().hades252_cipher_perms(msg_len))


def cipher_encrypt_witness(msgs_t, keys_t, nonces_t, msg_len: int, domain_mont: int = CIPHER_DOMAIN):
    """Gadget witness of the cipher, encrypt (``hades252_cipher_encrypt_witness_dev``; the arguments of ``cipher_encrypt``).
    Returns (wires [972, S, n, 4], inputs [S, n, 5, 4], ciphers [n, msg_len + 1, 4]) with S = cipher_perms(msg_len):
    inputs[s, i] enters permutation s of message i, wires.reshape(972, S * n, 4) == perm_witness(inputs) byte for byte,
    and the ciphers are those of ``cipher_encrypt``."""
    ptrs, n, dev = _cipher_front("cipher_encrypt_witness", msgs_t, keys_t, nonces_t, msg_len, False)
    wires, inputs = _witness_pair(dev, cipher_perms(msg_len), n)
    out = _dev_empty(dev, n, msg_len + 1, 4)
    _dev_call("cipher_encrypt_witness", dev, "hades252_cipher_encrypt_witness_dev", *ptrs, n, msg_len, _tag_arr(domain_mont),
              inputs.data_ptr(), wires.data_ptr(), out.data_ptr())
    return wires, inputs, out


def cipher_decrypt_witness(ciphers_t, keys_t, nonces_t, msg_len: int, domain_mont: int = CIPHER_DOMAIN):
    """Gadget witness of the cipher, decrypt (``hades252_cipher_decrypt_witness_dev``; the arguments of ``cipher_decrypt``).
    Returns (wires [972, S, n, 4], inputs [S, n, 5, 4], msgs [n, msg_len, 4], ok [n] uint8, n_rejected): the inputs carry
    the cipher words reduced mod p, so they are canonical for every message; msgs, ok and n_rejected are those of
    ``cipher_decrypt``.  n_rejected synchronises with the device."""
    ptrs, n, dev = _cipher_front("cipher_decrypt_witness", ciphers_t, keys_t, nonces_t, msg_len, True)
    wires, inputs = _witness_pair(dev, cipher_perms(msg_len), n)
    out, ok, rej = _decrypt_outputs(dev, n, msg_len)
    _dev_call("cipher_decrypt_witness", dev, "hades252_cipher_decrypt_witness_dev", *ptrs, n, msg_len, _tag_arr(domain_mont),
              inputs.data_ptr(), wires.data_ptr(), out.data_ptr(), ok.data_ptr(), rej.data_ptr())
    return wires, inputs, out, ok, int(rej.item())


def _cipher_host_front(what: str, words, keys, nonces, msg_len: int, decrypt: bool) -> int:
    return _cipher_shapes(what, msg_len, decrypt, *[_host_units(a, what) for a in (words, keys, nonces)])


def cipher_encrypt_host(msgs: np.ndarray, keys: np.ndarray, nonces: np.ndarray, msg_len: int,
                        domain_mont: int = CIPHER_DOMAIN) -> np.ndarray:
    """``hades252_cipher_encrypt`` on HOST arrays (C-contiguous uint64, Montgomery limbs): -> [n, msg_len + 1, 4] uint64."""
    n = _cipher_host_front("cipher_encrypt_host", msgs, keys, nonces, msg_len, False)
    out = np.zeros((n, msg_len + 1, 4), dtype=np.uint64)
    check(_lib.lib().hades252_cipher_encrypt(_ptr(msgs), _ptr(keys), _ptr(nonces), n, msg_len, _tag_arr(domain_mont),
                                             _ptr(out)), "cipher_encrypt_host")
    return out


def cipher_decrypt_host(ciphers: np.ndarray, keys: np.ndarray, nonces: np.ndarray, msg_len: int,
                        domain_mont: int = CIPHER_DOMAIN):
    """``hades252_cipher_decrypt`` on HOST arrays: -> (msgs [n, msg_len, 4] uint64, ok [n] uint8, n_rejected)."""
    n = _cipher_host_front("cipher_decrypt_host", ciphers, keys, nonces, msg_len, True)
    out = np.zeros((n, msg_len, 4), dtype=np.uint64)
    ok = np.zeros(n, dtype=np.uint8)
    rej = ctypes.c_size_t(0)
    check(_lib.lib().hades252_cipher_decrypt(_ptr(ciphers), _ptr(keys), _ptr(nonces), n, msg_len, _tag_arr(domain_mont),
                                             _ptr(out), _ptr(ok), ctypes.byref(rej)), "cipher_decrypt_host")
    return out, ok, int(rej.value)


# ---- batched duplex sponge (include/hades252.h, CONVENTION UNPINNED) ---------------------------------------------------
_SAFE_KINDS = {"absorb": _lib.SAFE_ABSORB, "squeeze": 0}


def _safe_calls(pattern, what: str):
    """[("absorb", 3), ("squeeze", 2)] -> (ctypes uint32 array, count); the library judges validity."""
    words = []
    for call in pattern:
        kind, n = call
        if kind not in _SAFE_KINDS or not isinstance(n, int) or not 0 <= n < _lib.SAFE_ABSORB:
            raise ValueError("%s: a call is (\"absorb\" | \"squeeze\", length), got %r" % (what, (call,)))
        words.append(_SAFE_KINDS[kind] | n)
    return (ctypes.c_uint32 * max(len(words), 1))(*words), len(words)


def safe_pattern(calls):
    """Validate an IO pattern (``hades252_safe_pattern``; no device needed) -> (words absorbed, words squeezed, permutations)
    per sponge.  Raises ValueError for an invalid pattern."""
    arr, k = _safe_calls(calls, "safe_pattern")
    n_in, n_out, n_perms = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    if _lib.lib().hades252_safe_pattern(arr, k, ctypes.byref(n_in), ctypes.byref(n_out), ctypes.byref(n_perms)) != _lib.OK:
        raise ValueError("safe_pattern: %r is not a valid IO pattern (absorb first, squeeze last, no empty call, at most %d "
                         "calls and %d words each way)" % (list(calls), _lib.SAFE_MAX_CALLS, _lib.SAFE_MAX_WORDS))
    return int(n_in.value), int(n_out.value), int(n_perms.value)


def _aggregate(pattern):
    """A valid pattern with neighbouring calls of one kind merged: [[kind, words], ...]."""
    calls = []
    for kind, n in pattern:
        if calls and calls[-1][0] == kind:
            calls[-1][1] += n
        else:
            calls.append([kind, n])
    return calls


def safe_tag_input(pattern, domain_sep: int) -> bytes:
    """The bytes SAFE hashes into a tag: the aggregated calls as big-endian 32-bit words, then the 64-bit domain separator
    big-endian.  NAMED, NOT PINNED (like SPONGE_PRESETS); hashing them to a scalar stays the caller's."""
    safe_pattern(pattern)
    return b"".join((_SAFE_KINDS[kind] | n).to_bytes(4, "big") for kind, n in _aggregate(pattern)) + \
        int(domain_sep).to_bytes(8, "big")


def _safe_front(what: str, pattern):
    """What the three whole-pattern calls share: -> (the pattern as the library takes it (array, count), words absorbed,
    words squeezed, permutations), each per sponge."""
    n_in, n_out, n_perms = safe_pattern(pattern)
    return _safe_calls(pattern, what), n_in, n_out, n_perms


def _whole_inputs(what: str, n_words: int, n_in: int) -> int:
    """How many sponges n_words scalars feed, n_in each."""
    if n_words % n_in:
        raise ValueError("%s: %d scalars are not a whole number of inputs of %d" % (what, n_words, n_in))
    return n_words // n_in


def safe_hash(inputs_t, pattern, tag_mont: int):
    """Batched duplex sponge, the whole pattern in one launch (``hades252_safe_hash_dev``): inputs_t holds n x n_in scalars
    (CUDA tensor, Montgomery limbs, message-major, in call order).  Returns [n, n_out, 4] int64."""
    calls, n_in, n_out, _ = _safe_front("safe_hash", pattern)
    ptr, n_words, dev = _dev_buffer(inputs_t, 32, "safe_hash")
    n = _whole_inputs("safe_hash", n_words, n_in)
    out = _dev_empty(dev, n, n_out, 4)
    _dev_call("safe_hash", dev, "hades252_safe_hash_dev", ptr, n, *calls, _tag_arr(tag_mont), out.data_ptr())
    return out


def safe_hash_host(inputs: np.ndarray, pattern, tag_mont: int) -> np.ndarray:
    """``hades252_safe_hash`` on a HOST array (C-contiguous uint64, Montgomery limbs): -> [n, n_out, 4] uint64."""
    calls, n_in, n_out, _ = _safe_front("safe_hash_host", pattern)
    n = _whole_inputs("safe_hash_host", _host_units(inputs, "safe_hash_host"), n_in)
    out = np.zeros((n, n_out, 4), dtype=np.uint64)
    check(_lib.lib().hades252_safe_hash(_ptr(inputs), n, *calls, _tag_arr(tag_mont), _ptr(out)), "safe_hash_host")
    return out


class SafeSponge:
    """n duplex sponges resident on the device that follow one IO pattern call by call (``hades252_safe_absorb_dev`` /
    ``_squeeze_dev``), for callers whose next input depends on what they read.  Calls may be split (absorb(2) then
    absorb(1) serves ("absorb", 3)); a call of the wrong kind, one that overruns the pattern's current call, or ``finish``
    before the pattern is used up raises ValueError: the analogue of dusk-safe's IO-pattern violation."""
    _NAME = "SafeSponge"

    def __init__(self, n: int, pattern, tag_mont: int, device="cuda"):
        safe_pattern(pattern)
        self._todo = _aggregate(pattern)                  # aggregated calls still to serve: [kind, words left]
        self._cursor = ctypes.c_uint32(0)
        self.states = _resident_states("SafeSponge", n, tag_mont, device)

    def _take(self, kind: str, k: int) -> None:
        if k <= 0:
            raise ValueError("SafeSponge.%s: a call moves at least one word" % kind)
        if not self._todo:
            raise ValueError("SafeSponge.%s: the IO pattern is used up" % kind)
        if self._todo[0][0] != kind:
            raise ValueError("SafeSponge.%s: the IO pattern expects %s(%d) here" % (kind, self._todo[0][0], self._todo[0][1]))
        if k > self._todo[0][1]:
            raise ValueError("SafeSponge.%s: %d words, the IO pattern has %d left in this call" % (kind, k, self._todo[0][1]))

    def _took(self, k: int) -> None:
        self._todo[0][1] -= k
        if self._todo[0][1] == 0:
            self._todo.pop(0)

    def _run(self, kind: str, k: int, *args) -> None:
        """The library call that serves k words of the current call (``_take`` has agreed to them; ``args``: what the
        library takes between the sponge count and the pattern cursor), then ticks them off."""
        self._lib_call(kind, self.states.data_ptr(), self.states.shape[0], *args, ctypes.byref(self._cursor))
        self._took(k)

    def _lib_call(self, kind: str, *args) -> None:
        _dev_call("%s.%s" % (self._NAME, kind), self.states.device, "hades252_safe_%s_dev" % kind, *args)

    def absorb(self, t) -> None:
        """t: n x k scalars (state-major) for the next k words of the current absorb call."""
        where = self._NAME + ".absorb"
        n = self.states.shape[0]
        ptr, n_words, dev = _dev_buffer(t, 32, where)
        _same_device(where, self.states.device, dev)
        if n == 0 or n_words % n:
            raise ValueError("%s: %d scalars do not split evenly over %d sponges" % (where, n_words, n))
        k = n_words // n
        self._take("absorb", k)
        self._run("absorb", k, ptr, k)

    def squeeze(self, k: int):
        """-> [n, k, 4] int64: the next k words of the current squeeze call."""
        self._take("squeeze", k)
        out = _dev_empty(self.states.device, self.states.shape[0], k, 4)
        self._run("squeeze", k, k, out.data_ptr())
        return out

    def finish(self) -> None:
        """The pattern must be used up (dusk-safe's `finish`)."""
        if self._todo:
            raise ValueError("SafeSponge.finish: the IO pattern still expects %s(%d)" % tuple(self._todo[0]))


def safe_witness(inputs_t, pattern, tag_mont: int):
    """Gadget witness of the duplex sponge, the whole pattern in one launch (``hades252_safe_witness_dev``; the arguments of
    ``safe_hash``).  Returns (wires [972, S, n, 4], inputs [S, n, 5, 4], out [n, n_out, 4]) with S the pattern's
    permutations per sponge: inputs[s, i] enters permutation s of sponge i, wires.reshape(972, S * n, 4) ==
    perm_witness(inputs) byte for byte, and out is what ``safe_hash`` returns."""
    calls, n_in, n_out, S = _safe_front("safe_witness", pattern)
    ptr, n_words, dev = _dev_buffer(inputs_t, 32, "safe_witness")
    n = _whole_inputs("safe_witness", n_words, n_in)
    wires, inputs = _witness_pair(dev, S, n)
    out = _dev_empty(dev, n, n_out, 4)
    _dev_call("safe_witness", dev, "hades252_safe_witness_dev", ptr, n, *calls, _tag_arr(tag_mont), inputs.data_ptr(),
              wires.data_ptr(), out.data_ptr())
    return wires, inputs, out


class SafeWitnessSponge(SafeSponge):
    """A ``SafeSponge`` that also records the permutations its calls run (``hades252_safe_absorb_witness_dev`` /
    ``_squeeze_witness_dev``): it owns the two record buffers, sized for the pattern's S permutations per sponge, and the
    step counter.  After ``finish`` (which also demands that all S steps were recorded) ``wires`` [972, S, n, 4] and
    ``inputs`` [S, n, 5, 4] hold what ``safe_witness`` returns for the same words."""
    _NAME = "SafeWitnessSponge"

    def __init__(self, n: int, pattern, tag_mont: int, device="cuda"):
        super().__init__(n, pattern, tag_mont, device)
        self._steps = safe_pattern(pattern)[2]
        self._step = ctypes.c_size_t(0)
        self._wires, self._inputs = _witness_pair(self.states.device, self._steps, n)
        self._finished = False

    def _lib_call(self, kind: str, *args) -> None:
        _dev_call("%s.%s" % (self._NAME, kind), self.states.device, "hades252_safe_%s_witness_dev" % kind, *args,
                  self._inputs.data_ptr(), self._wires.data_ptr(), self._steps, ctypes.byref(self._step))

    def finish(self) -> None:
        """The pattern must be used up; ``wires`` and ``inputs`` are readable afterwards."""
        super().finish()
        if self.states.shape[0] != 0 and self._step.value != self._steps:
            raise ValueError("SafeWitnessSponge.finish: %d of %d steps recorded" % (self._step.value, self._steps))
        self._finished = True

    def _records(self, t):
        if not self._finished:
            raise ValueError("SafeWitnessSponge: the records are complete after finish() only")
        return t

    @property
    def wires(self):
        return self._records(self._wires)

    @property
    def inputs(self):
        return self._records(self._inputs)


# ---- proof-of-work grinding (include/hades252.h, CONVENTION UNPINNED: tests/grind_model.py) -----------------------------
def grind_target(bits: int) -> int:
    """The target that asks for `bits` bits of work: p >> bits (a digest is uniform below p, so one nonce in 2^bits hits)."""
    if not isinstance(bits, int) or bits < 0:
        raise ValueError("grind_target: bits must be a non-negative integer, got %r" % (bits,))
    return _FR_P >> bits


def grind(seeds: np.ndarray, word: int, out_idx: int, target: int, first_nonce: int = 0, max_nonces: int = 1 << 32):
    """``hades252_grind``: per job (seeds[j]: five scalars, Montgomery limbs, HOST numpy uint64 [n, 5, 4]) the smallest nonce
    x in [first_nonce, first_nonce + max_nonces) for which word ``out_idx`` of perm(seed with seed[word] + x) is, as a
    canonical integer, strictly below ``target`` (a Python int below 2^256).  -> (nonces uint64 [n], found bool [n]);
    nonces[j] is 0 where found[j] is False."""
    n = _host_u64(seeds, "grind", (WIDTH, 4)).shape[0]
    for name, v in (("word", word), ("out_idx", out_idx)):
        if not isinstance(v, int) or not 0 <= v < WIDTH:
            raise ValueError("grind: %s must be 0 .. %d, got %r" % (name, WIDTH - 1, v))
    if not isinstance(target, int) or not 0 <= target < 1 << 256:
        raise ValueError("grind: the target is an integer in [0, 2^256), got %r" % (target,))
    if not isinstance(first_nonce, int) or not isinstance(max_nonces, int) or first_nonce < 0 or max_nonces < 0 or \
            first_nonce + max_nonces > 1 << 64 or max_nonces >= 1 << 64:
        raise ValueError("grind: the nonce range [%r, %r + %r) does not lie in [0, 2^64)" % (first_nonce, first_nonce, max_nonces))
    if n > _lib.GRIND_MAX_JOBS:
        raise ValueError("grind: at most %d jobs per call, got %d" % (_lib.GRIND_MAX_JOBS, n))
    nonces = np.zeros(n, dtype=np.uint64)
    found = np.zeros(n, dtype=np.uint8)
    check(_lib.lib().hades252_grind(_ptr(seeds), n, word, out_idx, _tag_arr(target), first_nonce, max_nonces, _ptr(nonces),
                                    _ptr(found)), "grind")
    return nonces, found.astype(bool)


def perm_inverse_rounds(states: np.ndarray, round_hi: int, round_lo: int) -> np.ndarray:
    """``hades252_perm_inverse_rounds``: rounds round_hi - 1, ..., round_lo of the permutation undone on HOST numpy uint64
    states [n, 5, 4] (Montgomery limbs): the state after round round_hi - 1 in, the state after round round_lo - 1 (the
    permutation's input for round_lo = 0) out, as a new array."""
    out = _host_u64(states, "perm_inverse_rounds", (WIDTH, 4)).copy()
    for v in (round_hi, round_lo):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError("perm_inverse_rounds: a round number is an int, got %r" % (v,))
    if not 0 <= round_lo <= round_hi <= ROUNDS_TOTAL:
        raise ValueError("perm_inverse_rounds: 0 <= round_lo <= round_hi <= %d, got (%r, %r)" % (ROUNDS_TOTAL, round_hi, round_lo))
    check(_lib.lib().hades252_perm_inverse_rounds(_ptr(out), out.shape[0], round_hi, round_lo), "perm_inverse_rounds")
    return out


def perm_inverse(states: np.ndarray) -> np.ndarray:
    """``hades252_perm_inverse_batch``: the preimages of HOST numpy uint64 states [n, 5, 4] under the permutation, as a new
    array: perm(perm_inverse(y)) == y."""
    out = _host_u64(states, "perm_inverse", (WIDTH, 4)).copy()
    check(_lib.lib().hades252_perm_inverse_batch(_ptr(out), out.shape[0]), "perm_inverse")
    return out


def fifth_root(scalars: np.ndarray) -> np.ndarray:
    """``hades252_fifth_root_batch``: x -> x^(1/5) on HOST numpy uint64 scalars [n, 4] (Montgomery limbs), as a new array: the
    inverse of quintic_s_box on independent scalars."""
    out = _host_u64(scalars, "fifth_root", (4,)).copy()
    check(_lib.lib().hades252_fifth_root_batch(_ptr(out), out.shape[0]), "fifth_root")
    return out


def _planes_shape(where: str, planes):
    """Type, contiguity and shape of columns [n_cols, plane_stride, 4] of a column-major matrix; -> (n_cols, plane_stride)."""
    planes = _host_u64(planes, where)
    if planes.ndim != 3 or planes.shape[2] != 4:
        raise ValueError("%s: planes must have shape [n_cols, plane_stride, 4], got %r" % (where, planes.shape))
    return planes.shape[0], planes.shape[1]


def _matrix_planes(where: str, planes, n_rows):
    """A whole column-major matrix and the rows of it that count; -> (n_rows, n_cols, plane_stride)."""
    n_cols, stride = _planes_shape(where, planes)
    if not 1 <= n_cols <= _lib.MATRIX_MAX_COLS:
        raise ValueError("%s: 1 .. %d columns, got %d" % (where, _lib.MATRIX_MAX_COLS, n_cols))
    if n_rows is None:
        n_rows = stride
    if not isinstance(n_rows, int) or isinstance(n_rows, bool) or not 0 <= n_rows <= stride:
        raise ValueError("%s: n_rows must be 0 .. plane_stride = %d, got %r" % (where, stride, n_rows))
    return n_rows, n_cols, stride


def _matrix_tree_shape(where: str, n_rows: int, arity: int):
    """(depth, digests in the tree) of the tree over n_rows leaves, without the library."""
    if not isinstance(arity, int) or isinstance(arity, bool) or not 2 <= arity <= 4 or n_rows < 2:
        raise ValueError("%s: need arity 2..4 and at least 2 rows (got arity %r, %d rows)" % (where, arity, n_rows))
    sizes = merkle_level_sizes(n_rows, arity)
    return len(sizes), sum(sizes)


def _matrix_modes(where: str, pad_mode, out_idx=1):
    if pad_mode not in (0, 1) or isinstance(pad_mode, bool):
        raise ValueError("%s: pad_mode is 0 or 1, got %r" % (where, pad_mode))
    if not isinstance(out_idx, int) or isinstance(out_idx, bool) or not 0 <= out_idx < WIDTH:
        raise ValueError("%s: out_idx must be 0 .. %d, got %r" % (where, WIDTH - 1, out_idx))


def _commit_outputs(n_rows: int, nodes: int, want_digests: bool, want_tree: bool):
    """What a commit call fills and returns: -> ((digests [n_rows, 4] or None, tree [nodes, 4] or None, root [4]), their
    pointers)."""
    outs = (np.zeros((n_rows, 4), dtype=np.uint64) if want_digests else None,
            np.zeros((nodes, 4), dtype=np.uint64) if want_tree else None, np.zeros(4, dtype=np.uint64))
    return outs, [None if a is None else _ptr(a) for a in outs]


def matrix_row_digests_host(planes: np.ndarray, capacity_mont: int, pad_mode: int = 1, n_rows: int | None = None) -> np.ndarray:
    """``hades252_matrix_row_digests``: the sponge digest [n_rows, 4] of every row of a matrix held column by column in HOST
    memory (numpy uint64 [n_cols, plane_stride, 4], Montgomery limbs; rows 0 .. n_rows - 1 of every plane, all of them by
    default): what sponge_hash_host gives for the transposed matrix."""
    n_rows, n_cols, stride = _matrix_planes("matrix_row_digests_host", planes, n_rows)
    _matrix_modes("matrix_row_digests_host", pad_mode)
    out = np.zeros((n_rows, 4), dtype=np.uint64)
    check(_lib.lib().hades252_matrix_row_digests(_ptr(planes), n_rows, n_cols, stride, _tag_arr(capacity_mont), pad_mode,
                                                 _ptr(out)), "matrix_row_digests_host")
    return out


def matrix_commit_host(planes: np.ndarray, capacity_mont: int, arity: int, tag_mont: int, pad_mode: int = 1, out_idx: int = 1,
                       pad: np.ndarray | None = None, n_rows: int | None = None, want_digests: bool = True,
                       want_tree: bool = True):
    """``hades252_matrix_commit``: (digests [n_rows, 4] or None, tree [nodes, 4] or None, root [4]) of the column-major matrix
    ``planes``: the row digests of matrix_row_digests_host under the tree merkle_build builds (``pad``: host table
    [depth, 4] or None), in one call; the digests stay on the device in between."""
    where = "matrix_commit_host"
    n_rows, n_cols, stride = _matrix_planes(where, planes, n_rows)
    depth, nodes = _matrix_tree_shape(where, n_rows, arity)
    _matrix_modes(where, pad_mode, out_idx)
    pptr = _host_pad(where, pad, depth)
    outs, out_ptrs = _commit_outputs(n_rows, nodes, want_digests, want_tree)
    check(_lib.lib().hades252_matrix_commit(_ptr(planes), n_rows, n_cols, stride, _tag_arr(capacity_mont), pad_mode, arity,
                                            _tag_arr(tag_mont), out_idx, pptr, *out_ptrs), where)
    return outs


def matrix_open_host(planes: np.ndarray, digests: np.ndarray, tree: np.ndarray, arity: int, indices,
                     pad: np.ndarray | None = None, n_rows: int | None = None):
    """``hades252_matrix_open``: (rows [q, n_cols, 4], paths [q, depth, arity - 1, 4]) for the row indices ``indices`` from what
    matrix_commit_host returned.  Plain host code: no device is touched.  An index >= n_rows gives zeros."""
    where = "matrix_open_host"
    n_rows, n_cols, stride = _matrix_planes(where, planes, n_rows)
    depth, nodes = _matrix_tree_shape(where, n_rows, arity)
    digests, tree = _host_u64(digests, where), _host_u64(tree, where)
    if digests.size != n_rows * 4 or tree.size != nodes * 4:
        raise ValueError("%s: need %d row digests and a tree of %d digests" % (where, n_rows, nodes))
    pptr = _host_pad(where, pad, depth)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    rows = np.zeros((idx.size, n_cols, 4), dtype=np.uint64)
    paths = np.zeros((idx.size, depth, arity - 1, 4), dtype=np.uint64)
    check(_lib.lib().hades252_matrix_open(_ptr(planes), n_rows, n_cols, stride, _ptr(digests), _ptr(tree), arity, pptr,
                                          _ptr(idx), idx.size, _ptr(rows), _ptr(paths)), where)
    return rows, paths


def matrix_verify_host(rows: np.ndarray, indices, paths: np.ndarray, arity: int, capacity_mont: int, tag_mont: int,
                       pad_mode: int = 1, out_idx: int = 1) -> np.ndarray:
    """``hades252_matrix_verify``: roots [q, 4] recomputed from opened rows [q, n_cols, 4], their indices and their paths
    [q, depth, arity - 1, 4] (what matrix_open_host returns); the caller compares them with the committed root."""
    where = "matrix_verify_host"
    rows, paths = _host_u64(rows, where), _host_u64(paths, where)
    if not isinstance(arity, int) or isinstance(arity, bool) or not 2 <= arity <= 4:
        raise ValueError("%s: arity 2..4, got %r" % (where, arity))
    if rows.ndim != 3 or rows.shape[2] != 4 or not 1 <= rows.shape[1] <= _lib.MATRIX_MAX_COLS:
        raise ValueError("%s: rows must have shape [q, n_cols, 4], got %r" % (where, rows.shape))
    q = rows.shape[0]
    if paths.ndim != 4 or paths.shape[0] != q or paths.shape[1] < 1 or paths.shape[2:] != (arity - 1, 4):
        raise ValueError("%s: paths must have shape [%d, depth, %d, 4], got %r" % (where, q, arity - 1, paths.shape))
    _matrix_modes(where, pad_mode, out_idx)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    if idx.size != q:
        raise ValueError("%s: %d indices for %d rows" % (where, idx.size, q))
    roots = np.zeros((q, 4), dtype=np.uint64)
    check(_lib.lib().hades252_matrix_verify(_ptr(rows), rows.shape[1], _ptr(idx), _ptr(paths), q, paths.shape[1], arity,
                                            _tag_arr(capacity_mont), pad_mode, _tag_arr(tag_mont), out_idx, _ptr(roots)), where)
    return roots


class MatrixStream:
    """``hades252_matstream_*``: a commitment to a column-major matrix of ``n_rows`` rows that arrives a group of columns at
    a time; the row sponges stay on the device between the calls.  After absorbs of g_1, ..., g_k columns, ``digests`` and
    ``commit`` give what matrix_row_digests_host / matrix_commit_host give for the concatenated matrix, and leave the stream
    as it is: it can go on absorbing, so every prefix can be committed to.  HOST numpy arrays in and out; a context manager::

        with MatrixStream(n_rows, capacity_mont) as ms:
            for group in groups:              # uint64 [g, plane_stride, 4], plane_stride >= n_rows
                ms.absorb(group)
            digests, tree, root = ms.commit(arity, tag_mont)
    """

    def __init__(self, n_rows: int, capacity_mont: int):
        self._h = None
        if not isinstance(n_rows, int) or isinstance(n_rows, bool) or not 1 <= n_rows <= 1 << 30:
            raise ValueError("MatrixStream: n_rows must be 1 .. 2^30, got %r" % (n_rows,))
        h = ctypes.c_void_p()
        check(_lib.lib().hades252_matstream_open(ctypes.byref(h), n_rows, _tag_arr(capacity_mont)), "MatrixStream")
        self._h, self.n_rows = h, n_rows

    def _handle(self, where: str):
        if self._h is None:
            raise ValueError("%s: the stream is closed" % where)
        return self._h

    def absorb(self, planes: np.ndarray, n_rows: int | None = None) -> "MatrixStream":
        """The next columns of every row: ``planes`` uint64 [g, plane_stride, 4] (Montgomery limbs), rows 0 .. n_rows - 1 of
        every plane.  ``n_rows``, when given, must be the stream's.  Synchronous; g = 0 is a no-op."""
        where = "MatrixStream.absorb"
        h = self._handle(where)
        n_cols, stride = _planes_shape(where, planes)
        if n_rows is not None and n_rows != self.n_rows:
            raise ValueError("%s: the stream has %d rows, got n_rows = %r" % (where, self.n_rows, n_rows))
        if stride < self.n_rows:
            raise ValueError("%s: planes of %d rows for a stream of %d" % (where, stride, self.n_rows))
        check(_lib.lib().hades252_matstream_absorb(h, _ptr(planes), n_cols, stride), where)
        return self

    @property
    def cols(self) -> int:
        """Columns absorbed so far."""
        h, n = self._handle("MatrixStream.cols"), ctypes.c_uint64()
        check(_lib.lib().hades252_matstream_cols(h, ctypes.byref(n)), "MatrixStream.cols")
        return int(n.value)

    def digests(self, pad_mode: int = 1) -> np.ndarray:
        """The row digests [n_rows, 4] of the columns absorbed so far; the stream is left as it is."""
        where = "MatrixStream.digests"
        h = self._handle(where)
        _matrix_modes(where, pad_mode)
        out = np.zeros((self.n_rows, 4), dtype=np.uint64)
        check(_lib.lib().hades252_matstream_digests(h, pad_mode, _ptr(out)), where)
        return out

    def commit(self, arity: int, tag_mont: int, pad_mode: int = 1, out_idx: int = 1, pad: np.ndarray | None = None,
               want_digests: bool = True, want_tree: bool = True):
        """(digests [n_rows, 4] or None, tree [nodes, 4] or None, root [4]) of the columns absorbed so far, as
        matrix_commit_host gives them (``pad``: host table [depth, 4] or None); the stream is left as it is."""
        where = "MatrixStream.commit"
        h = self._handle(where)
        depth, nodes = _matrix_tree_shape(where, self.n_rows, arity)
        _matrix_modes(where, pad_mode, out_idx)
        pptr = _host_pad(where, pad, depth)
        outs, out_ptrs = _commit_outputs(self.n_rows, nodes, want_digests, want_tree)
        check(_lib.lib().hades252_matstream_commit(h, pad_mode, arity, _tag_arr(tag_mont), out_idx, pptr, *out_ptrs), where)
        return outs

    def close(self) -> None:
        """Frees what the stream holds on the device; closing twice is fine."""
        h, self._h = self._h, None
        if h is not None:
            _lib.lib().hades252_matstream_close(h)

    def __enter__(self) -> "MatrixStream":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _mmcs_depth(where: str, max_rows, arity) -> int:
    """D of a tallest height ``max_rows`` = arity^D (D >= 1, at most 2^30 rows), without the library."""
    if not isinstance(arity, int) or isinstance(arity, bool) or not 2 <= arity <= 4:
        raise ValueError("%s: arity 2..4, got %r" % (where, arity))
    if not isinstance(max_rows, int) or isinstance(max_rows, bool) or not arity <= max_rows <= 1 << 30:
        raise ValueError("%s: the tallest height must be arity .. 2^30, got %r" % (where, max_rows))
    depth, n = 0, max_rows
    while n > 1:
        if n % arity:
            raise ValueError("%s: %d is not a power of the arity %d" % (where, max_rows, arity))
        n //= arity
        depth += 1
    return depth


def mmcs_tree_bytes(max_rows: int, arity: int) -> int:
    """``hades252_mmcs_tree_bytes``: bytes of the tree of a mixed-height commitment whose tallest group has ``max_rows`` rows
    (every level from the tallest group's digests to the root); 0 for an invalid shape."""
    return int(_lib.lib().hades252_mmcs_tree_bytes(max_rows, arity))


def mmcs_open(tree: np.ndarray, max_rows: int, arity: int, indices) -> np.ndarray:
    """``hades252_mmcs_open``: paths [q, depth, arity - 1, 4] for the indices ``indices`` from the tree Mmcs.commit returned.
    Plain host code: no device is touched.  An index >= max_rows gives zeros."""
    where = "mmcs_open"
    depth = _mmcs_depth(where, max_rows, arity)
    nodes = sum(arity ** l for l in range(depth + 1))
    if _host_u64(tree, where).size != nodes * 4:
        raise ValueError("%s: need a tree of %d digests" % (where, nodes))
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    paths = np.zeros((idx.size, depth, arity - 1, 4), dtype=np.uint64)
    check(_lib.lib().hades252_mmcs_open(_ptr(tree), max_rows, arity, _ptr(idx), idx.size, _ptr(paths)), where)
    return paths


def _mmcs_groups(where: str, heights, cols, arity):
    """The group tables of a verification, checked without the library: -> (heights, cols as uint64 arrays, depth)."""
    hs = np.ascontiguousarray(heights, dtype=np.uint64).reshape(-1)
    cs = np.ascontiguousarray(cols, dtype=np.uint64).reshape(-1)
    if not 1 <= hs.size <= _lib.MMCS_MAX_GROUPS or cs.size != hs.size:
        raise ValueError("%s: 1 .. %d groups, one height and one column count each" % (where, _lib.MMCS_MAX_GROUPS))
    depth = _mmcs_depth(where, int(hs[0]), arity)
    for g in range(hs.size):
        if g > 0:
            if not 1 <= int(hs[g]) < int(hs[g - 1]):
                raise ValueError("%s: heights must be strictly decreasing, got %r" % (where, hs.tolist()))
            n = int(hs[g])
            while n > 1 and n % arity == 0:
                n //= arity
            if n != 1:
                raise ValueError("%s: %d is not a power of the arity %d" % (where, int(hs[g]), arity))
        if not 1 <= int(cs[g]) <= 1 << 30:
            raise ValueError("%s: 1 .. 2^30 columns per group, got %d" % (where, int(cs[g])))
    return hs, cs, depth


def mmcs_verify(rows: np.ndarray, heights, cols, indices, paths: np.ndarray, arity: int, capacity_mont: int, tag_mont: int,
                inject_tag_mont: int, pad_mode: int = 1, out_idx: int = 1) -> np.ndarray:
    """``hades252_mmcs_verify``: roots [q, 4] recomputed from the openings of a mixed-height commitment, one launch per chunk
    of queries: ``rows`` [q, sum(cols), 4] holds, per query, the opened rows of all groups concatenated, tallest first;
    ``heights`` / ``cols`` describe the groups (strictly decreasing powers of the arity); ``paths`` [q, depth, arity - 1, 4]
    is what mmcs_open returns.  The caller compares the roots with the one it trusts."""
    where = "mmcs_verify"
    rows, paths = _host_u64(rows, where), _host_u64(paths, where)
    hs, cs, depth = _mmcs_groups(where, heights, cols, arity)
    total = int(cs.sum())
    if rows.ndim != 3 or rows.shape[1:] != (total, 4):
        raise ValueError("%s: rows must have shape [q, %d, 4], got %r" % (where, total, rows.shape))
    q = rows.shape[0]
    if paths.ndim != 4 or paths.shape != (q, depth, arity - 1, 4):
        raise ValueError("%s: paths must have shape [%d, %d, %d, 4], got %r" % (where, q, depth, arity - 1, paths.shape))
    _matrix_modes(where, pad_mode, out_idx)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    if idx.size != q:
        raise ValueError("%s: %d indices for %d openings" % (where, idx.size, q))
    roots = np.zeros((q, 4), dtype=np.uint64)
    check(_lib.lib().hades252_mmcs_verify(_ptr(rows), _ptr(hs), _ptr(cs), hs.size, _ptr(idx), _ptr(paths), q, arity,
                                          _tag_arr(capacity_mont), pad_mode, _tag_arr(tag_mont), _tag_arr(inject_tag_mont),
                                          out_idx, _ptr(roots)), where)
    return roots


def _dev_planes(where: str, part):
    """One device matrix of a commitment: a CUDA int64 tensor [n_cols, plane_stride, 4] (Montgomery limbs), or a pair
    (tensor, n_rows) when only rows 0 .. n_rows - 1 of every plane count; -> (pointer, n_rows, n_cols, stride, device)."""
    t, n_rows = part if isinstance(part, tuple) and len(part) == 2 else (part, None)
    ptr, _, dev = _dev_buffer(t, 32, where)
    import torch
    if t.dtype != torch.int64:
        raise TypeError("%s: planes must be int64 tensors" % where)
    if t.dim() != 3 or t.shape[2] != 4:
        raise ValueError("%s: planes must have shape [n_cols, plane_stride, 4], got %r" % (where, tuple(t.shape)))
    n_cols, stride = int(t.shape[0]), int(t.shape[1])
    n_rows = Mmcs._rows(where, stride if n_rows is None else n_rows)
    if stride < n_rows:
        raise ValueError("%s: planes of %d rows for a group of %d" % (where, stride, n_rows))
    return ptr, n_rows, n_cols, stride, dev


def _dev_rows(where: str, t):
    """One ROW-MAJOR device matrix of a commitment: a CUDA int64 tensor [n_rows, n_cols, 4] (Montgomery limbs) whose scalars
    are whole (stride(1) == 4, stride(2) == 1) and whose rows may lie further apart than their width -- a narrowed view
    ``wide[:, a:b]`` -- with stride(0) // 4 the row stride; -> (pointer, n_rows, n_cols, stride, device)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise TypeError("%s: expected a CUDA torch.Tensor" % where)
    if t.dtype != torch.int64:
        raise TypeError("%s: rows must be int64 tensors" % where)
    if t.dim() != 3 or t.shape[2] != 4:
        raise ValueError("%s: rows must have shape [n_rows, n_cols, 4], got %r" % (where, tuple(t.shape)))
    n_rows, n_cols = Mmcs._rows(where, int(t.shape[0])), int(t.shape[1])
    stride = t.stride(0) // 4 if n_rows > 1 else n_cols                # (a single row has no stride to speak of)
    if t.stride(2) != 1 or (n_cols > 1 and t.stride(1) != 4) or (n_rows > 1 and (t.stride(0) % 4 or stride < n_cols)):
        raise ValueError("%s: rows of whole scalars side by side, a whole number of scalars apart; got strides %r" % (where, t.stride()))
    if n_cols and t.data_ptr() % 16 != 0:
        raise ValueError("%s: buffer must be 16-byte aligned" % where)
    return t.data_ptr(), n_rows, n_cols, stride, t.device


def _dev_parts(where: str, parts, layouts=None):
    """The four host arrays hades252_dmmcs_absorb / _open take for ``parts`` (all on one device); -> (arrays, device).  With
    ``layouts`` (one of _lib.LAYOUT_COLS / _lib.LAYOUT_ROWS per part: the part is what _dev_planes / _dev_rows takes) a
    fifth array, uint32, for the ``_ex`` forms."""
    if not isinstance(parts, (list, tuple)) or not 1 <= len(parts) <= _lib.MMCS_MAX_GROUPS:
        raise ValueError("%s: a list of 1 .. %d parts" % (where, _lib.MMCS_MAX_GROUPS))
    if layouts is None:
        got = [_dev_planes(where, part) for part in parts]
    else:
        if not isinstance(layouts, (list, tuple)) or len(layouts) != len(parts) or \
                any(isinstance(l, bool) or l not in (_lib.LAYOUT_COLS, _lib.LAYOUT_ROWS) for l in layouts):
            raise ValueError("%s: layouts is one of LAYOUT_COLS (0) / LAYOUT_ROWS (1) per part, got %r" % (where, layouts))
        got = [(_dev_rows if l == _lib.LAYOUT_ROWS else _dev_planes)(where, part) for part, l in zip(parts, layouts)]
    _same_device(where, got[0][4], *[g[4] for g in got[1:]])
    arrays = [np.array([g[k] for g in got], dtype=np.uint64) for k in range(4)]
    if layouts is not None:
        arrays.append(np.array(layouts, dtype=np.uint32))
    return arrays, got[0][4]


def _mmcs_openings_dev(where: str, rows_t, heights, cols, indices_t, paths_t, arity, pad_mode, out_idx):
    """The openings of a batch on DEVICE tensors, checked without the library: -> (the first eight arguments of
    hades252_dmmcs_verify and its witness forms -- rows up to arity --, q, device, the (heights, cols) arrays they point to)."""
    rptr, n_row_scalars, dev = _dev_buffer(rows_t, 32, where)
    pptr, _, pdev = _dev_buffer(paths_t, 32, where)
    iptr, q, idev = _dev_buffer(indices_t, 8, where)
    _same_device(where, dev, pdev, idev)
    hs, cs, depth = _mmcs_groups(where, heights, cols, arity)
    total = int(cs.sum())
    if tuple(rows_t.shape) != (q, total, 4) or rows_t.element_size() != 8:
        raise ValueError("%s: rows must be 8-byte words of shape [%d, %d, 4], got %r" % (where, q, total, tuple(rows_t.shape)))
    if tuple(paths_t.shape) != (q, depth, arity - 1, 4) or paths_t.element_size() != 8:
        raise ValueError("%s: paths must be 8-byte words of shape [%d, %d, %d, 4], got %r"
                         % (where, q, depth, arity - 1, tuple(paths_t.shape)))
    if indices_t.dim() != 1 or indices_t.element_size() != 8:
        raise ValueError("%s: indices must be %d 8-byte words" % (where, q))
    _matrix_modes(where, pad_mode, out_idx)
    return (rptr, _ptr(hs), _ptr(cs), hs.size, iptr, pptr, q, arity), q, dev, (hs, cs)


def mmcs_verify_dev(rows_t, heights, cols, indices_t, paths_t, arity: int, capacity_mont: int, tag_mont: int,
                    inject_tag_mont: int, pad_mode: int = 1, out_idx: int = 1):
    """``hades252_dmmcs_verify``: mmcs_verify on DEVICE tensors, one launch on the current stream: ``rows_t`` int64
    [q, sum(cols), 4], ``indices_t`` int64 [q], ``paths_t`` int64 [q, depth, arity - 1, 4] (what Mmcs.open_dev returns);
    ``heights`` / ``cols`` stay host sequences.  -> roots int64 [q, 4] on that device; nothing is synchronised."""
    where = "mmcs_verify_dev"
    front, q, dev, _keep = _mmcs_openings_dev(where, rows_t, heights, cols, indices_t, paths_t, arity, pad_mode, out_idx)
    roots = _dev_empty(dev, q, 4)
    _dev_call(where, dev, "hades252_dmmcs_verify", *front, _tag_arr(capacity_mont), pad_mode, _tag_arr(tag_mont),
              _tag_arr(inject_tag_mont), out_idx, roots.data_ptr())
    return roots


def mmcs_perms(heights, cols, arity: int, pad_mode: int = 1) -> int:
    """``hades252_wmmcs_perms``: permutations of one opening's chain -- the groups' sponge blocks, the levels and the
    injections -- for the shape ``mmcs_verify`` takes."""
    where = "mmcs_perms"
    hs, cs, _ = _mmcs_groups(where, heights, cols, arity)
    _matrix_modes(where, pad_mode)
    return int(_lib.lib().hades252_wmmcs_perms(_ptr(hs), _ptr(cs), hs.size, arity, pad_mode))


def mmcs_steps(heights, cols, arity: int, pad_mode: int = 1) -> np.ndarray:
    """``hades252_wmmcs_steps``: the chain of one opening as data, uint32 [P, 3]: (kind, group, ordinal) of every step, kind
    one of _lib.WMMCS_SPONGE / WMMCS_INJECT / WMMCS_CLIMB, ordinal the block of the group's row, the child level counted from
    the leaves, or 0 for an injection."""
    where = "mmcs_steps"
    hs, cs, _ = _mmcs_groups(where, heights, cols, arity)
    _matrix_modes(where, pad_mode)
    steps = np.zeros((mmcs_perms(hs, cs, arity, pad_mode), 3), dtype=np.uint32)
    check(_lib.lib().hades252_wmmcs_steps(_ptr(hs), _ptr(cs), hs.size, arity, pad_mode, _ptr(steps), steps.shape[0]), where)
    return steps


def mmcs_inputs_dev(rows_t, heights, cols, indices_t, paths_t, arity: int, capacity_mont: int, tag_mont: int,
                    inject_tag_mont: int, pad_mode: int = 1, out_idx: int = 1):
    """``hades252_wmmcs_inputs``: the state that enters every permutation of the chains mmcs_verify_dev walks, one launch on
    the current stream; the arguments are mmcs_verify_dev's.  -> (inputs int64 [P, q, 5, 4], roots int64 [q, 4]) with P =
    mmcs_perms(...): inputs[t, i] enters step t of opening i, roots are mmcs_verify_dev's."""
    where = "mmcs_inputs_dev"
    front, q, dev, (hs, cs) = _mmcs_openings_dev(where, rows_t, heights, cols, indices_t, paths_t, arity, pad_mode, out_idx)
    inputs = _dev_empty(dev, mmcs_perms(hs, cs, arity, pad_mode), q, WIDTH, 4)
    roots = _dev_empty(dev, q, 4)
    _dev_call(where, dev, "hades252_wmmcs_inputs", *front, _tag_arr(capacity_mont), pad_mode, _tag_arr(tag_mont),
              _tag_arr(inject_tag_mont), out_idx, inputs.data_ptr(), roots.data_ptr())
    return inputs, roots


def mmcs_witness_dev(rows_t, heights, cols, indices_t, paths_t, arity: int, capacity_mont: int, tag_mont: int,
                     inject_tag_mont: int, pad_mode: int = 1, out_idx: int = 1):
    """``hades252_wmmcs_witness``: gadget witness of the openings mmcs_verify_dev verifies.  -> (wires int64 [972, P, q, 4],
    inputs int64 [P, q, 5, 4], roots int64 [q, 4]): wires.reshape(972, P * q, 4) == perm_witness(inputs) byte for byte, and
    r2[out_idx] of the last step's records is the roots."""
    where = "mmcs_witness_dev"
    front, q, dev, (hs, cs) = _mmcs_openings_dev(where, rows_t, heights, cols, indices_t, paths_t, arity, pad_mode, out_idx)
    wires, inputs = _witness_pair(dev, mmcs_perms(hs, cs, arity, pad_mode), q)
    roots = _dev_empty(dev, q, 4)
    _dev_call(where, dev, "hades252_wmmcs_witness", *front, _tag_arr(capacity_mont), pad_mode, _tag_arr(tag_mont),
              _tag_arr(inject_tag_mont), out_idx, inputs.data_ptr(), wires.data_ptr(), roots.data_ptr())
    return wires, inputs, roots


class _DeviceWords:
    """Device memory the library owns, as torch.as_tensor reads it (the CUDA array interface): int64 [n, 4]."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n, 4), "typestr": "<i8", "data": (ptr, False), "version": 2}


class Mmcs:
    """``hades252_mmcs_*``: ONE commitment to several column-major matrices of different heights.  The tree sits over the
    tallest matrix's row digests and the row digests of each shorter matrix are hashed into the level whose size equals its
    height: one root, one path per query.  ``absorb`` feeds the group of the planes' height (created at first use; calls for
    different heights interleave freely), ``commit`` is non-destructive.  HOST numpy arrays in and out; a context manager::

        with Mmcs(capacity_mont) as mc:
            mc.absorb(trace)                  # uint64 [g, plane_stride, 4]; n_rows defaults to plane_stride
            mc.absorb(quotient)               # another height
            tree, root = mc.commit(arity, tag_mont, inject_tag_mont)
    """

    def __init__(self, capacity_mont: int):
        self._h = None
        h = ctypes.c_void_p()
        check(_lib.lib().hades252_mmcs_new(ctypes.byref(h), _tag_arr(capacity_mont)), "Mmcs")
        self._h = h
        self._heights = []

    def _handle(self, where: str):
        if self._h is None:
            raise ValueError("%s: the commitment is closed" % where)
        return self._h

    @staticmethod
    def _rows(where: str, n_rows):
        if not isinstance(n_rows, int) or isinstance(n_rows, bool) or not 1 <= n_rows <= 1 << 30:
            raise ValueError("%s: n_rows must be 1 .. 2^30, got %r" % (where, n_rows))
        return n_rows

    def absorb(self, planes: np.ndarray, n_rows: int | None = None) -> "Mmcs":
        """The next columns of the group of height ``n_rows`` (default: the planes' stride): ``planes`` uint64
        [g, plane_stride, 4] (Montgomery limbs), rows 0 .. n_rows - 1 of every plane.  Synchronous; g = 0 is a no-op."""
        where = "Mmcs.absorb"
        h = self._handle(where)
        n_cols, stride = _planes_shape(where, planes)
        n_rows = self._rows(where, stride if n_rows is None else n_rows)
        if stride < n_rows:
            raise ValueError("%s: planes of %d rows for a group of %d" % (where, stride, n_rows))
        if n_cols and n_rows not in self._heights and len(self._heights) == _lib.MMCS_MAX_GROUPS:
            raise ValueError("%s: at most %d distinct heights" % (where, _lib.MMCS_MAX_GROUPS))
        check(_lib.lib().hades252_mmcs_absorb(h, _ptr(planes), n_rows, n_cols, stride), where)
        if n_cols and n_rows not in self._heights:
            self._heights.append(n_rows)
        return self

    def absorb_rows(self, rows: np.ndarray, n_cols: int | None = None) -> "Mmcs":
        """``hades252_rmmcs_absorb_rows``: the next columns of the group of height n_rows from a ROW-major matrix: ``rows``
        uint64 [n_rows, row_stride, 4] (Montgomery limbs), columns 0 .. n_cols - 1 of every row (default: all row_stride).
        Synchronous; n_cols = 0 is a no-op.  No transpose is made anywhere."""
        where = "Mmcs.absorb_rows"
        h = self._handle(where)
        rows = _host_u64(rows, where)
        if rows.ndim != 3 or rows.shape[2] != 4:
            raise ValueError("%s: rows must have shape [n_rows, row_stride, 4], got %r" % (where, rows.shape))
        n_rows, stride = self._rows(where, rows.shape[0]), rows.shape[1]
        if n_cols is None:
            n_cols = stride
        if not isinstance(n_cols, int) or isinstance(n_cols, bool) or not 0 <= n_cols <= stride:
            raise ValueError("%s: n_cols must be 0 .. row_stride = %d, got %r" % (where, stride, n_cols))
        if n_cols and n_rows not in self._heights and len(self._heights) == _lib.MMCS_MAX_GROUPS:
            raise ValueError("%s: at most %d distinct heights" % (where, _lib.MMCS_MAX_GROUPS))
        check(_lib.lib().hades252_rmmcs_absorb_rows(h, _ptr(rows), n_rows, n_cols, stride), where)
        if n_cols and n_rows not in self._heights:
            self._heights.append(n_rows)
        return self

    def cols(self, n_rows: int) -> int:
        """Columns absorbed so far for the height ``n_rows``; 0: no such group."""
        where = "Mmcs.cols"
        h, n_rows, n = self._handle(where), self._rows(where, n_rows), ctypes.c_uint64()
        check(_lib.lib().hades252_mmcs_cols(h, n_rows, ctypes.byref(n)), where)
        return int(n.value)

    @property
    def heights(self):
        """The groups' heights, tallest first."""
        return sorted(self._heights, reverse=True)

    def commit(self, arity: int, tag_mont: int, inject_tag_mont: int, pad_mode: int = 1, out_idx: int = 1,
               want_tree: bool = True):
        """(tree [nodes, 4] or None, root [4]) of everything absorbed so far: every level from the tallest group's row
        digests to the root, after the injections; the commitment is left as it is."""
        where = "Mmcs.commit"
        h = self._handle(where)
        if not self._heights:
            raise ValueError("%s: nothing absorbed yet" % where)
        depth = _mmcs_depth(where, max(self._heights), arity)
        for n in self._heights:
            if n > 1:                                                    # (a group of one row sits at the root)
                _mmcs_depth(where, n, arity)
        _matrix_modes(where, pad_mode, out_idx)
        tree = np.zeros((sum(arity ** l for l in range(depth + 1)), 4), dtype=np.uint64) if want_tree else None
        root = np.zeros(4, dtype=np.uint64)
        check(_lib.lib().hades252_mmcs_commit(h, pad_mode, arity, _tag_arr(tag_mont), _tag_arr(inject_tag_mont), out_idx,
                                              None if tree is None else _ptr(tree), _ptr(root)), where)
        return tree, root

    # ---- device memory (include/hades252.h, f15).  Everything below is enqueued on torch's current stream of the tensors'
    # device and returns at once.  The library orders nothing between that stream and the streams absorb / commit / close
    # run on: synchronise the stream before calling one of those on this commitment.
    def absorb_dev(self, parts, layouts=None) -> "Mmcs":
        """``hades252_dmmcs_absorb``: every part of ``parts`` -- a CUDA int64 tensor [g, plane_stride, 4] or a pair
        (tensor, n_rows) -- is the next g columns of the group of its height; the heights are distinct and all parts run as
        ONE launch.  A part with g = 0 is skipped.  With ``layouts`` (``hades252_rmmcs_absorb_ex``: LAYOUT_COLS or
        LAYOUT_ROWS per part) a LAYOUT_ROWS part is a ROW-major matrix: a CUDA int64 tensor [n_rows, g, 4], possibly a
        narrowed view of wider rows (stride(0) // 4 is its row stride, stride(1) == 4, stride(2) == 1)."""
        where = "Mmcs.absorb_dev"
        h = self._handle(where)
        (ptrs, rows, cols, strides, *lay), dev = _dev_parts(where, parts, layouts)
        live = [int(r) for r, c in zip(rows, cols) if c]
        if len(set(live)) != len(live):
            raise ValueError("%s: the heights of one call must be distinct, got %r" % (where, rows.tolist()))
        if len(set(live) | set(self._heights)) > _lib.MMCS_MAX_GROUPS:
            raise ValueError("%s: at most %d distinct heights" % (where, _lib.MMCS_MAX_GROUPS))
        if lay:
            _dev_call(where, dev, "hades252_rmmcs_absorb_ex", h, _ptr(ptrs), _ptr(rows), _ptr(cols), _ptr(strides), _ptr(lay[0]), len(parts))
        else:
            _dev_call(where, dev, "hades252_dmmcs_absorb", h, _ptr(ptrs), _ptr(rows), _ptr(cols), _ptr(strides), len(parts))
        self._heights += [r for r in live if r not in self._heights]
        return self

    def tree_dev(self, device=None):
        """``hades252_dmmcs_tree``: a copy of the device tree of the last commit, int64 [nodes, 4] (the root is its last row),
        made on the current stream of ``device`` (default: the current device) -> (tree, arity)."""
        where = "Mmcs.tree_dev"
        h = self._handle(where)
        ptr, n_bytes, arity = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
        check(_lib.lib().hades252_dmmcs_tree(h, ctypes.byref(ptr), ctypes.byref(n_bytes), ctypes.byref(arity)), where)
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return torch.as_tensor(_DeviceWords(ptr.value, n_bytes.value // 32), device=dev).clone(), int(arity.value)

    def open_dev(self, parts, indices_t, layouts=None):
        """``hades252_dmmcs_open``: (rows int64 [q, sum of the parts' columns, 4], paths int64 [q, depth, arity - 1, 4]) of the
        indices ``indices_t`` (CUDA int64 [q]) from the committed matrices ``parts`` (as absorb_dev takes them, tallest
        first) and the tree of the last commit: what mmcs_verify_dev reads.  An index >= the tallest height gives zeros.
        With ``layouts`` (``hades252_rmmcs_open_ex``) a LAYOUT_ROWS part is a row-major matrix, as in absorb_dev."""
        where = "Mmcs.open_dev"
        h = self._handle(where)
        (ptrs, rows, cols, strides, *lay), dev = _dev_parts(where, parts, layouts)
        iptr, q, idev = _dev_buffer(indices_t, 8, where)
        _same_device(where, dev, idev)
        if indices_t.dim() != 1 or indices_t.element_size() != 8:
            raise ValueError("%s: indices must be a vector of 8-byte words" % where)
        hs = [int(r) for r in rows]
        if any(a <= b for a, b in zip(hs, hs[1:])) or any(r not in self._heights for r in hs) or not cols.all():
            raise ValueError("%s: the parts are groups of the commitment with columns, tallest first; got heights %r" % (where, hs))
        ptr, n_bytes, arity = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
        check(_lib.lib().hades252_dmmcs_tree(h, ctypes.byref(ptr), ctypes.byref(n_bytes), ctypes.byref(arity)), where)
        depth = _mmcs_depth(where, hs[0], int(arity.value))
        out_rows = _dev_empty(dev, q, int(cols.sum()), 4)
        paths = _dev_empty(dev, q, depth, int(arity.value) - 1, 4)
        if lay:
            _dev_call(where, dev, "hades252_rmmcs_open_ex", h, _ptr(ptrs), _ptr(rows), _ptr(cols), _ptr(strides), _ptr(lay[0]),
                      len(parts), iptr, q, out_rows.data_ptr(), paths.data_ptr())
        else:
            _dev_call(where, dev, "hades252_dmmcs_open", h, _ptr(ptrs), _ptr(rows), _ptr(cols), _ptr(strides), len(parts), iptr, q,
                      out_rows.data_ptr(), paths.data_ptr())
        return out_rows, paths

    def close(self) -> None:
        """Frees what the commitment holds on the device; closing twice is fine."""
        h, self._h = self._h, None
        if h is not None:
            _lib.lib().hades252_mmcs_free(h)

    def __enter__(self) -> "Mmcs":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GEN_SEED = 0x4861646573323532


def gen_b(n_elems: int, device, first_elem: int = 0, seed: int = GEN_SEED, out=None):
    """Generator B on device: n_elems scalars starting at global element index."""
    out = _dev_empty(device, n_elems, 4) if out is None else out
    _dev_call("gen_b", out.device, "hades252_gen_b_dev", out.data_ptr(), first_elem, n_elems, seed)
    return out


def gen_a(n_elems: int, device, first_elem: int = 0):
    out = _dev_empty(device, n_elems, 4)
    _dev_call("gen_a", out.device, "hades252_gen_a_dev", out.data_ptr(), first_elem, n_elems)
    return out


def digest(t, first_index: int = 0):
    """256-bit position-sensitive digest of a device buffer (4 python ints)."""
    ptr, n, dev = _dev_buffer(t, 8, "digest")
    out = _dev_empty(dev, 4)
    _dev_call("digest", dev, "hades252_digest_dev", ptr, first_index, n, out.data_ptr())
    return [int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().tolist()]
