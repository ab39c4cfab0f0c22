"""Build libhades252.so (the HIP kernels + C ABI) in-tree with hipcc for gfx950.

    python -m hades252_amd.build [--force]

The library is built into ``hades252_amd/csrc/libhades252.so`` so that it travels with the source
tree (it is git-ignored).  hipcc cross-compiles without a GPU.

Staleness is decided by a content hash of the sources (kept in ``libhades252.so.stamp``), not by
mtimes -- a copied tree does not preserve them.  Builds are serialised with a file lock and the
library is replaced atomically, so several ranks of one job may call ``build()`` at once.
"""
from __future__ import annotations

import fcntl
import hashlib
import os
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libhades252.so")
STAMP = LIB + ".stamp"
LOCK = LIB + ".lock"
SOURCES = ["hades252.hip"]
# device code: arithmetic, kernels, generated tables
DEVICE_DEPS = ["fr32.hpp", "staging.hpp", "hades_literal.hpp", "hades_fast.hpp", "k_perm_fast.hpp", "hades_coop.hpp", "hades_lanes.hpp",
               "device_tables.hpp", "kernels_perm.hpp", "kernels_merkle.hpp", "kernels_sponge.hpp", "kernels_aux.hpp",
               "hades_constants.inc"]
# host code that decides WHAT is launched and with which geometry / LDS / level-fusion policy: a kernel's traffic per launch
# and the launches that make a tree depend on it
LAUNCH_POLICY_DEPS = ["launch.hpp", "abi_perm.hpp", "abi_merkle.hpp", "abi_sponge.hpp"]
# kernels (and their launchers) that no committed counter record covers: the batched cipher, the duplex sponge, the chain witnesses.  They are rebuilt like every
# other source (DEPS) but stay out of device_source_hash: they neither define nor launch any kernel of the
# `secondary_kernels` record, so an edit of them cannot change that record's traffic and must not drop it from bench.py.
# A kernel that gets a counter record of its own moves to DEVICE_DEPS / LAUNCH_POLICY_DEPS with it.
UNRECORDED_KERNEL_DEPS = ["kernels_cipher.hpp", "abi_cipher.hpp", "kernels_safe.hpp", "abi_safe.hpp", "kernels_witness.hpp", "abi_witness.hpp"]
# host plumbing (error / fault hook, page-locked memory, pipe pool, chunk pipeline, one-shot host callers, generators)
HOST_DEPS = ["hades252.hip", "host_fault.hpp", "abi_util.hpp", "host_pin.hpp", "host_pool.hpp", "host_pipe.hpp", "host_callers.hpp", "host_cipher.hpp", "host_safe.hpp"]
# proof-of-work grinding: a kernel and its host loop that the host simulation does not run yet (its driver includes every file
# of the three lists above, and would have to change), and that no committed counter record covers: rebuilt like every other
# source (DEPS), outside device_source_hash and perm_fast_hash
GRIND_DEPS = ["kernels_grind.hpp", "host_grind.hpp"]
# the inverse permutation and the fifth roots: kernels, their generated tables and their host loop, host pointers only.  No
# committed counter record covers them and no other kernel includes them: rebuilt like every other source (DEPS), outside
# device_source_hash and perm_fast_hash.  The host simulation runs them from a driver of their own (tests/hostsim_inverse).
INVERSE_DEPS = ["kernels_inverse.hpp", "hades_inverse_constants.inc", "host_inverse.hpp"]
# matrix commitments (row hashes of a column-major matrix, the tree over them, openings, verification): one kernel and its
# host calls, host pointers only.  No committed counter record covers them and no other kernel includes them: rebuilt like
# every other source (DEPS), outside device_source_hash and perm_fast_hash.  The host simulation runs the kernel from a
# driver of its own (tests/hostsim_matrix).
MATRIX_DEPS = ["kernels_matrix.hpp", "host_matrix.hpp"]
# streaming matrix commitments (the row sponges stay resident on the device, the matrix arrives a group of columns at a
# time): their kernels and host calls, host pointers only.  As MATRIX_DEPS: rebuilt like every other source (DEPS), outside
# device_source_hash and perm_fast_hash.  The host simulation runs the kernels from a driver of its own
# (tests/hostsim_matrix_stream).
MATRIX_STREAM_DEPS = ["kernels_matrix_stream.hpp", "host_matrix_stream.hpp"]
# mixed-height matrix commitments (several matrices of different heights under one tree, whole openings verified in one
# launch): their kernels and host calls, host pointers only, on top of the streams of MATRIX_STREAM_DEPS.  As those: rebuilt
# like every other source (DEPS), outside device_source_hash and perm_fast_hash.  The host simulation runs the kernels from
# a driver of its own (tests/hostsim_mmcs).
MMCS_DEPS = ["kernels_mmcs.hpp", "host_mmcs.hpp"]
# device-resident mixed-height commitments (the handle of MMCS_DEPS fed, opened and verified from device memory on the
# caller's stream): two kernels and their host calls.  As MMCS_DEPS: rebuilt like every other source (DEPS), outside
# device_source_hash and perm_fast_hash.  The host simulation runs the kernels from a driver of its own
# (tests/hostsim_dmmcs).
DMMCS_DEPS = ["kernels_dmmcs.hpp", "abi_dmmcs.hpp"]
# row-major matrices for the commitments of MMCS_DEPS / DMMCS_DEPS (a layout per matrix, device and host form): two kernels
# and their host calls, beside those of DMMCS_DEPS, which keep their own.  As DMMCS_DEPS: rebuilt like every other source
# (DEPS), outside device_source_hash and perm_fast_hash.  The host simulation runs the kernels from a driver of its own
# (tests/hostsim_rowmajor).
ROWMAJOR_DEPS = ["kernels_rowmajor.hpp", "abi_rowmajor.hpp", "host_rowmajor.hpp"]
# gadget witnesses of the openings of the commitments of MMCS_DEPS (the input state of every permutation of a verification's
# chain, then the wires of k_perm_witness): one kernel and its host calls.  As DMMCS_DEPS: rebuilt like every other source
# (DEPS), outside device_source_hash and perm_fast_hash.  The host simulation runs the kernel from a driver of its own
# (tests/hostsim_wmmcs).
WMMCS_DEPS = ["kernels_wmmcs.hpp", "abi_wmmcs.hpp"]
DEPS = HOST_DEPS + LAUNCH_POLICY_DEPS + DEVICE_DEPS + UNRECORDED_KERNEL_DEPS + GRIND_DEPS + INVERSE_DEPS + MATRIX_DEPS + MATRIX_STREAM_DEPS + MMCS_DEPS + DMMCS_DEPS + ROWMAJOR_DEPS + WMMCS_DEPS + [os.path.join("..", "..", "include", "hades252.h")]
# what the dominant kernel (k_perm_fast) is made of: profiles recorded for it stay valid while these are unchanged
PERM_FAST_DEPS = ["fr32.hpp", "staging.hpp", "hades_fast.hpp", "k_perm_fast.hpp"]
# ... plus these tables of hades_constants.inc (other kernels' tables may change without touching k_perm_fast)
PERM_FAST_TABLES = ("HADES_FAST_L", "HADES_FAST_MDS_SMALL", "HADES_NEG_P29", "HADES_TWO_P29", "HADES_P29", "HADES_FAST_ROUND_INIT",
                    "HADES_FAST_FINAL_F", "HADES_FAST_LIN_INIT", "HADES_FAST_FINAL_LIN")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", "-pthread",
         "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]


def source_hash() -> str:
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for d in DEPS:
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(d.encode() + b"\0" + f.read())
    return h.hexdigest()


def perm_fast_hash() -> str:
    """Hash of the sources + flags that determine k_perm_fast (keys committed PMC profiles to the kernel)."""
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for d in PERM_FAST_DEPS:
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(d.encode() + b"\0" + f.read())
    keep = False
    with open(os.path.join(CSRC, "hades_constants.inc")) as f:
        for line in f:
            if line.startswith("#define "):
                keep = line.split()[1] in PERM_FAST_TABLES
            if keep:
                h.update(line.encode())
                keep = line.rstrip().endswith("\\")
    return h.hexdigest()


def device_source_hash() -> str:
    """Hash of everything that determines what a launch (or a tree build: a SEQUENCE of launches) moves through HBM: the
    device code of every kernel (kernel headers, generated tables, flags) AND the host code that picks kernels, grids, LDS
    sizes and the level / fusion policy of a tree (launch.hpp, abi_*.hpp) -- not the host plumbing (pools, pipes, page
    locking, the fault hook), whose edits leave traffic per launch as it was.  Keys the committed counter records of the
    kernels other than k_perm_fast (profiles/hbm_traffic.json `secondary_kernels`)."""
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for d in sorted(DEVICE_DEPS + LAUNCH_POLICY_DEPS):
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(d.encode() + b"\0" + f.read())
    return h.hexdigest()


def _fresh(lib: str, want: str) -> bool:
    stamp = lib + ".stamp"
    if not (os.path.exists(lib) and os.path.exists(stamp)):
        return False
    with open(stamp) as f:
        return f.read().strip() == want


def compile_so(lib: str, sources, want: str, cwd: str, force: bool = False, verbose: bool = True) -> str:
    """hipcc FLAGS + sources -> lib (run in cwd), unless lib.stamp already holds `want`.  Serialised with lib.lock;
    the library and then its stamp are replaced atomically, so concurrent callers never load a half-written file."""
    if not force and _fresh(lib, want):
        return lib
    with open(lib + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and _fresh(lib, want):     # another process built it while we waited
                return lib
            tmp = lib + ".tmp.%d" % os.getpid()
            cmd = [HIPCC] + FLAGS + ["-o", tmp] + list(sources)
            if verbose:
                print("[hades252_amd.build]", " ".join(cmd), flush=True)
            subprocess.run(cmd, cwd=cwd, check=True)
            os.replace(tmp, lib)
            with open(lib + ".stamp.tmp", "w") as f:
                f.write(want + "\n")
            os.replace(lib + ".stamp.tmp", lib + ".stamp")
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return lib


def build(force: bool = False, verbose: bool = True) -> str:
    return compile_so(LIB, SOURCES, source_hash(), CSRC, force=force, verbose=verbose)


# ---- native measurement tool of the host-pointer boundary (tools/host_path_bench.cpp) -------------------------
# A plain C++ caller of the C ABI, linked against the SYSTEM HIP runtime like a Rust / C host would be (a PyTorch
# process loads PyTorch's own bundled runtime, under which the same pipeline overlaps its copies far worse).
ROOT = os.path.dirname(os.path.dirname(CSRC))
TOOL_SRC = os.path.join(ROOT, "tools", "host_path_bench.cpp")
TOOL_BIN = os.path.join(ROOT, "build_tools", "host_path_bench")


def build_host_path_bench(verbose: bool = True) -> str:
    build(verbose=verbose)
    h = hashlib.sha256()
    for f in (TOOL_SRC, os.path.join(ROOT, "include", "hades252.h")):
        with open(f, "rb") as fh:
            h.update(fh.read())
    want = h.hexdigest()
    stamp = TOOL_BIN + ".stamp"
    os.makedirs(os.path.dirname(TOOL_BIN), exist_ok=True)
    if os.path.exists(TOOL_BIN) and os.path.exists(stamp) and open(stamp).read().strip() == want:
        return TOOL_BIN
    with open(LOCK, "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            tmp = TOOL_BIN + ".tmp.%d" % os.getpid()
            cmd = [HIPCC, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", tmp, TOOL_SRC, "-L" + CSRC,
                   "-lhades252", "-Wl,-rpath,$ORIGIN/../hades252_amd/csrc"]
            if verbose:
                print("[hades252_amd.build]", " ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
            os.replace(tmp, TOOL_BIN)
            with open(stamp, "w") as f:
                f.write(want + "\n")
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return TOOL_BIN


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_host_path_bench()
    print(LIB)
